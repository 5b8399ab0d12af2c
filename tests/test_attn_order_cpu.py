"""CPU tier of use_new_attention_order (QKVAttention, openaimodel.py:401-428): the constructor against what the reference's gave
(tests/golden/make_golden_attn_order.py: parameter count, state-dict names and shapes - the same in both orders, which is why a swapped
layout gives a wrong picture and no error), the layout helpers of tests/refs_attn_order.py, and their restatement of QKVAttention against
the reference's module itself (fixture f33_qkvattention) and against the double-precision reference of tests/refs_attn.py."""
import json
import os

import numpy as np
import pytest
import torch

from tests import refs_attn as R
from tests import refs_attn_order as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(image_size=16, in_channels=7, model_channels=32, out_channels=4, num_res_blocks=2,
            attention_resolutions=[32, 16, 8], channel_mult=[1, 2, 4], num_heads=4)
torch.set_grad_enabled(False)


def _names():
    with open(os.path.join(ROOT, "tests", "golden", "f33_unet_neworder_names.json")) as f:
        return {k: tuple(v) for k, v in json.load(f).items()}


# ------------------------------------------------------------------------------------------------ the model
def test_new_attention_order_constructs_with_the_references_state_dict(golden):
    from stedm_amd import ops
    from stedm_amd.unet import AttentionBlock, UNetModel
    m = UNetModel(use_new_attention_order=True, **TINY)
    legacy = UNetModel(**TINY)
    for tag in ("neworder_tiny", "neworder_t64", "neworder_nhc_tiny"):
        assert sum(p.numel() for p in m.parameters()) == int(golden(f"f33_unet_{tag}")["n_params"]) == 3922660
    sd = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert sd == _names() and list(m.state_dict()) == list(_names()), "the reference's names, shapes and order"
    assert sd == {k: tuple(v.shape) for k, v in legacy.state_dict().items()}, "the state dict does not tell the orders apart"
    ab = m.middle_block[2]
    assert isinstance(ab, AttentionBlock) and ab.attn_order == ops.ATTN_QKV_FIRST == 1 and ab.num_heads == 4
    assert legacy.middle_block[2].attn_order == ops.ATTN_HEADS_FIRST == 0
    assert [n for n, l in m.named_modules() if isinstance(l, AttentionBlock)] == ["middle_block.2"], "the level attentions do not exist"
    nhc = UNetModel(use_new_attention_order=True, **dict(TINY, num_heads=-1, num_head_channels=64))
    assert nhc.middle_block[2].num_heads == 2 and nhc.middle_block[2].attn_order == 1
    assert {k: tuple(v.shape) for k, v in nhc.state_dict().items()} == _names()


def test_attention_block_records_the_order():
    from stedm_amd.unet import AttentionBlock
    new, old = AttentionBlock(128, 4, use_new_attention_order=True), AttentionBlock(128, 4)
    assert (new.attn_order, old.attn_order) == (1, 0) and new.num_heads == old.num_heads == 4
    assert {k: tuple(v.shape) for k, v in new.state_dict().items()} == {k: tuple(v.shape) for k, v in old.state_dict().items()}
    assert set(new.state_dict()) == {"norm.weight", "norm.bias", "qkv.weight", "qkv.bias", "proj_out.weight", "proj_out.bias"}
    assert AttentionBlock(128, num_head_channels=64, use_new_attention_order=True).num_heads == 2
    assert old.order_kw() == {} and new.order_kw() == {"order": 1}, "the default order calls the ops with their original arguments"


def test_spatial_transformer_ignores_the_order():
    """with use_spatial_transformer=True the reference builds no AttentionBlock, so the flag changes nothing (openaimodel.py:627-640)"""
    from stedm_amd.unet import AttentionBlock, UNetModel
    kw = dict(TINY, use_spatial_transformer=True, context_dim=128)
    a, b = UNetModel(use_new_attention_order=True, **kw), UNetModel(**kw)
    assert not any(isinstance(l, AttentionBlock) for l in a.modules())
    assert [(n, type(l)) for n, l in a.named_modules()] == [(n, type(l)) for n, l in b.named_modules()]
    assert {k: tuple(v.shape) for k, v in a.state_dict().items()} == {k: tuple(v.shape) for k, v in b.state_dict().items()}
    assert not any(hasattr(l, "attn_order") for l in a.modules())


def test_fixtures_keep_the_orders_apart(golden):
    """the outputs of the two orders on the same weights differ by more than twice the loosest mode threshold (bf16: 5e-2) in every fixture"""
    for tag in ("neworder_tiny", "neworder_t64", "neworder_nhc_tiny"):
        assert float(golden(f"f33_unet_{tag}")["order_gap"]) > 0.1
    for tag in ("neworder_tiny", "neworder_t64"):
        fx = golden(f"f33_grads_{tag}")
        assert float(fx["order_gap"]) > 0.1 and float(fx["qkv_grad_gap"]) > 0.1


# ------------------------------------------------------------------------------------------------ the layout helpers
CASES = [(2, 5, 3, 8), (1, 36, 2, 16), (3, 7, 1, 4)]


@pytest.mark.parametrize("B,T,heads,ch", CASES)
def test_order_pack_places_every_element_and_round_trips(B, T, heads, ch):
    g = torch.Generator().manual_seed(T + ch)
    q, k, v = (torch.randn(B * heads, T, ch, generator=g, dtype=torch.float64) for _ in range(3))
    C = heads * ch
    p1, p0 = O.order_pack(q, k, v, B, heads), R.legacy_pack(q, k, v, B, heads)
    assert p1.shape == p0.shape == (B, T, 3 * C) and p1.is_contiguous()
    for b in range(B):
        for h in range(heads):
            for i, x in enumerate((q, k, v)):
                assert torch.equal(p1[b, :, i * C + h * ch:i * C + (h + 1) * ch], x[b * heads + h])          # {q: 0, k: C, v: 2C} + h ch + c
                assert torch.equal(p0[b, :, h * 3 * ch + i * ch:h * 3 * ch + (i + 1) * ch], x[b * heads + h])  # h 3ch + {0, ch, 2ch} + c
    for got, want in zip(O.order_unpack(p1, B, heads), (q, k, v)):
        assert torch.equal(got, want)
    for got, want in zip(O.legacy_unpack_qkv(p0, B, heads), (q, k, v)):
        assert torch.equal(got, want)
    assert torch.equal(O.relayout(p0, B, heads, O.QKV_FIRST), p1) and torch.equal(O.relayout(p1, B, heads, O.HEADS_FIRST), p0)
    assert torch.equal(O.pack(1, q, k, v, B, heads), p1) and torch.equal(O.pack(0, q, k, v, B, heads), p0)
    if heads > 1:
        assert not torch.equal(p0, p1)


def test_restatement_equals_the_references_module(golden):
    """f33_qkvattention: the reference's QKVAttention(3) on a random fp32 qkv [2][72][5]"""
    fx = golden("f33_qkvattention")
    qkv, want, heads = torch.from_numpy(fx["qkv"]), torch.from_numpy(fx["out"]), int(fx["heads"])
    got = O.qkv_attention_new(qkv, heads)
    err = float((got - want).abs().max())
    print(f"restatement vs the reference's module: max |diff| {err:.2e} (|out| max {float(want.abs().max()):.2f})")
    assert got.shape == want.shape and err < 2e-6            # fp32 on both sides, another order of the sums
    from oracle.unet import qkv_attention_legacy
    assert float((qkv_attention_legacy(qkv, heads) - want).abs().max()) > 1e-2, "the legacy split of the same plane is another function"


@pytest.mark.parametrize("B,T,heads,ch", [(2, 36, 2, 16), (1, 100, 3, 64)])
def test_order_pack_feeds_the_new_order_what_legacy_pack_feeds_the_legacy_one(B, T, heads, ch):
    """on unrounded inputs: QKVAttention on order_pack(q, k, v) = QKVAttentionLegacy on legacy_pack(q, k, v) = refs_attn.legacy_ref(q, k, v)
    (the output plane has channel = head * ch + c in both orders)"""
    from oracle.unet import qkv_attention_legacy
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(B * heads, T, ch, generator=g, dtype=torch.float64) for _ in range(3))
    new = O.qkv_attention_new(O.order_pack(q, k, v, B, heads).transpose(1, 2).contiguous(), heads)             # [B][heads ch][T]
    old = qkv_attention_legacy(R.legacy_pack(q, k, v, B, heads).transpose(1, 2).contiguous(), heads)
    want = R.legacy_ref(q, k, v)["out"]
    e_new = float((R.legacy_unpack(new.transpose(1, 2), B, heads) - want).abs().max())
    e_old = float((R.legacy_unpack(old.transpose(1, 2), B, heads) - want).abs().max())
    assert e_new < 2e-6 and e_old < 2e-6, (e_new, e_old)          # the softmax of both restatements is fp32
    assert float((new - old).abs().max()) < 1e-12                   # and the two are the same arithmetic
    swapped = O.qkv_attention_new(R.legacy_pack(q, k, v, B, heads).transpose(1, 2).contiguous(), heads)
    assert float((swapped - new).abs().max()) > 1e-2, "a plane of the other order must not pass"


def test_binding_declares_the_new_entry_points():
    from stedm_amd import _lib, ops
    assert _lib.ABI_VERSION == 31
    for name, nargs in (("stedm_attn_qkv", 8), ("stedm_attn_qkv16", 10), ("stedm_attn_qkv_bwd", 10)):
        assert len(_lib.SIGNATURES[name][1]) == nargs == len(_lib.SIGNATURES[name.replace("qkv", "legacy")][1]) + 1, "the legacy entry plus `order`"
    with open(os.path.join(ROOT, "include", "stedm_hip.h")) as f:
        h = f.read()
    assert "#define STEDM_ATTN_HEADS_FIRST 0" in h and "#define STEDM_ATTN_QKV_FIRST 1" in h and "#define STEDM_ABI_VERSION 31" in h
    assert (ops.ATTN_HEADS_FIRST, ops.ATTN_QKV_FIRST) == (0, 1)
    import inspect
    for fn in (ops.attn_legacy, ops.attn_legacy16, ops.attn_legacy_bwd):
        assert inspect.signature(fn).parameters["order"].default == 0
