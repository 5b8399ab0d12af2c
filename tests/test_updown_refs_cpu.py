"""CPU tier: the restatement of tests/refs_updown.py against torch's own operators and inside its derived bound, and
UNetModel(resblock_updown=True) against what the reference's constructor gave (tests/golden/make_golden_updown.py: parameter count,
state-dict names and shapes, where the four up / down blocks sit)."""
import json
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import refs_gn as G
from tests import refs_updown as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(image_size=16, in_channels=7, model_channels=32, out_channels=4, num_res_blocks=2,
            attention_resolutions=[32, 16, 8], channel_mult=[1, 2, 4], num_heads=4)


def _nchw(x):
    return x.permute(0, 3, 1, 2)


@pytest.mark.parametrize("case", R.POOL_CASES + R.NEAREST_CASES, ids=R.case_id)
@pytest.mark.parametrize("mode", [R.POOL, R.NEAREST])
def test_restatement_is_torchs_group_norm_silu_resample(case, mode):
    B, H, W, C, groups = case
    if mode == R.POOL and (H % 2 or W % 2):
        with pytest.raises(AssertionError):
            R.resample(torch.zeros(B, H, W, C), mode)
        return
    x, gamma, beta = (v.double() for v in R.inputs(case))
    eps = 1e-5
    mr = G.stats_of(x.view(B, H * W, C), groups, eps)[0]
    for act in (0, 1):
        y, xr = R.gn_resample(x, mr, groups, gamma, beta, act, mode)
        a = F.group_norm(_nchw(x), groups, gamma, beta, eps)
        a = F.silu(a) if act else a
        if mode == R.POOL:
            want, wantx = F.avg_pool2d(a, 2, 2), F.avg_pool2d(_nchw(x), 2, 2)
        else:
            want, wantx = F.interpolate(a, scale_factor=2, mode="nearest"), F.interpolate(_nchw(x), scale_factor=2, mode="nearest")
        assert torch.allclose(_nchw(y), want, rtol=0, atol=1e-12)
        assert torch.allclose(_nchw(xr), wantx, rtol=0, atol=1e-14)
        if mode == R.NEAREST:
            assert torch.equal(_nchw(xr), wantx)


@pytest.mark.parametrize("case", R.POOL_CASES, ids=R.case_id)
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("hilo", [False, True], ids=["hi", "hilo"])
def test_fp32_pool_restatement_stays_inside_the_derived_bound(case, dtype, hilo):
    """the pass in fp32 (the kernel's order of operations, torch's sigmoid for silu_f) against the fp64 restatement on the same statistics:
    err / bound < 1 per element, SiLU on general inputs - the check tests/test_gpu_updown_kernel.py applies to the kernel's planes"""
    B, H, W, C, groups = case
    x, gamma, beta = R.inputs(case)
    eps = 1e-5
    cs = G.chan_partials(x.double()).float()
    mr64 = G.fold(cs, None, 0, groups, H * W, eps)
    y32, _ = R.gn_resample(x, mr64.float(), groups, gamma, beta, 1, R.POOL)
    hi, lo = R.planes(y32, dtype, hilo)
    got = G.planes_value(hi, lo, dtype)
    ref, bound = R.pool_bound(x.double(), mr64, groups, gamma.double(), beta.double(), 1, dtype, hilo)
    r = G.ratio((got - ref).abs(), bound)
    print(f"[{R.case_id(case)} {dtype} hilo={hilo}] worst err / bound {r:.3f}")
    assert r < 1.0
    # ... and the bound is not vacuous: a value off by four roundings of the stored format (u_T, or u_T^2 for hi + lo; at least 16 u, the
    # size of the fp32 terms) leaves it
    off = 4.0 * max(G.u_T(dtype) ** (2 if hilo else 1), 16.0 * G.U)
    assert G.ratio((got * (1.0 + off) - ref).abs(), bound) > 1.0


@pytest.mark.parametrize("case", R.POOL_CASES, ids=R.case_id)
@pytest.mark.parametrize("kind", ["A", "B"])
def test_exact_problem_is_exact_in_both_formats(case, kind):
    for dtype in (torch.float16, torch.bfloat16):
        p = R.exact_problem(case, kind, dtype)
        B, H, W, C, groups = case
        assert torch.equal(G.fold(p["cs"], None, 0, groups, H * W, 0.0).float(), p["mr"])
        assert torch.equal(p["xr"].double(), F.avg_pool2d(_nchw(p["x"].double()), 2, 2).permute(0, 2, 3, 1))


# ------------------------------------------------------------------------------------------------ the model
def _names(tag):
    with open(os.path.join(ROOT, "tests", "golden", f"f32_unet_{tag}_names.json")) as f:
        return {k: tuple(v) for k, v in json.load(f).items()}


UPDOWN_BLOCKS = {"input_blocks.3.0": (32, "down"), "input_blocks.6.0": (64, "down"), "output_blocks.2.1": (128, "up"), "output_blocks.5.1": (64, "up")}


@pytest.mark.parametrize("tag,film,count", [("updown", False, 4191652), ("updown_film", True, 4422820)])
def test_resblock_updown_constructs_with_the_references_state_dict(golden, tag, film, count):
    from stedm_amd.unet import Downsample, ResBlock, UNetModel, Upsample
    fx = golden(f"f32_unet_{tag}_tiny")
    m = UNetModel(resblock_updown=True, use_scale_shift_norm=film, **TINY)
    assert int(fx["n_params"]) == count
    assert sum(p.numel() for p in m.parameters()) == count
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == _names(tag)
    assert list(m.state_dict()) == list(_names(tag)), "the reference's order too"
    assert not any(".op." in k or ".conv." in k for k in m.state_dict()), "no resampling convolution is left"
    mods = dict(m.named_modules())
    found = {n: l for n, l in mods.items() if isinstance(l, ResBlock) and l.updown}
    assert set(found) == set(UPDOWN_BLOCKS)
    for n, (ch, way) in UPDOWN_BLOCKS.items():
        rb = found[n]
        assert rb.channels == ch and rb.out_channels == ch and isinstance(rb.skip_connection, nn.Identity)
        assert rb.up == (way == "up") and rb.down == (way == "down") and rb.use_scale_shift_norm == film
        kind = Upsample if way == "up" else Downsample
        for l in (rb.h_upd, rb.x_upd):
            assert isinstance(l, kind) and not l.use_conv and not list(l.parameters())
        assert m._first_norm(rb) is None, "no producer writes same-resolution planes for an up / down block"
    # against the default model: the eight resampling-convolution keys leave, 40 keys of the four blocks arrive
    base = {k: tuple(v.shape) for k, v in UNetModel(use_scale_shift_norm=film, **TINY).state_dict().items()}
    sd = _names(tag)
    gone = sorted(k for k in base if k not in sd)
    new = sorted(k for k in sd if k not in base)
    assert len(gone) == 8 and all(".op." in k or ".conv." in k for k in gone)
    assert len(new) == 40 and {k.rsplit(".", 3)[0] if k.count(".") > 3 else k for k in new} <= set(UPDOWN_BLOCKS)
    # the plain blocks are untouched; drop_site ordinals run over all ResBlocks, contiguous, in execution order
    assert [rb.drop_site for rb in m._all_resblocks()] == list(range(len(m._all_resblocks())))
    assert len(m._all_resblocks()) == len(UNetModel(**TINY)._all_resblocks()) + 4
    # every timestep block's emb_layers columns join the concatenated projection
    layout, width = m._emb_columns()
    assert {id(rb) for rb, _ in layout} >= {id(rb) for rb in found.values()}
    assert width == sum(rb.emb_layers[1].out_features for rb in m._timestep_blocks())


def test_default_model_has_no_updown_block():
    from stedm_amd.unet import ResBlock, UNetModel
    m = UNetModel(**TINY)
    assert not m.resblock_updown
    assert all(not l.updown and not hasattr(l, "h_upd") for l in m.modules() if isinstance(l, ResBlock))
    assert sum(p.numel() for p in m.parameters()) == 3922660


def test_up_wins_over_down_and_the_refusals_raise():
    from stedm_amd.unet import Downsample, ResBlock, UNetModel, Upsample
    rb = ResBlock(32, 128, 0, up=True, down=True)
    assert rb.updown and rb.up and not rb.down and isinstance(rb.h_upd, Upsample) and isinstance(rb.x_upd, Upsample)
    rb = ResBlock(32, 128, 0, down=True)
    assert rb.updown and rb.down and not rb.up and isinstance(rb.h_upd, Downsample) and isinstance(rb.x_upd, Downsample)
    assert set(rb.state_dict()) == set(ResBlock(32, 128, 0).state_dict()), "h_upd / x_upd add no state-dict key"
    for kw in (dict(up=True), dict(down=True)):
        with pytest.raises(NotImplementedError, match="out_channels"):
            ResBlock(32, 128, 0, out_channels=64, **kw)
    with pytest.raises(NotImplementedError):
        ResBlock(32, 128, 0, use_conv=True, down=True)
    with pytest.raises(NotImplementedError, match="conv_resample"):
        UNetModel(resblock_updown=True, conv_resample=False, **TINY)
    with pytest.raises(NotImplementedError, match="dropout"):
        UNetModel(resblock_updown=True, dropout=0.1, **TINY)
    for kw in (dict(num_classes=10), dict(n_embed=16), dict(dims=3)):
        with pytest.raises(NotImplementedError):
            UNetModel(resblock_updown=True, **dict(TINY, **kw))
