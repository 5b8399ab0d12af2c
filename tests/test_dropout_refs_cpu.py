"""CPU tier: the mask stream of the U-Net's ResBlock dropout sites (tests/refs_dropout.py) against the oracle's elementwise stream, its
statistics, the numpy drop pass and its backward against torch autograd in fp64, and the host logic of UNetModel(dropout=...)."""
import numpy as np
import pytest
import torch

from oracle import dropmask as OD
from tests import refs_dropout as RD

SEED = 0x1234ABCD5678
TINY = dict(image_size=16, in_channels=7, model_channels=32, out_channels=4, num_res_blocks=2,
            attention_resolutions=[32, 16, 8], channel_mult=[1, 2, 4], num_heads=4)


@pytest.mark.parametrize("n", [16384, 7200, 13])
@pytest.mark.parametrize("site", [RD.SITE0, RD.SITE0 + 3, 17])
def test_step0_is_the_oracles_elementwise_stream(n, site):
    for p in (0.1, 0.5):
        assert np.array_equal(RD.keep_mask(n, p, SEED, site, 0), OD.keep_elementwise(n, p, SEED, site))


def test_step_and_site_change_the_mask():
    n, p = 16384, 0.1
    base = RD.keep_mask(n, p, SEED, RD.SITE0, 0)
    d_step = float((base != RD.keep_mask(n, p, SEED, RD.SITE0, 1)).mean())
    d_site = float((base != RD.keep_mask(n, p, SEED, RD.SITE0 + 1, 0)).mean())
    print(f"masks differ in {100 * d_step:.1f} % (step) and {100 * d_site:.1f} % (site) of the positions")
    # two independent masks of keep probability 0.9 differ in 2 * 0.9 * 0.1 = 18 % of the positions
    assert 0.17 <= d_step <= 0.19 and 0.17 <= d_site <= 0.19


def test_kept_fraction():
    worst = 0.0
    for p in (0.1, 0.5):
        for site in (RD.SITE0, RD.SITE0 + 3):
            for step in (0, 1, 7):
                for n in (16384, 7200, 131072):
                    dev = abs(float(RD.keep_mask(n, p, SEED, site, step).mean()) - (1.0 - p))
                    worst = max(worst, dev)
                    assert dev <= 0.01, (p, site, step, n, dev)
    print(f"largest deviation of the kept fraction from 1 - p: {worst:.4f}")


def test_inv_keep_and_threshold():
    assert float(RD.inv_keep(0.5)) == 2.0
    assert RD.inv_keep(0.1) == np.float32(1.0 / (1.0 - float(np.float32(0.1))))
    assert OD.thr16(0.5) == 32768 and OD.thr16(0.1) == 6554


@pytest.mark.parametrize("film", [False, True], ids=["plain", "film"])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_numpy_drop_pass_and_backward_equal_torch_autograd(film, p):
    B, HW, C, groups, eps = 3, 25, 48, 6, 1e-5
    rng = np.random.default_rng(5)
    x = rng.normal(0.3, 1.5, (B, HW, C))
    gamma, beta = rng.normal(1.0, 0.5, C), rng.normal(0.0, 0.5, C)
    scale = rng.normal(0.0, 0.5, (B, C)) if film else None
    shift = rng.normal(0.0, 0.5, (B, C)) if film else None
    dA = rng.normal(0.0, 1.0, (B, HW, C))
    mask = RD.resblock_mask(B, HW, C, p, SEED, 4, 9).numpy()
    assert 0 < mask.sum() < mask.size
    y = RD.drop_pass_np(x, gamma, beta, groups, eps, mask, p, scale, shift)
    dx, dg, db, dsc, dsh = RD.drop_pass_bwd_np(x, gamma, beta, groups, eps, mask, p, dA, scale, shift)

    T = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    with torch.enable_grad():       # (other test modules switch autograd off process-wide when they are collected)
        xt, gt, bt = T(x), T(gamma), T(beta)
        # F.group_norm wants [B, C, *]
        v = torch.nn.functional.group_norm(xt.permute(0, 2, 1), groups, gt, bt, eps).permute(0, 2, 1)
        leaves = [xt, gt, bt]
        if film:
            st, ht = T(scale), T(shift)
            v = v * (1.0 + st[:, None, :]) + ht[:, None, :]
            leaves += [st, ht]
        # mask / (1 - p) with the stream's own scale: (float)(1 / (1 - p)), 6e-8 from the double quotient
        yt = torch.nn.functional.silu(v) * torch.from_numpy(mask) * float(RD.inv_keep(p))
        grads = torch.autograd.grad(yt, leaves, torch.from_numpy(dA))
    assert float(np.abs(yt.detach().numpy() - y).max()) < 1e-12
    assert np.array_equal(y == 0.0, ~mask | (yt.detach().numpy() == 0.0))
    for got, ref, name in zip((dx, dg, db, dsc, dsh), grads, ("dx", "dgamma", "dbeta", "dscale", "dshift")):
        err = float(np.abs(got - ref.numpy()).max()) / float(ref.abs().max())
        assert err < 1e-11, (name, err)


# ------------------------------------------------------------------------------------------------ host logic
def test_unet_with_dropout_constructs_with_the_same_state_dict():
    from stedm_amd.unet import UNetModel
    m0 = UNetModel(dropout=0, **TINY)
    m1 = UNetModel(dropout=0.1, **TINY)
    assert list(m0.state_dict().keys()) == list(m1.state_dict().keys())
    rbs = m1._all_resblocks()
    assert all(isinstance(rb.out_layers[2], torch.nn.Dropout) and rb.out_layers[2].p == 0.1 and rb.dropout == 0.1 for rb in rbs)
    assert m1.dropout_seed is None and m1.last_dropout is None
    assert m1.dropout_live() and not m0.dropout_live()
    m1.eval()
    assert not m1.dropout_live()
    with pytest.raises(ValueError):
        UNetModel(dropout=1.0, **TINY)


def test_site_ordinals_follow_the_execution_order():
    from stedm_amd.unet import ResBlock, ResBlockStyle, UNetModel
    m = UNetModel(dropout=0.1, **TINY)
    order = []
    for blk in list(m.input_blocks) + [m.middle_block] + list(m.output_blocks):
        for layer in blk:
            if isinstance(layer, ResBlock):
                order.append(layer)
            elif isinstance(layer, ResBlockStyle):
                order.append(layer.block)
    # 3 levels x 2 input blocks, 3 in the middle (the style block's inner block is the second of them), 3 x 3 output blocks
    assert len(order) == 6 + 3 + 9
    assert [rb.drop_site for rb in order] == list(range(len(order)))
    assert m.middle_block[1].block.drop_site == 7
    assert [rb.drop_site for rb in m._all_resblocks()] == list(range(18))


def test_other_unimplemented_options_still_raise():
    from stedm_amd.unet import UNetModel
    with pytest.raises(NotImplementedError):
        UNetModel(dropout=0.1, resblock_updown=True, **TINY)
    with pytest.raises(NotImplementedError):
        UNetModel(dropout=0.1, num_classes=10, **TINY)


def test_per_rank_seed_rule():
    from stedm_amd.unet import UNetModel
    s = 0x0123456789ABCDEF
    assert UNetModel.rank_dropout_seed(s, 0) == s
    assert UNetModel.rank_dropout_seed(s, 1) == s ^ 0x9E3779B97F4A7C15
    assert UNetModel.rank_dropout_seed(s, 3) == s ^ ((3 * 0x9E3779B97F4A7C15) % (1 << 64))
    assert len({UNetModel.rank_dropout_seed(s, r) for r in range(64)}) == 64
    for r in (0, 1, 3, 7):
        assert UNetModel.rank_dropout_seed(s, r) == RD.rank_seed(s, r)


def test_live_model_refuses_the_inference_entry_points_before_any_device_work():
    from stedm_amd.unet import UNetModel
    m = UNetModel(dropout=0.1, **TINY).train()
    x = torch.zeros((2, 7, 16, 16))
    t = torch.tensor([1, 2])
    ctx = torch.zeros((2, 128))
    with pytest.raises(RuntimeError, match=r"\.eval\(\)"):
        m(x, t, context=ctx)
    with pytest.raises(RuntimeError, match=r"\.eval\(\)"):
        m.forward_cfg(x[:, :4], x[:, 4:], t, ctx, ctx)
