"""CPU tier: the restatements of tests/refs_resample.py against torch's own operators, and UNetModel(conv_resample=False) against what the
reference's constructor gave (tests/golden/make_golden_noresample.py: parameter count, state-dict names and shapes)."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from tests import refs_resample as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(image_size=16, in_channels=7, model_channels=32, out_channels=4, num_res_blocks=2,
            attention_resolutions=[32, 16, 8], channel_mult=[1, 2, 4], num_heads=4)
SHAPES = [(2, 4, 4, 32), (3, 6, 10, 96), (1, 40, 32, 8), (2, 10, 16, 4)]


def _nchw(x):
    return x.permute(0, 3, 1, 2)


@pytest.mark.parametrize("shape", SHAPES)
def test_avgpool2x2_is_avg_pool2d(shape):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    ref = F.avg_pool2d(_nchw(x), 2, 2)
    assert torch.allclose(_nchw(R.avgpool2x2(x)), ref, rtol=0, atol=1e-15)
    d = R.dyadic(g, shape)          # dyadic values: exact in fp32, so equal to torch's fp32 operator whatever its order
    assert torch.equal(_nchw(R.avgpool2x2(d)), F.avg_pool2d(_nchw(d), 2, 2))
    with pytest.raises(AssertionError):
        R.avgpool2x2(torch.zeros(1, 3, 4, 4))


@pytest.mark.parametrize("shape", SHAPES)
def test_replicate2x2_is_nearest_interpolate_and_the_pools_gradient(shape):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    assert torch.equal(_nchw(R.replicate2x2(x)), F.interpolate(_nchw(x), scale_factor=2, mode="nearest"))
    # scale 0.25: the gradient of the average pool, by autograd; with a prior: added onto it
    B, H, W, C = shape
    xin = torch.randn((B, 2 * H, 2 * W, C), generator=g, dtype=torch.float64, requires_grad=True)
    with torch.enable_grad():        # (the GPU test modules switch autograd off process-wide when they are collected)
        (F.avg_pool2d(_nchw(xin), 2, 2) * _nchw(x)).sum().backward()
    assert torch.allclose(R.replicate2x2(x, 0.25), xin.grad, rtol=0, atol=1e-15)
    prior = torch.randn((B, 2 * H, 2 * W, C), generator=g, dtype=torch.float64)
    assert torch.equal(R.replicate2x2(x, 0.25, prior), prior + R.replicate2x2(x, 0.25))
    # the nearest x2's own gradient is the 2 x 2 block sum, i.e. four times the pool
    xl = x.clone().requires_grad_(True)
    with torch.enable_grad():
        (F.interpolate(_nchw(xl), scale_factor=2, mode="nearest") * _nchw(prior)).sum().backward()
    assert torch.allclose(xl.grad, 4 * R.avgpool2x2(prior), rtol=0, atol=1e-14)


@pytest.mark.parametrize("shape", SHAPES)
def test_chan_stats_fold_to_the_tensors_sums_for_any_partition(shape):
    g = torch.Generator().manual_seed(3)
    B, H, W, C = shape
    out = R.dyadic(g, shape)
    want = torch.stack([out.double().sum(dim=(1, 2)), (out.double() ** 2).sum(dim=(1, 2))], dim=-1)
    parts = [R.pool_slots(H, W), torch.randint(0, 5, (H, W), generator=g), torch.zeros((H, W), dtype=torch.long)]
    if H % 2 == 0 and W % 2 == 0:
        parts.append(R.replicate_slots(H // 2, W // 2))
    for slots in parts:
        cs = R.chan_stats(out, slots)
        assert cs.shape[0] == B and tuple(cs.shape[2:]) == (C, 2)
        assert torch.equal(R.fold(cs), want)
    # both kernels' partitions have stedm_gn_chan_nslab(Ho * Wo) slots
    assert int(R.pool_slots(H, W).max()) + 1 == R.nslab(H, W)
    assert int(R.replicate_slots(H, W).max()) + 1 == R.nslab(2 * H, 2 * W)
    # the replicate's statistics are four times those of the scaled input over the run of 64 input pixels
    x = R.dyadic(g, shape)
    cs_hi = R.chan_stats(R.replicate2x2(x, 0.25), R.replicate_slots(H, W))
    cs_lo = R.chan_stats(0.25 * x, (torch.arange(H * W) // 64).view(H, W))
    assert torch.equal(cs_hi, 4 * cs_lo)


def _names(tag):
    with open(os.path.join(ROOT, "tests", "golden", f"f31_unet_{tag}_names.json")) as f:
        return {k: tuple(v) for k, v in json.load(f).items()}


@pytest.mark.parametrize("tag,film", [("noconv", False), ("noconv_film", True)])
def test_conv_resample_false_constructs_with_the_references_state_dict(golden, tag, film):
    from stedm_amd.unet import Downsample, UNetModel, Upsample
    fx = golden(f"f31_unet_{tag}_tiny")
    m = UNetModel(conv_resample=False, use_scale_shift_norm=film, **TINY)
    assert sum(p.numel() for p in m.parameters()) == int(fx["n_params"])
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == _names(tag)
    assert list(m.state_dict()) == list(_names(tag)), "the reference's order too"
    res = [l for l in m.modules() if isinstance(l, (Downsample, Upsample))]
    assert len(res) == 4 and all(not l.use_conv and not list(l.parameters()) for l in res)
    if not film:
        assert int(fx["n_params"]) == 3691972


def test_conv_resample_true_is_unchanged():
    """the default model keeps its names: those of the conv-less model plus the four resampling convolutions; 3 922 660 parameters, as the
    reference's (checked when the fixtures were made)"""
    from stedm_amd.unet import UNetModel
    m = UNetModel(**TINY)
    sd = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    base = _names("noconv")
    extra = {k: v for k, v in sd.items() if k not in base}
    assert all(sd[k] == v for k, v in base.items())
    assert extra == {"input_blocks.3.0.op.weight": (32, 32, 3, 3), "input_blocks.3.0.op.bias": (32,),
                     "input_blocks.6.0.op.weight": (64, 64, 3, 3), "input_blocks.6.0.op.bias": (64,),
                     "output_blocks.2.1.conv.weight": (128, 128, 3, 3), "output_blocks.2.1.conv.bias": (128,),
                     "output_blocks.5.1.conv.weight": (64, 64, 3, 3), "output_blocks.5.1.conv.bias": (64,)}
    assert sum(p.numel() for p in m.parameters()) == 3922660


def test_downsample_without_conv_asserts_equal_channels_and_other_options_keep_raising():
    from stedm_amd.unet import Downsample, UNetModel
    with pytest.raises(AssertionError):
        Downsample(32, False, out_channels=64)
    for kw in (dict(resblock_updown=True), dict(num_classes=10), dict(n_embed=16), dict(dims=3)):
        with pytest.raises(NotImplementedError):
            UNetModel(conv_resample=False, **dict(TINY, **kw))
