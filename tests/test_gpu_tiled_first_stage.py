"""GPU tier: the patch-distributed first stage on the HIP path: stedm_unfold_tiles / stedm_fold_blend (csrc/tile.hip) and
LatentDiffusion.decode_first_stage / encode_first_stage(split=...) with the real VQ stage.

unfold_tiles copies: bit for bit against torch.nn.Unfold. fold_blend against the same plan in fp64 (tiling.fold_blend_cpu) and against the
reference's own stitched outputs (tests/golden/f23_tiled_first_stage.npz). Bound, as in the CPU tier: both sides are fp32 sums of n <= 9
products followed by one division, (n + 3) roundings each: |diff| <= 16 * 2^-23 * max|o|. The uint8 output is integer work: bit for bit
against ops.image_to_uint8 of the fp32 output."""
import numpy as np
import pytest
import torch

from stedm_amd.tiling import TilePlan, fold_blend_cpu, unfold_tiles_cpu
from stedm_amd.utils import prng
from tests.golden.make_golden_tiled import CASES, SCALE_FACTOR, case_input, case_stage

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
ULP16 = 16 * 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _plan(name):
    shape, encode, _, split = CASES[name]
    return TilePlan.from_split(split, shape[2], shape[3], encode)


# (input shape, ks, stride): (a) takes the 16-byte path, (c) the scalar one, the third spans two blocks per plane
UNFOLD = {"a": ((2, 3, 12, 16), (8, 8), (4, 4)), "c": ((2, 4, 11, 13), (5, 5), (2, 2)), "two_blocks": ((1, 2, 40, 72), (36, 40), (4, 8))}


@pytest.mark.parametrize("name", sorted(UNFOLD))
def test_unfold_tiles_equals_nn_unfold_bit_for_bit(dev, name):
    from stedm_amd import ops
    shape, ks, st = UNFOLD[name]
    x = prng.normal(23, f"gpu.unfold.{name}", shape)
    u = torch.nn.Unfold(kernel_size=ks, stride=st)(x)
    L = u.shape[-1]
    want = u.view(shape[0], shape[1], ks[0], ks[1], L).permute(4, 0, 1, 2, 3).contiguous()
    xd = x.to(dev)
    got = ops.unfold_tiles(xd, ks, st)
    assert got.shape == want.shape and torch.equal(got.cpu(), want)
    assert torch.equal(ops.unfold_tiles(xd, ks, st, 2, 3).cpu(), want[2:5])          # a chunk: crops 2 .. 4
    assert torch.equal(ops.unfold_tiles(xd, ks, st, L - 1).cpu(), want[L - 1:])
    with pytest.raises(ValueError):
        ops.unfold_tiles(xd, ks, st, L - 1, 2)


def _fold(dev, stack, plan, **kw):
    from stedm_amd import ops
    w_tile, w_tie = plan.weights(dev)
    return ops.fold_blend(stack.to(dev), w_tile, w_tie, plan.out_stride, (plan.Ly, plan.Lx), **kw)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fold_blend_vs_fp64_and_the_reference(dev, golden, name):
    """the golden cases: the toy stage's outputs on the crops of the prng input (CPU), stitched by the kernel"""
    shape, encode, _, _ = CASES[name]
    plan = _plan(name)
    st = case_stage(name)
    x = case_input(name) if encode else 1. / SCALE_FACTOR * case_input(name)
    crops = unfold_tiles_cpu(x, plan)
    o = (st.encode if encode else st.decode)(crops.view((-1,) + tuple(crops.shape[2:])))
    stack = o.view((plan.L, shape[0]) + tuple(o.shape[1:])).contiguous()
    out, none = _fold(dev, stack, plan)
    assert none is None and out.shape == (shape[0], o.shape[1]) + plan.out_size
    bound = ULP16 * float(stack.abs().max())
    e64 = float((out.cpu().double() - fold_blend_cpu(stack.double(), plan)).abs().max())
    ref = torch.from_numpy(golden("f23_tiled_first_stage")[f"{name}_out"])
    eref = float((out.cpu() - ref).abs().max())
    print(f"[fold_blend {name}] max |diff| vs fp64 {e64:.3e}, vs reference {eref:.3e} (bound {bound:.3e})")
    assert e64 <= bound and eref <= bound


# (h, w, ks, stride, B, C, tie_braker): tw = 6 takes the scalar path (and C = 5 a second channel chunk), tw = 16 the 16-byte path;
# the last spans several blocks and has three covering crops per axis
EXTRA = {"scalar_b1": (8, 12, (4, 6), (2, 3), 1, 5, False), "vector_b3": (16, 40, (8, 16), (4, 8), 3, 3, True),
         "vector_c5": (16, 40, (8, 16), (4, 8), 2, 5, False), "blocks": (64, 96, (32, 48), (16, 16), 2, 3, True)}


@pytest.mark.parametrize("name", sorted(EXTRA))
def test_fold_blend_prng_stacks_vs_fp64_and_uint8(dev, name):
    """prng tile stacks scaled so that values land on both sides of +-1: the fp32 output against fp64, the uint8 output bit for bit
    against image_to_uint8 of the fp32 output, with and without the fp32 output being written"""
    from stedm_amd import ops
    h, w, ks, st, B, C, tie = EXTRA[name]
    plan = TilePlan(h, w, ks, st, tie_braker=tie)
    stack = prng.normal(23, f"gpu.fold.{name}", (plan.L, B, C) + plan.tile) * 1.5
    out, u8 = _fold(dev, stack, plan, want_u8=True)
    bound = ULP16 * float(stack.abs().max())
    e64 = float((out.cpu().double() - fold_blend_cpu(stack.double(), plan)).abs().max())
    print(f"[fold_blend {name}] max |diff| vs fp64 {e64:.3e} (bound {bound:.3e})")
    assert e64 <= bound
    assert float(out.max()) > 1 and float(out.min()) < -1 and float(out.abs().min()) < 1
    assert u8.dtype == torch.uint8 and u8.shape == (B,) + plan.out_size + (C,)
    assert torch.equal(u8, ops.image_to_uint8(out))
    none, only = _fold(dev, stack, plan, want_f32=False, want_u8=True)
    assert none is None and torch.equal(only, u8)
    assert torch.equal(_fold(dev, stack, plan)[0], out)           # deterministic


class _Net(torch.nn.Module):
    def forward_parts(self, x, xc, t, cc, out=None, uniform_t=False):
        return x


@pytest.fixture(scope="module")
def real(dev):
    """LatentDiffusion over the HIP VQ stage (DD_TINY of tests/test_gpu_vq.py, parity mode)"""
    from stedm_amd.latent_diffusion import LatentDiffusion
    from tests.test_gpu_vq import DD_TINY, build
    m = build(DD_TINY, dev)
    ld = LatentDiffusion(_Net(), linear_start=0.0015, linear_end=0.0205, image_size=8, channels=3, conditioning_key="hybrid", loss_type="l1",
                         scale_factor=SCALE_FACTOR).to(dev)
    ld.first_stage_model = m
    return ld, m


def _torch_crops(x, ks, st):
    u = torch.nn.Unfold(kernel_size=ks, stride=st)(x)
    L = u.shape[-1]
    return u.view(x.shape[0], x.shape[1], ks[0], ks[1], L).permute(4, 0, 1, 2, 3).contiguous()


def _e2e(dev, real, encode):
    ld, m = real
    B = 2
    if encode:
        x = prng.uniform(23, "gpu.e2e.x", (B, 3, 96, 128)).to(dev)
        split = dict(ks=(64, 64), stride=(32, 32), vqf=4, patch_distributed_vq=True, clip_min_weight=0.01, clip_max_weight=0.5, tie_braker=False)
        src, run, call = x, m.encode, lambda **kw: ld.encode_first_stage(x, split=split, **kw)
    else:
        z = prng.normal(23, "gpu.e2e.z", (B, 3, 24, 32)).to(dev)
        split = dict(ks=(16, 16), stride=(8, 8), vqf=4, patch_distributed_vq=True, clip_min_weight=0.01, clip_max_weight=0.5, tie_braker=True,
                     clip_min_tie_weight=0.01, clip_max_tie_weight=0.5)
        src, run, call = 1. / SCALE_FACTOR * z, m.decode, lambda **kw: ld.decode_first_stage(z, split=split, **kw)
    plan = TilePlan.from_split(split, src.shape[2], src.shape[3], encode)
    assert plan.L == 6 and plan.default_tile_batch(B) == 6
    return B, src, run, call, plan


@pytest.mark.parametrize("encode", [False, True])
def test_end_to_end_with_the_real_stage(dev, real, encode):
    """the HIP tiled path against fold_blend_cpu over the existing m.decode / m.encode on torch-unfolded crops: the new code alone, not the
    first stage's own tolerance"""
    B, src, run, call, plan = _e2e(dev, real, encode)
    crops = _torch_crops(src.cpu(), plan.ks, plan.stride).to(dev)
    o = run(crops.view((-1,) + tuple(crops.shape[2:])))
    stack = o.view((plan.L, B) + tuple(o.shape[1:])).cpu()
    want = fold_blend_cpu(stack, plan)
    got = call()
    assert got.shape == want.shape == (B, 3) + plan.out_size
    bound = ULP16 * float(stack.abs().max())
    err = float((got.cpu() - want).abs().max())
    print(f"[tiled {'encode' if encode else 'decode'}, real stage] max |diff| vs fold_blend_cpu of the stage's crops {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    if not encode:
        from stedm_amd import ops
        assert torch.equal(call(out_u8=True), ops.image_to_uint8(got))


@pytest.mark.parametrize("encode", [False, True])
def test_tile_batch_4_and_default_agree_bit_for_bit(dev, real, encode):
    """tile_batch 4 (calls of 4 + 2 crops, 8 + 4 samples) and the default (one call of 12 samples) must give the same bits. The VQ stage's
    convolutions choose their K split from the number of tiles in a launch, i.e. from the call's batch (csrc/conv_rs.inc, pick_split); the
    tiled path therefore runs the stage in its batch_invariant mode (no split-K workspace). Without that mode the encode differed by
    2.1e-06 at max |out| 3.2 (4285 of 4608 elements) between the two settings."""
    B, src, run, call, plan = _e2e(dev, real, encode)
    one, chunked = call(), call(tile_batch=4)
    diff = float((one - chunked).abs().max())
    print(f"[tiled {'encode' if encode else 'decode'}, real stage] tile_batch 4 vs default: max |diff| {diff:.3e}, "
          f"{int((one != chunked).sum())} of {one.numel()} elements differ (max |out| {float(one.abs().max()):.3f})")
    assert torch.equal(chunked, one)
