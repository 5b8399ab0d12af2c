"""CPU tier: the patch-distributed first stage (stedm_amd/tiling.py, LatentDiffusion.decode_first_stage / encode_first_stage with
`split_input_params`) against the reference's own get_weighting / get_fold_unfold / decode_first_stage / encode_first_stage
(tests/golden/f23_tiled_first_stage.npz, written by tests/golden/make_golden_tiled.py from the toy stage defined there).

Bound: this path and the reference are both fp32 sums of n <= 9 products followed by one division, so (n + 3) roundings on each side:
|diff| <= 16 * 2^-23 * max|o| per case."""
import numpy as np
import pytest
import torch

from stedm_amd.tiling import TilePlan, fold_blend_cpu, unfold_tiles_cpu
from tests.golden.make_golden_tiled import CASES, SCALE_FACTOR, case_input, case_split, case_stage

torch.set_grad_enabled(False)
ULP16 = 16 * 2.0 ** -23


class _Net(torch.nn.Module):
    """a denoiser stand-in with the one entry point DiffusionWrapper calls"""

    def forward_parts(self, x, xc, t, cc, out=None, uniform_t=False):
        return x + 0.0


def _ld(stage, scale_factor=SCALE_FACTOR):
    from stedm_amd.latent_diffusion import LatentDiffusion
    ld = LatentDiffusion(_Net(), linear_start=0.0015, linear_end=0.0205, image_size=8, channels=3, conditioning_key="hybrid", loss_type="l1",
                         scale_factor=scale_factor)
    ld.first_stage_model = stage
    return ld


def _plan(name):
    shape, encode, _, split = CASES[name]
    return TilePlan.from_split(split, shape[2], shape[3], encode)


@pytest.mark.parametrize("name", sorted(CASES))
def test_weight_tables_equal_the_reference_bit_for_bit(golden, name):
    fx = golden("f23_tiled_first_stage")
    plan = _plan(name)
    assert [plan.Ly, plan.Lx] == fx[f"{name}_grid"].tolist() and plan.L == plan.Ly * plan.Lx
    assert plan.w_tile.dtype == torch.float32 and plan.w_tie.dtype == torch.float32
    assert np.array_equal(plan.w_tile.numpy(), fx[f"{name}_w_tile"])
    assert np.array_equal(plan.w_tie.numpy(), fx[f"{name}_w_tie"])
    th, tw = plan.tile
    prod = plan.w_tile.reshape(th * tw, 1) * plan.w_tie.reshape(1, plan.L)
    assert np.array_equal(prod.numpy(), fx[f"{name}_weighting"])
    assert (plan.w_tie == 1).all() or CASES[name][3]["tie_braker"]


def test_plan_geometry():
    p = _plan("a")
    assert (p.tile, p.out_stride, p.out_size, p.L) == ((16, 16), (8, 8), (24, 32), 6)
    p = _plan("d")
    assert (p.tile, p.out_stride, p.out_size, p.L) == ((4, 4), (2, 2), (6, 8), 6)
    p = _plan("c")
    assert (p.tile, p.out_stride, p.out_size, (p.Ly, p.Lx)) == ((5, 5), (2, 2), (11, 13), (4, 5))
    p = _plan("e")                                      # ks and stride larger than the input are reduced to the input: one crop
    assert (p.ks, p.stride, p.L, p.out_size) == ((10, 10), (10, 10), 1, (20, 20))
    assert TilePlan(16, 16, 8, 4).ks == (8, 8)          # an int stands for a square


def test_unfold_is_nn_unfold_and_fold_of_constant_tiles_is_constant():
    x = case_input("c")
    plan = _plan("c")
    t = unfold_tiles_cpu(x, plan)
    u = torch.nn.Unfold(kernel_size=plan.ks, stride=plan.stride)(x)                     # [B, C*kh*kw, L]
    want = u.view(x.shape[0], x.shape[1], plan.ks[0], plan.ks[1], plan.L).permute(4, 0, 1, 2, 3)
    assert torch.equal(t, want)
    assert torch.equal(unfold_tiles_cpu(x, plan, 2, 3), want[2:5])
    ones = torch.full((plan.L, 1, 1) + plan.tile, 3.0)
    out = fold_blend_cpu(ones, plan)
    assert out.shape == (1, 1) + plan.out_size and float((out - 3.0).abs().max()) <= 3.0 * 4 * 2.0 ** -23
    with pytest.raises(ValueError):
        unfold_tiles_cpu(x, plan, 18, 3)


def _run(ld, name, **kw):
    x = case_input(name)
    return ld.encode_first_stage(x, **kw) if CASES[name][1] else ld.decode_first_stage(x, **kw)


@pytest.mark.parametrize("name", sorted(CASES))
def test_attribute_route_matches_the_reference(golden, name):
    ref = torch.from_numpy(golden("f23_tiled_first_stage")[f"{name}_out"])
    ld = _ld(case_stage(name))
    ld.split_input_params = case_split(name)
    out = _run(ld, name)
    assert out.shape == ref.shape and out.dtype == torch.float32
    bound = ULP16 * float(ref.abs().max())
    err = float((out - ref).abs().max())
    print(f"[tiled {name}] max |diff| vs reference {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    if CASES[name][1]:
        assert tuple(ld.split_input_params["original_image_size"]) == CASES[name][0][2:]          # ddpm.py:835
    # crops run in batches: every tile_batch gives the same crops, the same stage outputs and the same blend
    for tb in (1, 4, 100):
        assert torch.equal(_run(ld, name, tile_batch=tb), out)


def test_split_keyword_route_and_int_ks(golden):
    ref = torch.from_numpy(golden("f23_tiled_first_stage")["b_out"])
    ld = _ld(case_stage("b"))
    split = dict(case_split("b"), ks=8, stride=4)
    out = ld.decode_first_stage(case_input("b"), split=split)
    assert float((out - ref).abs().max()) <= ULP16 * float(ref.abs().max())
    assert not hasattr(ld, "split_input_params")
    u8 = ld.decode_first_stage(case_input("b"), split=split, out_u8=True)
    assert u8.dtype == torch.uint8 and u8.shape == (2, 24, 32, 3)
    assert torch.equal(u8, ((out.clamp(-1, 1).permute(0, 2, 3, 1) + 1) * 127.5).to(torch.uint8))
    # patch_distributed_vq false: the one-call path, whichever route carries it
    off = dict(split, patch_distributed_vq=False)
    whole = ld.first_stage_model.decode(case_input("b") / SCALE_FACTOR)
    assert torch.equal(ld.decode_first_stage(case_input("b"), split=off), whole)
    ld.split_input_params = off
    assert torch.equal(ld.decode_first_stage(case_input("b")), whole)


def test_without_split_the_path_is_todays(golden):
    """neither keyword nor attribute: one first-stage call on z / scale_factor (decode) or x (encode), other keywords ignored"""
    st = case_stage("a")
    ld = _ld(st)
    z = case_input("a")
    want = st.decode(z / SCALE_FACTOR)
    assert want.shape == (2, 3, 24, 32)
    assert torch.equal(ld.decode_first_stage(z), want)
    assert torch.equal(ld.decode_first_stage(z, predict_cids=False, force_not_quantize=True), want)
    std = case_stage("d")
    x = case_input("d")
    assert torch.equal(_ld(std).encode_first_stage(x), std.encode(x))
    # and the tiled result differs from it: the toy stage's ramp restarts in every crop
    assert not torch.allclose(ld.decode_first_stage(z.new_zeros(2, 3, 12, 16), split=case_split("a")), st.decode(z.new_zeros(2, 3, 12, 16)))


def test_apply_model_refuses_the_attribute_route_only():
    ld = _ld(case_stage("a"))
    x = torch.zeros(2, 3, 8, 8)
    t = torch.zeros(2, dtype=torch.long)
    cond = {"c_concat": [torch.zeros(2, 1, 8, 8)], "c_crossattn": [torch.zeros(2, 4)]}
    assert torch.equal(ld.apply_model(x, t, cond), x)
    ld.decode_first_stage(case_input("a"), split=case_split("a"))          # the keyword route leaves sampling alone
    assert torch.equal(ld.apply_model(x, t, cond), x)
    ld.split_input_params = case_split("a")
    with pytest.raises(NotImplementedError, match="len\\(cond\\) == 1"):
        ld.apply_model(x, t, cond)
    with pytest.raises(NotImplementedError):
        ld.apply_model_cfg(x, t, cond, cond)


@pytest.mark.parametrize("kw,exc,msg", [
    (dict(h=13, w=16, ks=8, stride=4), ValueError, "covered by no crop"),
    (dict(h=12, w=17, ks=8, stride=4), ValueError, "covered by no crop"),
    (dict(h=8, w=16, ks=8, stride=4, tie_braker=True), ValueError, "h - 1 = 0"),                 # Ly == 1
    (dict(h=12, w=8, ks=8, stride=4, tie_braker=True), ValueError, "h - 1 = 0"),                 # Lx == 1
    (dict(h=8, w=8, ks=4, stride=4, df=4), ValueError, "h - 1 = 0"),                             # output tile side of 1
    (dict(h=12, w=16, ks=(8, 4), stride=4, uf=2), ValueError, "kernel_size\\[0\\]"),
    (dict(h=24, w=32, ks=(16, 8), stride=8, df=4), ValueError, "kernel_size\\[0\\]"),
    (dict(h=24, w=24, ks=18, stride=6, df=4), ValueError, "divisible by df"),
    (dict(h=28, w=28, ks=16, stride=6, df=4), ValueError, "divisible by df"),
    (dict(h=12, w=20, ks=4, stride=8), ValueError, "lie under no crop"),                        # stride > ks: gaps between the crops
    (dict(h=12, w=16, ks=8, stride=4, uf=2, df=2), NotImplementedError, "uf > 1 together with df > 1"),
])
def test_refusals(kw, exc, msg):
    with pytest.raises(exc, match=msg):
        TilePlan(**kw)


def test_refusals_reach_the_public_interface_before_the_first_stage():
    class Boom:
        def decode(self, z):
            raise AssertionError("the first stage must not run")
        encode = decode
    ld = _ld(Boom())
    with pytest.raises(ValueError, match="covered by no crop"):
        ld.decode_first_stage(torch.zeros(1, 3, 13, 16), split=case_split("a"))
    with pytest.raises(ValueError, match="divisible by df"):
        ld.encode_first_stage(torch.zeros(1, 3, 24, 24), split=dict(case_split("d"), ks=(18, 18), stride=(6, 6)))
    with pytest.raises(NotImplementedError):
        TilePlan(12, 16, 8, 4, uf=2, df=2)


def test_default_tile_batch_bounds_a_call():
    """CALL_LATENT_PIXELS: 16 latents of 128^2 per call, half of what the VQ-f4 decoder's 32-bit plane offsets admit (its widest plane has
    16 * 256 elements per latent pixel: 2^31 at 32 latents of 128^2)"""
    from stedm_amd.tiling import CALL_LATENT_PIXELS
    assert CALL_LATENT_PIXELS == 16 * 128 * 128 and CALL_LATENT_PIXELS * 16 * 256 == 2 ** 30
    assert TilePlan(256, 256, 128, 64, uf=4).default_tile_batch(4) == 4          # 9 crops of 128^2 at B = 4: four crops per call
    assert TilePlan(128, 128, 64, 32, uf=4).default_tile_batch(64) == 1          # 64^2 crops at B = 64: one crop per call
    assert TilePlan(512, 512, 256, 128, uf=4).default_tile_batch(64) == 1        # never below one crop
    assert TilePlan(512, 512, 256, 128, df=4).default_tile_batch(8) == 8         # encode: ks in image pixels, 64^2 latent pixels per crop
    assert TilePlan(24, 32, 16, 8, uf=4).default_tile_batch(2) == 6              # small inputs: every crop in one call
