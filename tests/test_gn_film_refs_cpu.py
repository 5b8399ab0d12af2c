"""CPU tier for the FiLM (use_scale_shift_norm) GroupNorm kernels: the fp32 emulations of tests/refs_gn_film.py against the fp64 statement
of the reference's formula inside the derived bounds, the closed-form backward against torch.autograd, the kernel form every GPU case
reaches, the seeded defects outside a tier, and the host logic of the model (state dict, embedding layout). No GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import refs_gn as RG
from tests import refs_gn_film as RF

TINY = dict(image_size=16, in_channels=7, model_channels=32, out_channels=4, num_res_blocks=2,
            attention_resolutions=[32, 16, 8], channel_mult=[1, 2, 4], num_heads=4)
SMALL_FWD = [c for c in RF.FWD if c[1] * c[2] * c[3] * c[4] <= 1 << 20]      # the emulation of the large cases adds nothing on the CPU


def _emu_fwd(case, prob, dtype, defects=()):
    name, B, H, W, C, groups, hilo, chan, lay = case
    mr32 = RG.emu_fold(prob["cs"], None, 0, groups, H * W, prob["eps"])
    return RF.emu_apply16c_film(prob["x"], mr32, groups, prob["gamma"], prob["beta"], prob["film"], prob["bstride"], prob["off"], prob["act"],
                                dtype, hilo, defects), mr32


# ------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("case", RF.FWD, ids=RF.FWD_IDS)
def test_forward_cases_reach_the_8_wide_kernel_form_they_name(case):
    name, B, H, W, C, groups, hilo, chan, lay = case
    kernel, slab, cb, pair = RG.apply16c_geometry(B, H * W, C, 0, groups, hilo, False)
    assert kernel == "v8" and C % 8 == 0 and 5 * C * 4 <= 48 * 1024
    assert (cb > 0) == chan
    total = (C // 4) * (H * W if cb else min(slab, H * W))          # quads of a (first) block run; a block iteration takes 512
    per = (cb // 4) * H * W if cb else total
    if name == "px_tail":
        assert per < 512                                             # tail body only
    if name == "px_full":
        assert per % 512 == 0 and per >= 512                         # full iterations, no tail
    if name == "px_full_tail":
        assert per > 512 and per % 512 != 0
    if name == "chan_runs":
        assert cb == 128
    if name == "cpg1_tiny":
        assert C // groups == 1


@pytest.mark.parametrize("case", RF.BWD, ids=RF.BWD_IDS)
def test_backward_cases_reach_the_form_they_name(case):
    name, B, H, W, C, groups, form = case[:7]
    cb, ppt = RG.gn_bwd_fused_cb(C, 0, groups, H * W)
    assert (cb > 0) == form[0]
    assert ((2 if ppt <= 2 else 4 if ppt <= 4 else 8) if cb else 0) == form[1]         # the PPT instantiation, 0: the three-kernel chain
    if name == "ragged":
        assert (H * W) % (512 // (cb // 4)) != 0                     # the last pixel step of a lane is partly dead


def test_backward_cases_cover_every_instantiation():
    seen = set()
    for c in RF.BWD:
        cb, ppt = RG.gn_bwd_fused_cb(c[4], 0, c[5], c[2] * c[3])
        seen.add((2 if ppt <= 2 else 4 if ppt <= 4 else 8) if cb else 0)
    assert seen == {0, 2, 4, 8}


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("case", SMALL_FWD, ids=[c[0] for c in SMALL_FWD])
def test_forward_emulation_is_exact_on_the_exact_pattern(case, dtype):
    prob = RF.fwd_problem(case, True, dtype, 0, 0.0)
    (hi, lo), mr32 = _emu_fwd(case, prob, dtype)
    assert torch.equal(mr32, prob["mr"])
    assert torch.equal(hi, prob["hi"])
    if case[6]:
        assert torch.equal(lo, torch.zeros_like(lo))
    # scale and shift differ between samples and between channels (else a row or channel mix-up would go unseen)
    s, sh = RF.film_rows(prob["film"], case[1], case[4], prob["bstride"], prob["off"])
    assert s.unique().numel() == 4 and sh.unique().numel() == 9
    if prob["bstride"]:
        assert not torch.equal(s[0], s[1])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("act,eps", [(0, 1e-5), (1, 1e-6)])
@pytest.mark.parametrize("case", SMALL_FWD, ids=[c[0] for c in SMALL_FWD])
def test_forward_emulation_within_the_bound(case, act, eps, dtype):
    prob = RF.fwd_problem(case, False, dtype, act, eps)
    (hi, lo), _ = _emu_fwd(case, prob, dtype)
    r = RF.ratio(RG.planes_value(hi, lo, dtype) - prob["ref"], prob["bound"])
    print(f"[{case[0]} act={act} eps={eps} {dtype}] worst err / bound {r:.3f}")
    assert r < 1.0


def test_forward_reference_is_the_reference_formula():
    """film_group_norm against F.group_norm(x) * (1 + scale) + shift -> SiLU in fp64 (openaimodel.py:280-284)"""
    B, HW, C, groups = 3, 20, 24, 4
    x = RG.normal((B, HW, C), 1, "ff.x").double()
    g, b = RG.normal((C,), 1, "ff.g").double(), RG.normal((C,), 1, "ff.b").double()
    film = RG.normal((B, 2 * C), 1, "ff.film", std=0.5).double()
    s, sh = RF.film_rows(film, B, C, 2 * C, 0)
    ref = F.silu(F.group_norm(x.permute(0, 2, 1), groups, g, b, 1e-5) * (1 + film[:, :C, None]) + film[:, C:, None]).permute(0, 2, 1)
    out = RF.film_group_norm(x, groups, g, b, 1e-5, 1, s, sh)
    assert float((out - ref).abs().max()) < 1e-12


@pytest.mark.parametrize("defect", ["row0", "swap", "no_one", "no_off"])
def test_forward_seeded_defects_are_caught(defect):
    case = RF.FWD[1]                     # px_tail: per-sample rows at an offset inside a wider row
    for dtype in (torch.float16, torch.bfloat16):
        prob = RF.fwd_problem(case, False, dtype, 1, 1e-5)
        (hi, lo), _ = _emu_fwd(case, prob, dtype, (defect,))
        assert RF.ratio(RG.planes_value(hi, lo, dtype) - prob["ref"], prob["bound"]) >= 1.0, (defect, "bound tier")
        prob = RF.fwd_problem(case, True, dtype, 0, 0.0)
        (hi, lo), _ = _emu_fwd(case, prob, dtype, (defect,))
        assert not torch.equal(hi, prob["hi"]), (defect, "exact tier")


# ------------------------------------------------------------------------------------------------ backward
def _emu_bwd(case, prob, dtype, defects=()):
    name, B, H, W, C, groups, form, act, use_add, acc, acc_param, planes = case
    return RF.emu_gn_bwd_film(prob["x"], prob["mr32"], groups, prob["gamma"], prob["beta"], prob["film"], prob["bstride"], prob["off"], act,
                              prob["dA"], prob["add"], prob["old"], acc, dtype, planes, prob["dg0"], prob["db0"], acc_param, prob["dE0"],
                              prob["d_off"], defects)


@pytest.mark.parametrize("case", RF.BWD, ids=RF.BWD_IDS)
def test_backward_emulation_within_the_bounds(case):
    dtype = torch.bfloat16
    prob = RF.bwd_problem(case, dtype)
    r = RF.bwd_ratios(case, prob, _emu_bwd(case, prob, dtype), dtype)
    print(f"[{case[0]}] worst err / bound", {k: round(v, 3) for k, v in r.items()})
    assert max(r.values()) < 1.0, r


def test_backward_closed_form_is_the_autograd_gradient():
    """film_group_norm_bwd with exact statistics against autograd through F.group_norm(x) * (1 + s) + sh -> SiLU, fp64"""
    B, HW, C, groups, eps = 3, 12, 16, 4, 1e-5
    x = RG.normal((B, HW, C), 2, "fa.x").double().requires_grad_(True)
    g = RG.normal((C,), 2, "fa.g", mean=1.0).double().requires_grad_(True)
    b = RG.normal((C,), 2, "fa.b").double().requires_grad_(True)
    s = RG.normal((B, 1, C), 2, "fa.s", std=0.5).double().requires_grad_(True)
    sh = RG.normal((B, 1, C), 2, "fa.sh", std=0.5).double().requires_grad_(True)
    dA = RG.normal((B, HW, C), 2, "fa.dA").double()
    with torch.enable_grad():
        out = F.silu(F.group_norm(x.permute(0, 2, 1), groups, g, b, eps).permute(0, 2, 1) * (1 + s) + sh)
        (out * dA).sum().backward()
    mr = RG.stats_of(x.detach(), groups, eps)[0]
    dx, dg, db, dsc, dsh = RF.film_group_norm_bwd(x.detach(), mr, groups, g.detach(), b.detach(), 1, s.detach(), sh.detach(), dA)
    for got, ref in ((dx, x.grad), (dg, g.grad), (db, b.grad), (dsc, s.grad[:, 0]), (dsh, sh.grad[:, 0])):
        assert float((got - ref).abs().max()) < 1e-10 * (1.0 + float(ref.abs().max()))


@pytest.mark.parametrize("defect,outputs", [("row0", ("dx",)), ("swap", ("dx",)), ("no_one", ("dx", "dgamma")), ("no_off", ("dx",)),
                                            ("dscale_no_beta", ("dscale",)), ("dgamma_unweighted", ("dgamma",))])
def test_backward_seeded_defects_are_caught(defect, outputs):
    case, dtype = RF.BWD[0], torch.bfloat16
    prob = RF.bwd_problem(case, dtype)
    r = RF.bwd_ratios(case, prob, _emu_bwd(case, prob, dtype, (defect,)), dtype)
    for o in outputs:
        assert r[o] >= 1.0, (defect, o, r)


# ------------------------------------------------------------------------------------------------ host logic of the model
def test_film_model_builds_with_the_reference_state_dict():
    """UNetModel(TINY, use_scale_shift_norm=True) on the CPU: the names and shapes of the model without the flag, except that every
    emb_layers.1 emits 2 * out_channels values (openaimodel.py:231-237)"""
    from stedm_amd.unet import ResBlock, UNetModel
    m = UNetModel(use_scale_shift_norm=True, **TINY)
    plain = UNetModel(**TINY)
    sd, sp = m.state_dict(), plain.state_dict()
    assert list(sd.keys()) == list(sp.keys())
    ted = TINY["model_channels"] * 4
    n_emb = 0
    for k, v in sd.items():
        if k.endswith("emb_layers.1.weight"):
            assert tuple(v.shape) == (2 * sp[k].shape[0], ted), k
            n_emb += 1
        elif k.endswith("emb_layers.1.bias"):
            assert tuple(v.shape) == (2 * sp[k].shape[0],), k
        else:
            assert tuple(v.shape) == tuple(sp[k].shape), k
    blocks = [mod for mod in m.modules() if isinstance(mod, ResBlock)]
    assert n_emb == len(blocks) == 18 and all(rb.use_scale_shift_norm for rb in blocks)       # 6 + 3 (middle: the style block's included) + 9
    assert tuple(sd["middle_block.1.block.emb_layers.1.weight"].shape) == (2 * 128, ted)
    assert tuple(sd["input_blocks.1.0.emb_layers.1.weight"].shape) == (2 * 32, ted)


def _layout(m):
    layout, n = m._emb_columns()          # the rule _prepare files the embedding rows by
    return [o for _, o in layout], n


def test_emb_layout_follows_each_blocks_width():
    from stedm_amd.unet import UNetModel
    film, plain = UNetModel(use_scale_shift_norm=True, **TINY), UNetModel(**TINY)
    of, nf = _layout(film)
    op, np_ = _layout(plain)
    cos = [rb.out_channels for rb in plain._timestep_blocks()]
    assert op == [sum(cos[:i]) for i in range(len(cos))] and np_ == sum(cos)          # a model without the flag: the layout it has today
    assert of == [2 * o for o in op] and nf == 2 * np_
    assert all(rb.emb_layers[1].out_features == rb.out_channels for rb in plain._timestep_blocks())
