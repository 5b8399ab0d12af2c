"""CPU tier of the GroupNorm tests (no GPU): tests/refs_gn.py against torch, and the two tiers of tests/test_gpu_gn_exact.py against fp32
emulations of the kernels on that file's own cases.

  references   group_norm / fold / scale_shift against F.group_norm in float64; group_norm_bwd against autograd in float64.
  exact tier   the patterns fold to mean = m_g and rstd = 1 / a_g after the float rounding, also for n = cpg * HW that is no power of two;
               the honest emulations reproduce partials, {mean, rstd} and planes bit for bit.
  bound tiers  the honest emulations stay below err / bound = 1 on every case, both formats, act 0 and 1.
  defects      every seeded defect (refs_gn.emu_* `defects`) is rejected by the exact tier, and by a bound tier where it is not exact; the
               table of which tier rejects what is printed (pytest -s) and recorded in DESIGN.md.
  offsets      correctly rounded fp32 F.group_norm stays inside the statistics-tier bound over the offset sweep; its err / bound is printed
               next to the emulation's."""
import pytest
import torch
import torch.nn.functional as F

from tests import refs_gn as R

torch.set_grad_enabled(False)


def _nchw(x, H, W):
    return x.view(x.shape[0], H, W, -1).permute(0, 3, 1, 2)


# ================================================================================================ references
@pytest.mark.parametrize("B,H,W,c1,c2,bmod,groups,act", [(2, 4, 6, 12, 0, 0, 4, 0), (4, 5, 5, 8, 16, 2, 6, 1), (3, 2, 2, 36, 28, 0, 32, 1)])
def test_references_match_torch_in_float64(B, H, W, c1, c2, bmod, groups, act):
    HW, C = H * W, c1 + c2
    x1 = R.normal((B, HW, c1), 1, "r.x1", 1.7, 0.3).double()
    x2 = R.normal((bmod or B, HW, c2), 1, "r.x2", 0.6, -0.2).double() if c2 else None
    gamma, beta = R.normal((C,), 1, "r.g", 0.3, 1.0).double(), R.normal((C,), 1, "r.b", 0.2).double()
    x = R.concat(x1, x2, bmod)
    want = F.group_norm(_nchw(x, H, W), groups, gamma, beta, 1e-5)
    want = F.silu(want) if act else want
    got = _nchw(R.group_norm(x1, x2, bmod, groups, gamma, beta, 1e-5, act), H, W)
    assert float((got - want).abs().max()) < 1e-12
    # the fold of fp64 partials (each tensor with its own slot count) gives the centred statistics
    cs1 = R.chan_partials(x1, 3)
    cs2 = R.chan_partials(x2, 5) if c2 else None
    mr = R.fold(cs1, cs2, bmod, groups, HW, 1e-5)
    assert float((mr - R.stats_of(x, groups, 1e-5)[0]).abs().max()) < 1e-11
    assert float((R.group_norm(x1, x2, bmod, groups, gamma, beta, 1e-5, act, mean_rstd=mr).reshape(-1) - got.permute(0, 2, 3, 1).reshape(-1)).abs().max()) < 1e-10
    sc, sh = R.scale_shift(x1, x2, bmod, groups, gamma, beta, 1e-5)
    y = x * sc.unsqueeze(1) + sh.unsqueeze(1)
    assert float((_nchw(R.RB.silu(y) if act else y, H, W) - want).abs().max()) < 1e-11
    # backward against autograd
    dA = R.normal((B, HW, C), 2, "r.dA").double()
    add = R.normal((B, HW, C), 2, "r.add").double()
    with torch.enable_grad():
        xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        y = F.group_norm(_nchw(xr, H, W), groups, gr, br, 1e-5)
        y = F.silu(y) if act else y
        (y * _nchw(dA, H, W)).sum().backward()
    dx, dg, db = R.group_norm_bwd(x, R.stats_of(x, groups, 1e-5)[0], groups, gamma, beta, act, dA, add)
    assert float((dx - (xr.grad + add)).abs().max()) < 1e-11
    assert float((dg - gr.grad).abs().max()) < 1e-10 and float((db - br.grad).abs().max()) < 1e-10


def test_chan_partials_slot_rule():
    x = torch.arange(2 * 20 * 4, dtype=torch.float64).view(2, 20, 4)
    assert R.slab_px(20 * 20, 2) == 256 and R.slab_px(20 * 20, 8) == 50 and R.slab_px(64, 4) == 16
    cs = R.chan_partials(x, 3)        # 7-pixel runs: 7, 7, 6
    assert torch.equal(cs[:, 2, :, 0], x[:, 14:].sum(1)) and torch.equal(cs.sum(1)[..., 1], (x * x).sum(1))
    big = R.chan_partials(torch.ones(1, 300, 4, dtype=torch.float64), 5)      # 60-pixel runs
    assert big[0, :, 0, 0].tolist() == [60.0] * 5
    over = R.chan_partials(torch.ones(1, 10, 4, dtype=torch.float64), 4)      # 3-pixel runs: 3, 3, 3, 1
    assert over[0, :, 0, 0].tolist() == [3.0, 3.0, 3.0, 1.0]
    over = R.chan_partials(torch.ones(1, 4, 4, dtype=torch.float64), 8)       # over-allocated: trailing slots stay zero
    assert over[0, :, 0, 0].tolist() == [1.0] * 4 + [0.0] * 4


def test_geometry_names_every_form():
    """the cases reach the forms their names say, by refs_gn's RESTATEMENT of the launch rules (apply16c_geometry: gn_apply16c_launch;
    gn_bwd_fused_cb, chan_stats_qbs: their namesakes). It pins the cases to the rules as written today, not to the library: whoever changes
    a launch heuristic in gn.hip / gn_bwd.hip restates it there, and this test then shows which cases moved to another instantiation."""
    got = {c[0]: R.apply16c_geometry(c[1], c[2] * c[3], c[4], c[5], c[7], c[8] == "hilo", c[8] == "x16") for c in R.FWD}
    assert all(got[n][0] == "quad" for n in got if n.startswith("quad"))
    assert got["quad_two_passes"] == ("quad", 2, 0, False) and 1024 < 2 * (1540 + 1536) // 4 < 2048      # quads of a block: two passes of 1024
    assert all(got[n][1] * (c[4] + c[5]) // 4 <= 1024 for n, c in zip(R.FWD_IDS, R.FWD) if n.startswith("quad") and n != "quad_two_passes")
    assert got["v8_pixel_tail_only"] == ("v8", 2, 0, False) and got["v8_pixel_notail"] == ("v8", 4, 0, False)
    assert got["v8_pixel_full_tail"] == ("v8", 4, 0, False) and got["v8_chan"] == ("v8", 16, 128, False) and got["v8_chan_bmod"][2] == 128
    assert got["x16_pair_chan"] == ("o8", 4, 128, True) and got["x16_pair_pixel"] == ("o8", 3, 0, True) and got["x16_pixel_notail"] == ("o8", 4, 0, True)
    assert got["x16_unpaired"] == ("o8", 1, 0, False) and got["x16_straddle"] == ("o8", 1, 0, True)
    # block runs: quads (octets) of a block against the 512 (256) of one iteration
    assert 4 * 512 // 4 == 512 and 4 * 640 // 4 == 512 + 128 and 4 * 512 // 8 == 256 and 3 * 256 // 8 < 256
    bw = {c[0]: R.gn_bwd_fused_cb(c[4], c[5], c[6], c[2] * c[3]) for c in R.BWD}
    assert bw["fused_ppt2"][1] == 2 and bw["fused_ppt4"][1] == 4 and 4 < bw["fused_ppt8"][1] <= 8 and bw["fused_ragged"][0] > 0
    assert all(bw[n] == (0, 0) for n in bw if n.startswith("chain"))
    qb = [R.chan_stats_qbs(c[0], (c[2] * c[3] + 255) // 256 * c[4] + c[5], c[1] // 4) for c in R.CHAN_STATS]
    assert qb == [8, 8, 64, 32, 16, 8, 8, 8]


# ================================================================================================ exact tier
@pytest.mark.parametrize("kind", ["A", "B"])
def test_exact_pattern_folds_to_m_and_one_over_a(kind):
    """mean = m_g and rstd = 1 / a_g after the float rounding, for powers of two and for n = cpg * HW in {600, 49152 * 3, 100 * 6, ...}"""
    for B, HW, c1, c2, bmod, groups in [(2, 64, 36, 28, 0, 32), (3, 100, 36, 12, 2, 8), (1, 4096, 72, 24, 0, 8), (2, 400, 64, 32, 0, 8), (2, 64, 8, 8, 0, 1)]:
        x1, x2, sign, mr = R.exact_pattern(B, HW, c1, c2, bmod, groups, kind)
        cs1 = R.chan_partials(x1.double())
        cs2 = R.chan_partials(x2.double())
        assert torch.equal(cs1.float().double(), cs1) and torch.equal(cs2.float().double(), cs2)       # every partial is an fp32 number
        got = R.fold(cs1.float(), cs2.float(), bmod, groups, HW, 0.0).float()
        assert torch.equal(got, mr), (B, HW, c1, c2)
        # the kernels' own arithmetic (s * (1 / n), not s / n) lands on the same floats
        s = R._group_sums(cs1, cs2, bmod, groups)
        inv_n = 1.0 / float((c1 + c2) // groups * HW)
        mean = s[..., 0] * inv_n
        assert torch.equal(torch.stack([mean, 1.0 / torch.sqrt(s[..., 1] * inv_n - mean * mean)], -1).float(), mr)
        assert int(sign.sum()) == 0 and bool((sign.sum(1) == 0).all())


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("case", R.FWD, ids=R.FWD_IDS)
def test_forward_emulation_inside_both_tiers(case, prec):
    dtype = R.dt(prec)
    x1, x2, gamma, beta = R.fwd_inputs(case)
    for c in R.forms(case):
        for kind in "AB":
            exp = R.fwd_exact_problem(c, kind, dtype)
            out = R.emu_forward(c, exp["x1"], exp["x2"], exp["gamma"], exp["beta"], 0.0, 0, dtype)
            assert R.exact_mismatches(exp, out) == [], (c[0], c[8], kind)
        for act, eps in ((0, 1e-5), (1, 1e-6)):
            out = R.emu_forward(c, x1, x2, gamma, beta, eps, act, dtype)
            r = R.fwd_ratios(c, x1, x2, gamma, beta, eps, act, dtype, out)
            print(f"{c[0]} {c[8]} {prec} act {act}: err/bound " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
            assert max(r.values()) < 1.0, r
            raw_ref = R.concat(R.x16_words(x1, dtype).view(dtype).float() if c[8] == "x16" else x1, x2, c[6]).to(dtype).contiguous().view(torch.int16)
            assert torch.equal(out["raw"], raw_ref)


def _bwd_emu(case, act, dtype, planes, acc1, acc2, use_add, acc_param, defects=(), exact=None):
    name, B, H, W, c1, c2, groups = case
    HW, C = H * W, c1 + c2
    if exact:
        x1, x2, sign, mr = R.exact_pattern(B, HW, c1, c2, 0, groups, exact)
        gamma, beta = R.dyadic_affine(C)
        dA, dx_want, dg_want, db_want = R.exact_bwd(sign, mr, groups, gamma, B, HW, C)
        add = R.RB.dyadic((B, HW, C), 3) if use_add else None
        old = R.RB.dyadic((B, HW, C), 4)
    else:
        x1, x2, gamma, beta, dA, add, old = R.bwd_inputs(case)
        add = add if use_add else None
        mr = R.emu_fold(R.emu_chan_stats(x1), R.emu_chan_stats(x2) if c2 else None, 0, groups, HW, 1e-5)
    old1 = old[..., :c1].contiguous() if acc1 else None
    old2 = old[..., c1:].contiguous() if (acc2 and c2) else None
    dg0 = torch.arange(C, dtype=torch.float32) / 4.0 if acc_param else None
    db0 = -torch.arange(C, dtype=torch.float32) / 8.0 if acc_param else None
    out = R.emu_gn_bwd(x1, x2, mr, groups, gamma, beta, act, dA, add, old1, old2, acc1, acc2, dtype, planes, dg0, db0, acc_param, defects)
    if exact:
        want = dx_want + (add if use_add else 0.0)
        wold = torch.zeros_like(want)
        if acc1:
            wold[..., :c1] = old1
        if acc2 and c2:
            wold[..., c1:] = old2
        want = want + wold
        exp = dict(dx1=want[..., :c1].contiguous(), dx2=want[..., c1:].contiguous() if c2 else None,
                   dgamma=dg_want + (dg0 if acc_param else 0.0), dbeta=db_want + (db0 if acc_param else 0.0))
        if planes:
            exp["hi"], exp["lo"] = R._split(want, dtype, planes == "hilo")
        return R.exact_mismatches(exp, out, ("dx1", "dx2", "dgamma", "dbeta", "hi", "lo"))
    return R.bwd_ratios(case, x1, x2, mr, gamma, beta, act, dA, add, old1, old2, dtype, planes, dg0, db0, out)


@pytest.mark.parametrize("case", R.BWD, ids=R.BWD_IDS)
def test_backward_emulation_inside_both_tiers(case):
    for prec, planes, acc1, acc2, use_add, accp in [("f16", "hilo", False, True, True, False), ("bf16", "hi", True, False, False, True)]:
        for kind in "AB":
            assert _bwd_emu(case, 0, R.dt(prec), planes, acc1, acc2, use_add, accp, exact=kind) == [], (case[0], kind)
        for act in (0, 1):
            r = _bwd_emu(case, act, R.dt(prec), planes, acc1, acc2, use_add, accp)
            print(f"{case[0]} {prec} act {act}: err/bound " + " ".join(f"{k} {v:.3f}" for k, v in r.items()))
            assert max(r.values()) < 1.0, r


# ================================================================================================ seeded defects
# defect -> the cases on which it is live
FWD_DEFECTS = {
    "fold_last_slot": ["v8_pixel_tail_only", "x16_pair_pixel"], "cs2_row": ["v8_chan_bmod", "x16_g64"], "quad_group": ["quad_cpg2", "quad_cpg6"],
    "cut_table": ["v8_chan", "x16_pair_chan"], "nslab1_both": ["quad_cpg6", "x16_pair_pixel"], "lo_unrounded": ["v8_hilo", "quad_cpg6"],
    "tail": ["v8_pixel_full_tail", "x16_pair_pixel"], "x16_rewrite": ["x16_unpaired"], "x16_skip": ["x16_unpaired"], "stats_tail": ["v8_pixel_tail_only"],
}


@pytest.mark.parametrize("defect", sorted(FWD_DEFECTS))
def test_forward_defect_is_rejected(defect):
    for name in FWD_DEFECTS[defect]:
        case = R.FWD[R.FWD_IDS.index(name)]
        dtype = torch.bfloat16
        exact = []
        for kind in "AB":
            exp = R.fwd_exact_problem(case, kind, dtype)
            exact += R.exact_mismatches(exp, R.emu_forward(case, exp["x1"], exp["x2"], exp["gamma"], exp["beta"], 0.0, 0, dtype, defects=(defect,)))
        x1, x2, gamma, beta = R.fwd_inputs(case)
        out = R.emu_forward(case, x1, x2, gamma, beta, 1e-5, 1, dtype, defects=(defect,))
        r = R.fwd_ratios(case, x1, x2, gamma, beta, 1e-5, 1, dtype, out)
        raw_ref = R.concat(R.x16_words(x1, dtype).view(dtype).float() if case[8] == "x16" else x1, x2, case[6]).to(dtype).contiguous().view(torch.int16)
        raw_bad = not torch.equal(out["raw"], raw_ref)
        print(f"defect {defect} on {name}: exact tier {'rejects' if exact else 'PASSES'} ({'; '.join(exact[:3])}); bound tier worst err/bound "
              f"{max(r.values()):.3g} ({'rejects' if max(r.values()) > 1 or raw_bad else 'PASSES'})")
        if defect == "lo_unrounded":      # lo == 0 is what the exact pattern expects: only the bound tier (hi + lo residual) separates it
            assert not exact and r["apply"] > 1.0
        else:
            assert exact, (defect, name)
            assert max(r.values()) > 1.0 or raw_bad, (defect, name, r)


def test_variance_clamp_defect_is_rejected():
    """a non-dyadic constant group: fp32 partials make q / n - mean^2 negative for some constants; without the clamp the value is NaN"""
    sw = R.SWEEP[0]
    x, gamma, beta = R.sweep_inputs(sw, 0.0)
    C, groups = sw[4], sw[5]
    cs = R.emu_chan_stats(x)
    mr = R.emu_fold(cs, None, 0, groups, 16, 1e-5)
    out = R.emu_apply16c(x, None, 0, mr, groups, gamma, beta, 0, torch.float16, True, ("quad", 1, 0, False), C)
    r, _, nerr, const_ok = R.sweep_ratio(sw, x, gamma, beta, 1e-5, torch.float16, out["hi"], out["lo"], R.chan_stats_k(sw[1], C, 16, 1))
    assert r < 1.0 and const_ok and bool(torch.isfinite(mr).all())
    # the clamp matters when the rounded partials give a negative variance: seek such a constant among a fixed list, and hold the defect to it
    hit = 0
    for cval in (1234.567, 0.1, 3.3, 1e3 / 7, 77.7, 0.7, 12345.678):
        xc = torch.full((1, 16, 8), cval)
        csc = R.emu_chan_stats(xc)
        if float(R.fold(csc, None, 0, 1, 16, 0.0, clamp=False)[0, 0, 1].nan_to_num(nan=-1.0)) < 0:
            hit += 1
            bad = R.emu_fold(csc, None, 0, 1, 16, 0.0, ("no_clamp",))
            assert not bool(torch.isfinite(bad[0, 0, 1]))
            good = R.emu_fold(csc, None, 0, 1, 16, 1e-5)
            assert bool(torch.isfinite(good).all())
    print(f"variance clamp: {hit} of 7 constants give a negative one-pass variance from fp32 partials")
    assert hit > 0


BWD_DEFECTS = {"acc2": (False, True), "acc_param": (True, True), "add_planes": (False, False), "x2_means": (False, False)}


@pytest.mark.parametrize("defect", sorted(BWD_DEFECTS))
def test_backward_defect_is_rejected(defect):
    acc1, acc2 = BWD_DEFECTS[defect]
    for name in ("fused_ppt2", "chain_ragged_cpg6"):
        case = R.BWD[R.BWD_IDS.index(name)]
        exact = []
        for kind in "AB":
            exact += _bwd_emu(case, 0, torch.float16, "hilo", acc1, acc2, True, True, defects=(defect,), exact=kind)
        r = _bwd_emu(case, 1, torch.float16, "hilo", acc1, acc2, True, True, defects=(defect,))
        print(f"defect {defect} on {name}: exact tier {'rejects' if exact else 'PASSES'} ({'; '.join(exact[:3])}); bound tier worst err/bound {max(r.values()):.3g}")
        assert exact and max(r.values()) > 1.0, (defect, name, exact, r)


# ================================================================================================ offset sweep
@pytest.mark.parametrize("sw", R.SWEEP, ids=[s[0] for s in R.SWEEP])
def test_offset_sweep_fp32_group_norm_and_emulation_inside_the_statistics_bound(sw):
    name, B, H, W, C, groups = sw
    HW = H * W
    k = R.chan_stats_k(B, C, HW, 0)
    for mu in R.OFFSETS:
        x, gamma, beta = R.sweep_inputs(sw, mu)
        y32 = F.group_norm(_nchw(x, H, W), groups, gamma, beta, 1e-5).permute(0, 2, 3, 1).reshape(B, HW, C)
        hi, lo = R._split(y32, torch.float16, True)
        a_t, r_t, n_t, _ = R.sweep_ratio(sw, x, gamma, beta, 1e-5, torch.float16, hi, lo, k)
        mr = R.emu_fold(R.emu_chan_stats(x), None, 0, groups, HW, 1e-5)
        out = R.emu_apply16c(x, None, 0, mr, groups, gamma, beta, 0, torch.float16, True, ("quad", 1, 0, False), C)
        a_e, r_e, n_e, ok = R.sweep_ratio(sw, x, gamma, beta, 1e-5, torch.float16, out["hi"], out["lo"], k)
        mr2 = R.emu_gn_stats_fold(x, None, 0, groups, 1e-5)
        out2 = R.emu_apply16c(x, None, 0, mr2, groups, gamma, beta, 0, torch.float16, True, ("quad", 1, 0, False), C)
        a_s, r_s, n_s, ok2 = R.sweep_ratio(sw, x, gamma, beta, 1e-5, torch.float16, out2["hi"], out2["lo"], R.gn_stats_k(C, HW))
        sc, sh = R.emu_scale_shift(x, None, 0, groups, gamma, beta, 1e-5)
        sc64, sh64 = R.scale_shift(x.double(), None, 0, groups, gamma.double(), beta.double(), 1e-5)
        e_sc, e_sh = R.scale_shift_bound(x.double(), groups, gamma.double(), beta.double(), 1e-5, True)
        r_c = max(R.ratio((sc.double() - sc64).abs(), e_sc), R.ratio((sh.double() - sh64).abs(), e_sh))
        print(f"{name} mu/sigma {mu:6.0f}: err/bound F.group_norm fp32 {r_t:.3f} | chan_stats emulation {r_e:.3f} | gn_stats emulation {r_s:.3f} | "
              f"scale_shift emulation {r_c:.3f}; worst |err| of a normalised value {n_t:.2e} | {n_e:.2e} | {n_s:.2e}")
        assert max(r_t, a_t) < 1.0 and max(r_e, a_e) < 1.0 and max(r_s, a_s) < 1.0 and r_c < 1.0 and ok and ok2
