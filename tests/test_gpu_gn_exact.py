"""GPU tier (-m gpu): the GroupNorm kernels (stedm_amd/csrc/gn.hip, gn_fold / gn_bwd in gn_bwd.hip) against tests/refs_gn.py, in two tiers.

  exact   inputs m_g +- a_g (refs_gn.exact_pattern; 'A' alternating signs, 'B' a fixed shuffle with m_g distinct per sample), eps = 0,
          dyadic gamma / beta, act = 0: the fp32 partials, {mean, rstd} and every plane word are known bit for bit - torch.equal on the
          partials, on the mean_rstd side output / gn_fold, and on the planes (hi + lo where the entry takes it, lo == 0, and single-product).
  bound   N(0.3, 1.7) | N(-0.2, 0.6) data, act 0 and 1, eps 1e-5 and 1e-6: per-element err / bound < 1 against the fp64 reference, for
          the apply tier (statistics given: fold() of the kernel's own partials) and the statistics tier (end to end), bounds derived in
          refs_gn's docstring from each kernel's rounding points. Every case prints its worst err / bound.
Every output is filled with NaN / 0x7e7e first and must be written everywhere; the [0, c1) half of the X16 form's raw plane must keep
its words. tests/test_gn_refs_cpu.py holds fp32 emulations of the kernels to the same checks, and seeded defects outside them.

Kernel instantiation -> case. The branch rules are RESTATED in Python (refs_gn.apply16c_geometry / gn_bwd_fused_cb / chan_stats_qbs) and the
mapping is asserted against that restatement on the CPU tier (test_geometry_names_every_form), as the guard tests do: a change of a launch
heuristic in gn.hip / gn_bwd.hip has to be restated there, or cases silently move to other instantiations. Every stedm_gn_apply16c case runs
single-product and hi + lo in both tiers (refs_gn.forms; both modes of an 8-wide shape run in the quad-pair kernel):

  gn_scale_shift_kernel<true>                cpg, c1, c2 multiples of 4                      test_scale_shift[vec4*]
  gn_scale_shift_kernel<false>               cpg = 6 / c1 = 6                                test_scale_shift[scalar*]
  gn_stats_kernel                            Q = C / 4 <= 256 (npl lanes) and Q = 384 > 256 (2 slots per thread), bmod
                                                                                             test_gn_stats_apply16 (f16 / bf16 x single / hi + lo)
  gn_apply16_kernel<_Float16 / __bf16>       the same cases; gamma == NULL: plain conversion test_gn_stats_apply16, test_apply16_plain_conversion
  gn_chan_stats_kernel<__bf16, false>        block widths qbs 8 / 16 / 32 / 64, C = 4 and 1536, ragged last slot (20 x 20), caller-chosen
                                             partition (4 x default), over-allocated (trailing zero slots)   test_chan_stats
  gn_chan_stats_kernel<_Float16 / __bf16, true>   the same statistics + the plain planes (hi, hi + lo)        test_chan_stats16
  gn_fold_kernel                             every forward case (nslab1 != nslab2 in the cases with a 4 x partition; groups 1, 8, 16, 32, 64)
  gn_apply16c_kernel<_Float16 / __bf16>      c1 % 8 != 0: quad_cpg2, quad_cpg6 (per-element group lookup), quad_cpg4_c1_4 (cpg % 4 == 0),
                                             quad_g64 (L = 4 lanes per group), quad_two_passes (1538 quads per block: the loop runs twice,
                                             second load_batch, cursor advance and wrap; the others have <= 1024 and run it once)
  gn_apply16c_v8_kernel<T>                   pixel runs: v8_pixel_tail_only (96 quads < 512), v8_pixel_notail (4 px x 128 quads = 512),
                                             v8_pixel_full_tail (640 = 512 + 128), v8_hilo (hi + lo keeps this kernel), v8_g1, v8_cpg5;
                                             channel runs cb = 128: v8_chan, v8_chan_bmod (hi + lo)
  gn_apply16c_o8_kernel<T, true>             stedm_gn_apply16c_x16, PAIR: x16_pair_chan (cb = 128, bmod, nslab1 = 4 nslab2), x16_pair_pixel
                                             (tail only), x16_pixel_notail (4 px x 64 octets = 256), x16_c2_0, x16_straddle (1024 + 512,
                                             cpg 48: groups across the seam), x16_g64
  gn_apply16c_o8_kernel<T, false>            c1 = 136: no multiple of 16: x16_unpaired
  gn_bwd_fused_kernel<T, 2 / 4 / 8>          fused_ppt2, fused_ppt4 / fused_ragged (10 x 10) / fused_g64, fused_ppt8 (ppt 7)
  gn_bwd_stats / _fold / _apply_kernel<T>    no admissible channel run: chain_c1536 (1024 + 512), chain_64x64 (ppt > 8), chain_ragged_cpg6
  gn_bwd_param_kernel                        every backward case; accumulate on and off
"""
import pytest
import torch

from tests import refs_gn as R

pytestmark = pytest.mark.gpu

torch.set_grad_enabled(False)

NAN = float("nan")
FILL16 = R.FILL16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stedm_amd import _lib
    _lib.lib()  # must load: no fallback
    return torch.device("cuda:0")


def _prec(prec, hilo):
    from stedm_amd import ops
    return ops.Precision(ops.Precision.parse(prec).mm_dtype, 3 if hilo else 1)


def _written(name, *planes):
    for p in planes:
        if p is not None:
            if p.dtype == torch.int16:
                assert not bool((p == FILL16).any()), f"{name}: words left unwritten"
            else:
                assert not bool(torch.isnan(p).any()), f"{name}: values left unwritten"


def _run_fwd(dev, case, x1, x2, gamma, beta, eps, act, prec, with_raw=True):
    """gn_chan_stats of both tensors (their own slot counts), gn_fold, then the apply entry of the case's form with every optional output.
    Returns the CPU outputs refs_gn.fwd_ratios / exact_mismatches read."""
    from stedm_amd import ops
    name, B, H, W, c1, c2, bmod, groups, form, _, _ = case
    _, HW, _, _, _, _, _, ns1, ns2 = R.case_dims(case)
    C, dtype, hilo = c1 + c2, R.dt(prec), form == "hilo"
    pr = _prec(prec, hilo)
    d1 = x1.view(B, H, W, c1).to(dev)
    d2 = x2.view(x2.shape[0], H, W, c2).to(dev) if c2 else None
    g_, b_ = gamma.to(dev), beta.to(dev)
    cs1 = torch.full((B, ns1, c1, 2), NAN, device=dev); ops.gn_chan_stats(d1, cs1)
    cs2 = None
    if c2:
        cs2 = torch.full((d2.shape[0], ns2, c2, 2), NAN, device=dev); ops.gn_chan_stats(d2, cs2)
    mr_fold = torch.full((B, groups, 2), NAN, device=dev)
    cs2_rows = cs2[torch.arange(B, device=dev) % bmod].contiguous() if (c2 and bmod) else cs2       # gn_fold has no bmod: hand it the rows
    ops.gn_fold(cs1, cs2_rows, groups, HW, eps, mr_fold)
    hi = torch.full((B, H, W, C), FILL16, dtype=torch.int16, device=dev)
    raw = torch.full_like(hi, FILL16) if (with_raw or form == "x16") else None
    lo = torch.full_like(hi, FILL16) if hilo else None
    rlo = torch.full_like(hi, FILL16) if (hilo and with_raw) else None
    mr = None
    if form == "x16":
        words = R.x16_words(x1, dtype).view(B, H, W, c1).to(dev)
        raw[..., :c1] = words
        ops.gn_apply16c_x16(c1, cs1, d2, cs2, hi, raw, pr, g_, b_, eps, groups, act, bmod)
        torch.cuda.synchronize()
        assert torch.equal(raw[..., :c1], words), f"{name}: the [0, c1) half of the raw plane was rewritten"
    else:
        mr = torch.full((B, groups, 2), NAN, device=dev)
        ops.gn_apply16c(d1, cs1, d2, cs2, hi, lo, pr, g_, b_, eps, groups, act, bmod, raw=(raw, rlo) if with_raw else None, mean_rstd=mr)
        torch.cuda.synchronize()
    _written(name, cs1, cs2, mr_fold, mr, hi, lo, raw, rlo)
    cpu = lambda t: None if t is None else t.cpu().view(t.shape[0], -1, t.shape[-1]) if t.dtype == torch.int16 else t.cpu()
    return dict(cs1=cpu(cs1), cs2=cpu(cs2), mr=cpu(mr_fold), mr_side=cpu(mr), hi=cpu(hi), lo=cpu(lo), raw=cpu(raw), raw_lo=cpu(rlo),
                x16=R.x16_words(x1, dtype).view(dtype).double() if form == "x16" else None)


def _raw_ref(case, x1, x2, dtype):
    src1 = R.x16_words(x1, dtype).view(dtype).float() if case[8] == "x16" else x1
    return R.concat(src1, x2, case[6])


def _exact_case(dev, case, prec, with_raw=True):
    dtype = R.dt(prec)
    for kind in "AB":
        exp = R.fwd_exact_problem(case, kind, dtype)
        out = _run_fwd(dev, case, exp["x1"], exp["x2"], exp["gamma"], exp["beta"], 0.0, 0, prec, with_raw)
        bad = R.exact_mismatches(exp, out)
        if out.get("mr_side") is not None and not torch.equal(out["mr_side"], exp["mr"]):
            bad.append("mean_rstd side output")
        assert bad == [], f"{case[0]} {prec} pattern {kind}: {bad}"


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("case", R.FWD, ids=R.FWD_IDS)
def test_forward_exact(dev, case, prec):
    """exact tier of every apply form: partials, gn_fold, the mean_rstd side output and all planes bit for bit. Every stedm_gn_apply16c case
    runs single-product AND hi + lo (lo == 0), with the raw planes and without (where the mode changes the kernel, the docstring table says so)"""
    for c in R.forms(case):
        _exact_case(dev, c, prec)
        if c[8] != "x16":       # without the raw planes (the X16 form always has its raw plane)
            _exact_case(dev, c, prec, with_raw=False)


@pytest.mark.parametrize("prec", ["f16", "bf16"])
@pytest.mark.parametrize("case", R.FWD, ids=R.FWD_IDS)
def test_forward_bounds(dev, case, prec):
    """bound tiers of every apply form, single-product and hi + lo, act 0 / eps 1e-5 and act 1 / eps 1e-6; the raw planes are torch's own
    cast, bit for bit; gn_fold and the side output agree within the fold's own bound, and bitwise where they share the lane partition"""
    dtype = R.dt(prec)
    x1, x2, gamma, beta = R.fwd_inputs(case)
    B, HW, bmod, groups = case[1], case[2] * case[3], case[6], case[7]
    for c in R.forms(case):
        for act, eps in ((0, 1e-5), (1, 1e-6)):
            out = _run_fwd(dev, c, x1, x2, gamma, beta, eps, act, prec)
            r = R.fwd_ratios(c, x1, x2, gamma, beta, eps, act, dtype, out)
            ndiff = -1
            if out["mr_side"] is not None:
                r["mr_side"] = R.ratio((out["mr_side"].double() - R.fold(out["cs1"], out["cs2"], bmod, groups, HW, eps)).abs(),
                                       R.mean_rstd_bound(out["cs1"], out["cs2"], bmod, groups, HW, eps))
                ndiff = int((out["mr_side"] != out["mr"]).sum())
            print(f"{c[0]} {c[8]} {prec} act {act} eps {eps:g}: worst err/bound " + " ".join(f"{k} {v:.3f}" for k, v in r.items()) +
                  f"; gn_fold vs side output: {ndiff} words differ")
            assert max(r.values()) < 1.0, r
            if R.apply16c_geometry(B, HW, c[4], c[5], groups, c[8] == "hilo", c[8] == "x16")[2] == 0 and ndiff >= 0:
                assert ndiff == 0      # pixel-run blocks fold with gn_fold's own lane partition (L = 256 / groups): the same sums in the same order
            rh, rl = R._split(_raw_ref(c, x1, x2, dtype), dtype, c[8] == "hilo")
            assert torch.equal(out["raw"], rh) and (rl is None or torch.equal(out["raw_lo"], rl)), f"{c[0]}: raw planes"


# ================================================================================================ gn_chan_stats / gn_chan_stats16
def _chan_case(c):
    B, C, H, W, mult, extra = c
    return B, C, H, W, (H * W + 255) // 256 * mult + extra


@pytest.mark.parametrize("c", R.CHAN_STATS, ids=[f"B{c[0]}_C{c[1]}_{c[2]}x{c[3]}_m{c[4]}_x{c[5]}" for c in R.CHAN_STATS])
def test_chan_stats(dev, c):
    """gn_chan_stats_kernel at every block width, exact on the pattern and within gamma_k sum|x| / gamma_(k+1) sum x^2 per slot on normal data;
    trailing slots of an over-allocated partition are zero; run to run bitwise"""
    from stedm_amd import ops
    B, C, H, W, ns = _chan_case(c)
    HW = H * W
    groups = 4 if C % 4 == 0 and C > 4 else 1
    xe = R.exact_pattern(B, HW, C, 0, 0, groups, "B")[0]
    for x, exact in ((xe, True), (R.normal((B, HW, C), 3, "cs", 1.7, 0.3), False)):
        cs = torch.full((B, ns, C, 2), NAN, device=dev)
        ops.gn_chan_stats(x.view(B, H, W, C).to(dev), cs)
        cs_again = torch.full_like(cs, NAN)
        ops.gn_chan_stats(x.view(B, H, W, C).to(dev), cs_again)
        torch.cuda.synchronize()
        assert torch.equal(cs, cs_again)
        got = cs.cpu()
        if exact:
            assert torch.equal(got, R.chan_partials(x.double(), ns).float())
        else:
            r = R.partials_ratio(x, got)
            print(f"gn_chan_stats B {B} C {C} HW {HW} nslab {ns} qbs {R.chan_stats_qbs(B, ns, C // 4)}: worst err/bound {r:.3f}")
            assert r < 1.0
        used = (HW + R.slab_px(HW, ns) - 1) // R.slab_px(HW, ns)
        assert bool((got[:, used:] == 0).all())


@pytest.mark.parametrize("prec,hilo", [("f16", False), ("f16", True), ("bf16", False), ("bf16", True)])
def test_chan_stats16(dev, prec, hilo):
    """gn_chan_stats_kernel<T, CAST>: the partials bit for bit on the exact pattern and inside the same per-slot bound on normal data (the two
    instantiations contract x * x + q differently: equal to rounding, each bitwise run to run), and the planes torch's own cast (hi, lo = x - hi)"""
    from stedm_amd import ops
    for c in (R.CHAN_STATS[1], R.CHAN_STATS[3], R.CHAN_STATS[6]):
        B, C, H, W, ns = _chan_case(c)
        xe = R.exact_pattern(B, H * W, C, 0, 0, 4, "B")[0]
        for x, exact in ((xe, True), (R.normal((B, H * W, C), 4, "cs16", 1.7, 0.3), False)):
            d = x.view(B, H, W, C).to(dev)
            outs = []
            for _ in range(2):
                cs16 = torch.full((B, ns, C, 2), NAN, device=dev)
                hi = torch.full((B, H, W, C), FILL16, dtype=torch.int16, device=dev)
                lo = torch.full_like(hi, FILL16) if hilo else None
                ops.gn_chan_stats16(d, cs16, hi, lo, _prec(prec, hilo))
                torch.cuda.synchronize()
                outs.append((cs16.cpu(), hi.cpu().view(B, -1, C), None if lo is None else lo.cpu().view(B, -1, C)))
            assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
            cs16, hi, lo = outs[0]
            if exact:
                assert torch.equal(cs16, R.chan_partials(x.double(), ns).float())
            else:
                r = R.partials_ratio(x, cs16)
                print(f"gn_chan_stats16 {prec}{' hi+lo' if hilo else ''} B {B} C {C} HW {H * W} nslab {ns}: worst err/bound {r:.3f}")
                assert r < 1.0
            rh, rl = R._split(x, R.dt(prec), hilo)
            assert torch.equal(hi, rh) and (not hilo or torch.equal(lo, rl))


# ================================================================================================ gn_stats + gn_apply16, gn_scale_shift
# (id, B, H, W, c1, c2, bmod, groups)
STATS16 = [("q_le_256", 2, 10, 10, 64, 32, 0, 8), ("q_gt_256_bmod", 4, 8, 8, 1024, 512, 2, 32), ("cpg6", 2, 8, 8, 36, 12, 0, 8)]


def _run_stats16(dev, case, x1, x2, gamma, beta, eps, act, prec, hilo):
    from stedm_amd import ops
    name, B, H, W, c1, c2, bmod, groups = case
    C = c1 + c2
    d1 = x1.view(B, H, W, c1).to(dev)
    d2 = x2.view(x2.shape[0], H, W, c2).to(dev)
    stats = torch.full((B * ops.gn_nslab(C, H * W) * groups * 2,), NAN, dtype=torch.float64, device=dev)
    ops.gn_stats(d1, d2, stats, groups, bmod)
    hi = torch.full((B, H, W, C), FILL16, dtype=torch.int16, device=dev)
    lo = torch.full_like(hi, FILL16) if hilo else None
    ops.gn_apply16(d1, d2, hi, lo, _prec(prec, hilo), None if gamma is None else gamma.to(dev), None if beta is None else beta.to(dev), eps, groups, act,
                   stats, bmod)
    torch.cuda.synchronize()
    _written(name, stats, hi, lo)
    return hi.cpu().view(B, -1, C), None if lo is None else lo.cpu().view(B, -1, C)


@pytest.mark.parametrize("prec,hilo", [("f16", False), ("f16", True), ("bf16", False), ("bf16", True)])
@pytest.mark.parametrize("case", STATS16, ids=[c[0] for c in STATS16])
def test_gn_stats_apply16(dev, case, prec, hilo):
    name, B, H, W, c1, c2, bmod, groups = case
    HW, C, dtype = H * W, c1 + c2, R.dt(prec)
    x1, x2, sign, mr = R.exact_pattern(B, HW, c1, c2, bmod, groups, "B")
    gamma, beta = R.dyadic_affine(C)
    hi, lo = _run_stats16(dev, case, x1, x2, gamma, beta, 0.0, 0, prec, hilo)
    assert torch.equal(hi, R.exact_planes(sign, gamma, beta, dtype)) and (lo is None or not bool(lo.any()))
    x1, x2 = R.normal((B, HW, c1), 7, "s16.x1", 1.7, 0.3), R.normal((bmod or B, HW, c2), 7, "s16.x2", 0.6, -0.2)
    gamma, beta = R.normal((C,), 7, "s16.g", 0.3, 1.0), R.normal((C,), 7, "s16.b", 0.2)
    x64 = R.concat(x1, x2, bmod).double()
    for act, eps in ((0, 1e-5), (1, 1e-6)):
        hi, lo = _run_stats16(dev, case, x1, x2, gamma, beta, eps, act, prec, hilo)
        mr64 = R.stats_of(x64, groups, eps)[0]
        em, drstd = R.stats_shift(x64, groups, eps, R.gn_stats_k(C, HW), fold_terms=64)
        ref = R.group_norm(x64, None, 0, groups, gamma.double(), beta.double(), eps, act, mean_rstd=mr64)
        r = R.ratio((R.planes_value(hi, lo, dtype) - ref).abs(), R.apply_bound(x64, mr64, gamma.double(), beta.double(), act, dtype, hilo, em, drstd))
        print(f"gn_stats + gn_apply16 {name} {prec}{' hi+lo' if hilo else ''} act {act}: worst err/bound {r:.3f}")
        assert r < 1.0


@pytest.mark.parametrize("prec,hilo", [("f16", False), ("f16", True), ("bf16", False), ("bf16", True)])
def test_apply16_plain_conversion(dev, prec, hilo):
    case = STATS16[0]
    name, B, H, W, c1, c2, bmod, groups = case
    x1, x2 = R.normal((B, H * W, c1), 8, "pc.x1", 1.7, 0.3), R.normal((B, H * W, c2), 8, "pc.x2", 0.6, -0.2)
    from stedm_amd import ops
    hi = torch.full((B, H, W, c1 + c2), FILL16, dtype=torch.int16, device=dev)
    lo = torch.full_like(hi, FILL16) if hilo else None
    ops.gn_apply16(x1.view(B, H, W, c1).to(dev), x2.view(B, H, W, c2).to(dev), hi, lo, _prec(prec, hilo))
    torch.cuda.synchronize()
    rh, rl = R._split(R.concat(x1, x2, 0), R.dt(prec), hilo)
    assert torch.equal(hi.cpu().view(B, -1, c1 + c2), rh) and (not hilo or torch.equal(lo.cpu().view(B, -1, c1 + c2), rl))


SCALE_SHIFT = [("vec4", 2, 10, 10, 64, 32, 0, 8), ("vec4_bmod", 4, 8, 8, 256, 256, 2, 32), ("scalar_cpg6", 2, 8, 8, 36, 12, 0, 8), ("scalar_c1_6", 3, 5, 5, 6, 10, 0, 4)]


@pytest.mark.parametrize("case", SCALE_SHIFT, ids=[c[0] for c in SCALE_SHIFT])
def test_scale_shift(dev, case):
    from stedm_amd import ops
    name, B, H, W, c1, c2, bmod, groups = case
    HW, C = H * W, c1 + c2
    vec4 = (C // groups) % 4 == 0 and c1 % 4 == 0 and c2 % 4 == 0
    assert vec4 == name.startswith("vec4")

    def run(x1, x2, gamma, beta, eps):
        sc, sh = torch.full((B, C), NAN, device=dev), torch.full((B, C), NAN, device=dev)
        ops.gn_scale_shift(x1.view(B, H, W, c1).to(dev), x2.view(x2.shape[0], H, W, c2).to(dev), gamma.to(dev), beta.to(dev), eps, sc, sh, groups, bmod)
        torch.cuda.synchronize()
        _written(name, sc, sh)
        return sc.cpu(), sh.cpu()
    if HW % 2 == 0:      # exact: scale = gamma / a_g, shift = beta - m_g gamma / a_g (dyadic, a few bits)
        x1, x2, sign, mr = R.exact_pattern(B, HW, c1, c2, bmod, groups, "B")
        gamma, beta = R.dyadic_affine(C)
        sc, sh = run(x1, x2, gamma, beta, 0.0)
        esc = R.per_channel(mr[..., 1], C)[:, 0] * gamma
        assert torch.equal(sc, esc) and torch.equal(sh, beta - R.per_channel(mr[..., 0], C)[:, 0] * esc)
    x1, x2 = R.normal((B, HW, c1), 9, "ss.x1", 1.7, 0.3), R.normal((bmod or B, HW, c2), 9, "ss.x2", 0.6, -0.2)
    gamma, beta = R.normal((C,), 9, "ss.g", 0.3, 1.0), R.normal((C,), 9, "ss.b", 0.2)
    sc, sh = run(x1, x2, gamma, beta, 1e-5)
    x64 = R.concat(x1, x2, bmod).double()
    sc64, sh64 = R.scale_shift(x64, None, 0, groups, gamma.double(), beta.double(), 1e-5)
    e_sc, e_sh = R.scale_shift_bound(x64, groups, gamma.double(), beta.double(), 1e-5, vec4)
    r = (R.ratio((sc.double() - sc64).abs(), e_sc), R.ratio((sh.double() - sh64).abs(), e_sh))
    print(f"gn_scale_shift {name}: worst err/bound scale {r[0]:.3f} shift {r[1]:.3f}")
    assert max(r) < 1.0


# ================================================================================================ offset sweep
@pytest.mark.parametrize("sw", R.SWEEP, ids=[s[0] for s in R.SWEEP])
def test_offset_sweep(dev, sw):
    """x = mu + z, mu / sigma in {0, 4, 32, 256, 2048}, with an all-zero, a dyadic-constant (y = beta exactly) and a non-dyadic constant group
    (variance clamp: finite, inside the bound): the three statistics paths against their derived bounds. Prints the worst |err| of a
    normalised value per path and offset (the table of DESIGN.md)."""
    from stedm_amd import ops
    name, B, H, W, C, groups = sw
    HW = H * W
    for mu in R.OFFSETS:
        x, gamma, beta = R.sweep_inputs(sw, mu)
        d = x.view(B, H, W, C).to(dev)
        g_, b_ = gamma.to(dev), beta.to(dev)
        line = []
        for prec, hilo in (("f16", True), ("bf16", False)):
            dtype, pr = R.dt(prec), _prec(prec, hilo)
            hi = torch.full((B, H, W, C), FILL16, dtype=torch.int16, device=dev)
            lo = torch.full_like(hi, FILL16) if hilo else None
            cs = torch.full((B, ops.gn_chan_nslab(HW), C, 2), NAN, device=dev); ops.gn_chan_stats(d, cs)
            ops.gn_apply16c(d, cs, None, None, hi, lo, pr, g_, b_, 1e-5, groups, 0)
            torch.cuda.synchronize()
            _written(name, hi, lo)
            a1, r1, n1, ok1 = R.sweep_ratio(sw, x, gamma, beta, 1e-5, dtype, hi.cpu().view(B, HW, C), None if lo is None else lo.cpu().view(B, HW, C),
                                            R.chan_stats_k(B, C, HW, 0))
            hi.fill_(FILL16)
            stats = torch.full((B * ops.gn_nslab(C, HW) * groups * 2,), NAN, dtype=torch.float64, device=dev)
            ops.gn_stats(d, None, stats, groups)
            ops.gn_apply16(d, None, hi, lo, pr, g_, b_, 1e-5, groups, 0, stats)
            torch.cuda.synchronize()
            _written(name, hi, lo)
            a2, r2, n2, ok2 = R.sweep_ratio(sw, x, gamma, beta, 1e-5, dtype, hi.cpu().view(B, HW, C), None if lo is None else lo.cpu().view(B, HW, C),
                                            R.gn_stats_k(C, HW))
            assert bool(torch.isfinite(hi.view(dtype).float()).all())
            line.append(f"{prec}{' hi+lo' if hilo else ''}: chan_stats+apply16c err/bound {max(a1, r1):.3f} (random groups {r1:.3f}) |err xhat| {n1:.2e}; "
                        f"gn_stats+apply16 {max(a2, r2):.3f} ({r2:.3f}) {n2:.2e}")
            assert max(a1, r1, a2, r2) < 1.0 and ok1 and ok2
        sc, sh = torch.full((B, C), NAN, device=dev), torch.full((B, C), NAN, device=dev)
        ops.gn_scale_shift(d, None, g_, b_, 1e-5, sc, sh, groups)
        torch.cuda.synchronize()
        x64 = x.double()
        sc64, sh64 = R.scale_shift(x64, None, 0, groups, gamma.double(), beta.double(), 1e-5)
        e_sc, e_sh = R.scale_shift_bound(x64, groups, gamma.double(), beta.double(), 1e-5, True)
        r3 = max(R.ratio((sc.cpu().double() - sc64).abs(), e_sc), R.ratio((sh.cpu().double() - sh64).abs(), e_sh))
        y = x64 * sc.cpu().double().unsqueeze(1) + sh.cpu().double().unsqueeze(1)
        cpg = C // groups
        n3 = float((((y - R.group_norm(x64, None, 0, groups, gamma.double(), beta.double(), 1e-5, 0)).abs()) / gamma.double().abs())[:, :, 3 * cpg:].max())
        print(f"sweep {name} mu/sigma {mu:6.0f}: " + " || ".join(line) + f" || gn_scale_shift err/bound {r3:.3f} |err xhat| {n3:.2e}")
        assert r3 < 1.0


# ================================================================================================ backward
# (precision, planes, acc1, acc2, add, acc_param): all four acc1 / acc2 combinations, dx16 = (hi, lo) / (hi, None) / None, add on / off
BWD_CFG = [("f16", "hilo", False, False, True, False), ("f16", "hi", True, False, False, True), ("bf16", "hilo", False, True, True, True),
           ("bf16", "hi", True, True, False, False), ("bf16", None, False, False, True, False)]
GUARD = 64


def _run_bwd(dev, case, x1, x2, mr, gamma, beta, act, dA, add, old, prec, planes, acc1, acc2, dg0, db0):
    from stedm_amd import ops
    name, B, H, W, c1, c2, groups = case
    HW, C = H * W, c1 + c2
    nhwc = lambda t, c: None if t is None else t.reshape(B, H, W, c).contiguous().to(dev)
    nws = ops.gn_bwd_ws_floats(B, HW, C, groups)
    assert nws == R.gn_bwd_ws_floats(B, HW, C, groups)
    ws = torch.full((nws + GUARD,), NAN, device=dev)
    ws[nws:] = 12345.0
    dx1 = nhwc(old[..., :c1], c1) if acc1 else torch.full((B, H, W, c1), NAN, device=dev)
    dx2 = None
    if c2:
        dx2 = nhwc(old[..., c1:], c2) if acc2 else torch.full((B, H, W, c2), NAN, device=dev)
    hi = torch.full((B, H, W, C), FILL16, dtype=torch.int16, device=dev) if planes else None
    lo = torch.full_like(hi, FILL16) if planes == "hilo" else None
    dg = dg0.to(dev).clone() if dg0 is not None else torch.full((C,), NAN, device=dev)
    db = db0.to(dev).clone() if db0 is not None else torch.full((C,), NAN, device=dev)
    ops.gn_bwd(nhwc(x1, c1), nhwc(x2, c2), mr.to(dev), gamma.to(dev), beta.to(dev), groups, act, nhwc(dA, C), nhwc(add, C), ws, dx1, acc1, dx2, acc2,
               None if not planes else (hi, lo), _prec(prec, planes == "hilo"), dg, db, dg0 is not None)
    torch.cuda.synchronize()
    assert bool((ws[nws:] == 12345.0).all()), f"{name}: words behind the workspace were written"
    _written(name, dx1, dx2, hi, lo, dg, db)
    f = lambda t: None if t is None else t.cpu().view(B, HW, -1)
    return dict(dx1=f(dx1), dx2=f(dx2), hi=f(hi), lo=f(lo), dgamma=dg.cpu(), dbeta=db.cpu())


def _mean_rstd(dev, case, x1, x2, eps, side):
    """{mean, rstd} from gn_fold, or (side) from the forward pass's side output"""
    from stedm_amd import ops
    name, B, H, W, c1, c2, groups = case
    d1 = x1.view(B, H, W, c1).to(dev)
    d2 = x2.view(B, H, W, c2).to(dev) if c2 else None
    ns = ops.gn_chan_nslab(H * W)
    cs1 = torch.full((B, ns, c1, 2), NAN, device=dev); ops.gn_chan_stats(d1, cs1)
    cs2 = None
    if c2:
        cs2 = torch.full((B, ns, c2, 2), NAN, device=dev); ops.gn_chan_stats(d2, cs2)
    mr = torch.full((B, groups, 2), NAN, device=dev)
    if side:
        hi = torch.empty((B, H, W, c1 + c2), dtype=torch.int16, device=dev)
        g = torch.ones(c1 + c2, device=dev)
        ops.gn_apply16c(d1, cs1, d2, cs2, hi, None, _prec("bf16", False), g, g, eps, groups, 0, mean_rstd=mr)
    else:
        ops.gn_fold(cs1, cs2, groups, H * W, eps, mr)
    torch.cuda.synchronize()
    return mr.cpu()


@pytest.mark.parametrize("case", R.BWD, ids=R.BWD_IDS)
def test_backward_exact(dev, case):
    """dA = d_c + e_c s on the exact pattern, act = 0 (refs_gn.exact_bwd): dx, the planes, dgamma and dbeta bit for bit, in every
    configuration of BWD_CFG; {mean, rstd} from gn_fold (pattern A) and from the forward's side output (pattern B)"""
    name, B, H, W, c1, c2, groups = case
    HW, C = H * W, c1 + c2
    for kind in "AB":
        x1, x2, sign, mr_want = R.exact_pattern(B, HW, c1, c2, 0, groups, kind)
        gamma, beta = R.dyadic_affine(C)
        mr = _mean_rstd(dev, case, x1, x2, 0.0, side=kind == "B")
        assert torch.equal(mr, mr_want)
        dA, dx_want, dg_want, db_want = R.exact_bwd(sign, mr, groups, gamma, B, HW, C)
        add_t, old = R.RB.dyadic((B, HW, C), 3), R.RB.dyadic((B, HW, C), 4)
        for prec, planes, acc1, acc2, use_add, accp in BWD_CFG:
            dg0 = torch.arange(C, dtype=torch.float32) / 4.0 if accp else None
            db0 = -torch.arange(C, dtype=torch.float32) / 8.0 if accp else None
            out = _run_bwd(dev, case, x1, x2, mr, gamma, beta, 0, dA, add_t if use_add else None, old, prec, planes, acc1, acc2, dg0, db0)
            want = dx_want + (add_t if use_add else 0.0)
            if acc1:
                want[..., :c1] += old[..., :c1]
            if acc2 and c2:
                want[..., c1:] += old[..., c1:]
            exp = dict(dx1=want[..., :c1].contiguous(), dx2=want[..., c1:].contiguous() if c2 else None,
                       dgamma=dg_want + (dg0 if accp else 0.0), dbeta=db_want + (db0 if accp else 0.0))
            if planes:
                exp["hi"], exp["lo"] = R._split(want, R.dt(prec), planes == "hilo")
            bad = R.exact_mismatches(exp, out, ("dx1", "dx2", "dgamma", "dbeta", "hi", "lo"))
            assert bad == [], f"{name} pattern {kind} {prec} planes {planes} acc {acc1}/{acc2} add {use_add} acc_param {accp}: {bad}"


@pytest.mark.parametrize("case", R.BWD, ids=R.BWD_IDS)
def test_backward_bounds(dev, case):
    name, B, H, W, c1, c2, groups = case
    C = c1 + c2
    x1, x2, gamma, beta, dA, add_t, old = R.bwd_inputs(case)
    mr = _mean_rstd(dev, case, x1, x2, 1e-5, side=False)
    worst = {}
    for prec, planes, acc1, acc2, use_add, accp in BWD_CFG:
        dg0 = R.normal((C,), 6, "dg0") if accp else None
        db0 = R.normal((C,), 6, "db0") if accp else None
        for act in (0, 1):
            out = _run_bwd(dev, case, x1, x2, mr, gamma, beta, act, dA, add_t if use_add else None, old, prec, planes, acc1, acc2, dg0, db0)
            r = R.bwd_ratios(case, x1, x2, mr, gamma, beta, act, dA, add_t if use_add else None, old[..., :c1] if acc1 else None,
                             old[..., c1:] if (acc2 and c2) else None, R.dt(prec), planes, dg0, db0, out)
            for k, v in r.items():
                worst[k] = max(worst.get(k, 0.0), v)
            assert max(r.values()) < 1.0, (prec, planes, acc1, acc2, use_add, accp, act, r)
    print(f"gn_bwd {name} (cb, ppt) {R.gn_bwd_fused_cb(c1, c2, groups, H * W)}: worst err/bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ================================================================================================ argument checks
def test_argument_checks(dev):
    """every STEDM_CHECK_ARG of the GroupNorm entries a Python caller can trip, once, each tied to its own message (match=): the error is
    raised and no output word is written. Where the ops wrapper cannot express the arguments (a slot count of 0 beside a valid pointer -
    an empty tensor's data_ptr() is null and would trip the null-pointer check instead -, raw_lo without raw_hi, C > 4096 without such a
    tensor) the entry is called itself. Every buffer has the size the arguments state."""
    import re
    from stedm_amd import ops
    from stedm_amd._lib import StedmHipError
    B, H, W = 2, 4, 4
    HW = H * W
    f = lambda *s: torch.zeros(s, device=dev)
    i16 = lambda *s: torch.full(s, FILL16, dtype=torch.int16, device=dev)
    pr = _prec("f16", False)
    lib, p = ops.lib(), lambda t: t.data_ptr()
    outs = []

    def trip(msg, fn, *out):
        with pytest.raises(StedmHipError, match=re.escape(msg)):
            fn()
        outs.extend(out)

    def apply16c(x1, c1, cs1, ns1, x2, c2, cs2, ns2, g, groups, hi, lo=None, rhi=None, rlo=None, b=B, hw=HW, dtype=pr.mm_dtype):
        ops.check(lib.stedm_gn_apply16c(p(x1), c1, p(cs1), ns1, None if x2 is None else p(x2), c2, None if cs2 is None else p(cs2), ns2, 0, p(g), p(g), 1e-5,
                                        groups, 0, b, hw, p(hi), None if lo is None else p(lo), None if rhi is None else p(rhi),
                                        None if rlo is None else p(rlo), dtype, None), "stedm_gn_apply16c")

    def x16(c1, cs1, ns1, x2, c2, cs2, ns2, g, groups, hi, raw, b=B, hw=HW):
        ops.check(lib.stedm_gn_apply16c_x16(c1, p(cs1), ns1, None if x2 is None else p(x2), c2, None if cs2 is None else p(cs2), ns2, 0, p(g), p(g), 1e-5,
                                            groups, 0, b, hw, p(hi), p(raw), pr.mm_dtype, None), "stedm_gn_apply16c_x16")
    x40, cs40, g40 = f(B, H, W, 40), f(B, 1, 40, 2), f(40)
    x64, cs64, g64 = f(B, H, W, 64), f(B, 1, 64, 2), f(64)
    x24, cs24 = f(B, H, W, 24), f(B, 1, 24, 2)
    x6, cs6, g6, hi6 = f(B, H, W, 6), f(B, 1, 6, 2), f(6), i16(B, H, W, 6)
    big, csb, gb, hib = f(B, 1, 1, 128), f(B, 1, 128, 2), f(128), i16(B, 1, 1, 128)
    hi40, hi64, lo64, raw64 = i16(B, H, W, 40), i16(B, H, W, 64), i16(B, H, W, 64), i16(B, H, W, 64)
    # ---- stedm_gn_apply16c
    grp = "gn_apply16c: need groups <= 64 and C % groups == 0"
    trip(grp, lambda: ops.gn_apply16c(x40, cs40, None, None, hi40, None, pr, g40, g40, 1e-5, 32), hi40)                 # C % groups
    trip(grp, lambda: ops.gn_apply16c(big, csb, None, None, hib, None, pr, gb, gb, 1e-5, 128), hib)                     # groups > 64
    trip("gn_apply16c: channels must be multiples of 4", lambda: ops.gn_apply16c(x6, cs6, None, None, hi6, None, pr, g6, g6, 1e-5, 3), hi6)
    wide, csw, gw, hiw = f(1, 1, 1, 4100), f(1, 1, 4100, 2), f(4100), i16(1, 1, 1, 4100)                                # C = 4100 > 4096
    trip("gn_apply16c: channels must be multiples of 4, C <= 4096", lambda: apply16c(wide, 4100, csw, 1, None, 0, None, 0, gw, 4, hiw, b=1, hw=1), hiw)
    trip("gn_apply16c: raw_lo without raw_hi", lambda: apply16c(x64, 64, cs64, 1, None, 0, None, 0, g64, 32, hi64, rlo=lo64), hi64, lo64)
    slots = "gn_apply16c: nslab1 / nslab2 must be the slot counts"
    trip(slots, lambda: apply16c(x64, 64, cs64, 0, None, 0, None, 0, g64, 32, hi64), hi64)                              # nslab1 == 0, cs1 valid
    trip(slots, lambda: apply16c(x40, 40, cs40, 1, x24, 24, cs24, 0, g64, 32, hi64), hi64)                              # nslab2 == 0 with x2, cs2 valid
    trip("gn_apply16c: x2/c2/cs2 mismatch", lambda: apply16c(x40, 40, cs40, 1, x24, 24, None, 1, g64, 32, hi64), hi64)  # x2 without cs2
    trip("gn_apply16c: bad mm_dtype", lambda: apply16c(x64, 64, cs64, 1, None, 0, None, 0, g64, 32, hi64, dtype=77), hi64)
    # ---- stedm_gn_apply16c_x16
    trip("gn_apply16c_x16: need c1, c1 + c2 multiples of 8", lambda: ops.gn_apply16c_x16(36, f(B, 1, 36, 2), f(B, H, W, 28), f(B, 1, 28, 2), hi64, raw64, pr,
                                                                                         g64, g64, 1e-5, 32), hi64, raw64)           # c1 % 8
    w16, cs16, g16, hi16, raw16 = f(1, 1, 1, 4104), f(1, 1, 4104, 2), f(4104), i16(1, 1, 1, 4104), i16(1, 1, 1, 4104)            # 3 C floats > 48 KiB
    trip("gn_apply16c_x16: need c1, c1 + c2 multiples of 8, C <= 4096", lambda: x16(4104, cs16, 1, None, 0, None, 0, g16, 8, hi16, raw16, b=1, hw=1), hi16, raw16)
    raw40 = i16(B, H, W, 40)
    trip("gn_apply16c_x16: need groups <= 64 and C % groups == 0", lambda: ops.gn_apply16c_x16(40, cs40, None, None, hi40, raw40, pr, g40, g40, 1e-5, 32),
         hi40, raw40)
    trip("gn_apply16c_x16: need groups <= 64 and C % groups == 0", lambda: x16(128, csb, 1, None, 0, None, 0, gb, 128, hib, i16(B, 1, 1, 128), hw=1), hib)
    xslots = "gn_apply16c_x16: nslab1 / nslab2 must be the slot counts"
    trip(xslots, lambda: x16(64, cs64, 0, None, 0, None, 0, g64, 32, hi64, raw64), hi64, raw64)                          # nslab1 == 0, cs1 valid
    trip(xslots, lambda: x16(40, cs40, 1, x24, 24, cs24, 0, g64, 32, hi64, raw64), hi64, raw64)                          # nslab2 == 0 with x2
    trip("gn_apply16c_x16: x2/c2/cs2 mismatch", lambda: x16(40, cs40, 1, x24, 24, None, 1, g64, 32, hi64, raw64), hi64, raw64)
    # ---- gn_chan_stats, gn_fold
    csn = torch.full((B, 1, 6, 2), NAN, device=dev)
    trip("gn_chan_stats: bad args", lambda: ops.gn_chan_stats(x6, csn))                                                  # C % 4
    trip("gn_chan_stats16: bad args", lambda: ops.gn_chan_stats16(x6, csn, hi6, None, pr), hi6)
    assert bool(torch.isnan(csn).all())
    mr, mr128 = torch.full((B, 32, 2), NAN, device=dev), torch.full((B, 128, 2), NAN, device=dev)
    trip("gn_fold: bad args", lambda: ops.gn_fold(cs40, None, 32, HW, 1e-5, mr))                                         # C % groups
    trip("gn_fold: bad args", lambda: ops.gn_fold(csb, None, 128, 1, 1e-5, mr128))                                       # groups > 64
    assert bool(torch.isnan(mr).all()) and bool(torch.isnan(mr128).all())
    # ---- gn_stats, gn_apply16, gn_scale_shift
    st = torch.full((B * 128 * 2,), NAN, dtype=torch.float64, device=dev)
    trip("gn_stats: need groups <= 64", lambda: ops.gn_stats(x40, None, st, 32))                                         # C % groups
    trip("gn_stats: need groups <= 64", lambda: ops.gn_stats(big, None, st, 128))                                        # groups > 64
    trip("gn_apply16: C % groups != 0", lambda: ops.gn_apply16(x40, None, hi40, None, pr, g40, g40, 1e-5, 32, 0, st), hi40)
    trip("gn_apply16: channels must be multiples of 4", lambda: ops.gn_apply16(x6, None, hi6, None, pr), hi6)
    trip("gn_apply16: gamma needs beta, stats, groups", lambda: ops.gn_apply16(x64, None, hi64, None, pr, g64, None, 1e-5, 32, 0, st), hi64)     # no beta
    trip("gn_apply16: gamma needs beta, stats, groups", lambda: ops.gn_apply16(x64, None, hi64, None, pr, g64, g64, 1e-5, 32, 0, None), hi64)    # no stats
    trip("gn_apply16: groups <= 64", lambda: ops.gn_apply16(big, None, hib, None, pr, gb, gb, 1e-5, 128, 0, st), hib)
    assert bool(torch.isnan(st).all())
    sc, sh = torch.full((B, 40), NAN, device=dev), torch.full((B, 40), NAN, device=dev)
    trip("not divisible by groups", lambda: ops.gn_scale_shift(x40, None, g40, g40, 1e-5, sc, sh, 32))
    assert bool(torch.isnan(sc).all()) and bool(torch.isnan(sh).all())
    # ---- gn_bwd
    dx, dg, db = torch.full((B, H, W, 40), NAN, device=dev), torch.full((40,), NAN, device=dev), torch.full((40,), NAN, device=dev)
    ws = torch.full((ops.gn_bwd_ws_floats(B, HW, 40, 32) + 8,), NAN, device=dev)
    trip("gn_bwd: channel constraints", lambda: ops.gn_bwd(x40, None, f(B, 32, 2), g40, g40, 32, 0, x40, None, ws, dx, False, None, False, None, pr, dg, db, False))
    dxb, dgb, wsb = torch.full((B, 1, 1, 128), NAN, device=dev), torch.full((128,), NAN, device=dev), torch.full((2048,), NAN, device=dev)
    trip("gn_bwd: channel constraints", lambda: ops.gn_bwd(big, None, f(B, 128, 2), gb, gb, 128, 0, big, None, wsb, dxb, False, None, False, None, pr, dgb,
                                                           dgb.clone(), False))                                          # groups > 64
    trip("gn_bwd: x2/c2/dx2 mismatch", lambda: ops.gn_bwd(x40, x24, f(B, 32, 2), g64, g64, 32, 0, x64, None, f(4096), dx, False, None, False, None, pr,
                                                          f(64), f(64), False))                                          # x2 without dx2
    torch.cuda.synchronize()
    for t in (dx, dg, db, ws, dxb, dgb, wsb):
        assert bool(torch.isnan(t).all())
    for o in outs:
        assert bool((o == FILL16).all()), "an entry that refused its arguments wrote to an output"
