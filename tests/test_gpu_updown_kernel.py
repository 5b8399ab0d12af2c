"""GPU tier (-m gpu): stedm_gn_apply16c_resample (stedm_amd/csrc/resample.hip), the front of ResBlock(up / down), against its siblings bit for
bit and against tests/refs_updown.py. Both modes, f16 and bf16, hi-only and hi + lo planes, sentinels around every buffer; every output is
filled first (NaN / 0x5a5a) and must be written everywhere.

Exact checks, no tolerance:
  (a) xr equals ops.avgpool2x2 / ops.replicate2x2 (scale 1) of the same x;
  (b) nearest: the four copies of the planes equal the planes ops.gn_apply16c writes for the same x, cs, gamma, beta;
  (c) pool of a cell-constant input (a low-resolution tensor replicated 2 x 2): the planes equal ops.gn_apply16c's planes of that input at
      [:, ::2, ::2] - four equal terms and a quarter are exact;
  (d) pool, act = 0, the exact tier of refs_gn (x = m_g +- a_g, dyadic gamma / beta, eps = 0): torch.equal with the restatement, lo == 0;
  (e) mean_rstd equals the side output of ops.gn_apply16c (stedm_gn_apply16c_mr).
With SiLU on general inputs, pool mode: per-element err / bound < 1 against the fp64 restatement on fold() of the kernel's own partials, the
bound derived in refs_updown's docstring (tests/test_updown_refs_cpu.py holds the fp32 restatement to the same bound). Printed per case.
The fp16 guard: an activation beyond the f16 range sets bit NORM through this kernel, in either mode; the same input in bf16 sets nothing.
Shapes: refs_updown.POOL_CASES / NEAREST_CASES (the smallest that reach each edge; see there)."""
import pytest
import torch

from tests import refs_gn as G
from tests import refs_guard as RG
from tests import refs_updown as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

PAD = 64                # sentinel elements on either side of a buffer (>= 128 B: the payload stays 16-byte aligned)
SENT, SENT16, FILL16 = 12345.0, 0x7e7e, 0x5a5a
NAN = float("nan")
FORMS = [pytest.param(p, h, id=f"{p}-{'hilo' if h else 'hi'}") for p in ("f16", "bf16") for h in (False, True)]


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


def guarded(dev, shape, dtype=torch.float32):
    n = 1
    for s in shape:
        n *= s
    i16 = dtype == torch.int16
    flat = torch.full((n + 2 * PAD,), SENT16 if i16 else SENT, dtype=dtype, device=dev)
    v = flat[PAD:PAD + n].view(shape)
    v.fill_(FILL16 if i16 else NAN)
    return flat, v


def sentinels_ok(flat):
    s = SENT16 if flat.dtype == torch.int16 else SENT
    return bool((flat[:PAD] == s).all()) and bool((flat[-PAD:] == s).all())


def written(*ts):
    for t in ts:
        if t is not None:
            assert not bool((t == FILL16).any() if t.dtype == torch.int16 else torch.isnan(t).any()), "elements left unwritten"


def new_shape(shape, mode):
    B, H, W, C = shape
    return (B, H // 2, W // 2, C) if mode == R.POOL else (B, 2 * H, 2 * W, C)


def run(dev, x, gamma, beta, groups, eps, act, mode, prec, hilo, want_xr=True, want_mr=True):
    """the partials of x from stedm_gn_chan_stats, then the pass with every output in a guarded buffer: dict of device tensors"""
    from stedm_amd import ops
    B, H, W, C = x.shape
    d = x.to(dev)
    cs = torch.full((B, ops.gn_chan_nslab(H * W), C, 2), NAN, device=dev)
    ops.gn_chan_stats(d, cs)
    ns = new_shape(x.shape, mode)
    bufs = dict(hi=guarded(dev, ns, torch.int16), lo=guarded(dev, ns, torch.int16) if hilo else None,
                xr=guarded(dev, ns) if want_xr else None, mr=guarded(dev, (B, groups, 2)) if want_mr else None)
    get = lambda k: None if bufs[k] is None else bufs[k][1]
    ops.gn_apply16c_resample(d, cs, get("hi"), get("lo"), _prec(prec, hilo), gamma.to(dev), beta.to(dev), mode, eps, groups, act,
                             xr=get("xr"), mean_rstd=get("mr"))
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert b is None or sentinels_ok(b[0]), f"{k}: a sentinel was overwritten"
    out = {k: get(k) for k in bufs}
    written(*out.values())
    out.update(x=d, cs=cs)
    return out


def apply16c(dev, o, gamma, beta, groups, eps, act, prec, hilo):
    """(hi, lo, mean_rstd) of ops.gn_apply16c for the x and cs of a run"""
    from stedm_amd import ops
    B, H, W, C = o["x"].shape
    hi = torch.full((B, H, W, C), FILL16, dtype=torch.int16, device=dev)
    lo = torch.full_like(hi, FILL16) if hilo else None
    mr = torch.full((B, groups, 2), NAN, device=dev)
    ops.gn_apply16c(o["x"], o["cs"], None, None, hi, lo, _prec(prec, hilo), gamma.to(dev), beta.to(dev), eps, groups, act, mean_rstd=mr)
    torch.cuda.synchronize()
    return hi, lo, mr


def rep(t):
    return t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


@pytest.mark.parametrize("prec,hilo", FORMS)
@pytest.mark.parametrize("case", R.NEAREST_CASES, ids=R.case_id)
def test_nearest_is_the_apply_pass_four_times_and_replicate2x2(dev, case, prec, hilo):
    from stedm_amd import ops
    B, H, W, C, groups = case
    x, gamma, beta = R.inputs(case)
    for act in (1, 0):
        o = run(dev, x, gamma, beta, groups, 1e-5, act, R.NEAREST, prec, hilo)
        hi, lo, mr = apply16c(dev, o, gamma, beta, groups, 1e-5, act, prec, hilo)
        assert torch.equal(o["hi"], rep(hi)), "(b) hi plane"
        if hilo:
            assert torch.equal(o["lo"], rep(lo)), "(b) lo plane"
        assert torch.equal(o["mr"], mr), "(e) mean_rstd"
        want = torch.empty((B, 2 * H, 2 * W, C), device=dev)
        ops.replicate2x2(o["x"], want)
        assert torch.equal(o["xr"], want), "(a) xr"
    # xr and mean_rstd are optional: the planes do not depend on them
    o2 = run(dev, x, gamma, beta, groups, 1e-5, 0, R.NEAREST, prec, hilo, want_xr=False, want_mr=False)
    assert torch.equal(o2["hi"], o["hi"]) and (not hilo or torch.equal(o2["lo"], o["lo"]))


@pytest.mark.parametrize("prec,hilo", FORMS)
@pytest.mark.parametrize("case", R.POOL_CASES, ids=R.case_id)
def test_pool_xr_statistics_and_bound(dev, case, prec, hilo):
    from stedm_amd import ops
    B, H, W, C, groups = case
    dtype = G.dt(prec)
    x, gamma, beta = R.inputs(case)
    eps = 1e-5
    o = run(dev, x, gamma, beta, groups, eps, 1, R.POOL, prec, hilo)
    want = torch.empty((B, H // 2, W // 2, C), device=dev)
    ops.avgpool2x2(o["x"], want)
    assert torch.equal(o["xr"], want), "(a) xr"
    _, _, mr = apply16c(dev, o, gamma, beta, groups, eps, 1, prec, hilo)
    assert torch.equal(o["mr"], mr), "(e) mean_rstd"
    # SiLU on general inputs: per-element bound, statistics = fold() of the partials the kernel read
    mr_own = G.fold(o["cs"].cpu(), None, 0, groups, H * W, eps)
    ref, bound = R.pool_bound(x.double(), mr_own, groups, gamma.double(), beta.double(), 1, dtype, hilo)
    got = G.planes_value(o["hi"].cpu(), o["lo"].cpu() if hilo else None, dtype)
    r = G.ratio((got - ref).abs(), bound)
    print(f"[pool {R.case_id(case)} {prec} {'hi + lo' if hilo else 'hi'}] worst err / bound {r:.3f}")
    assert r < 1.0
    # two calls give the same bits; without the optional outputs the planes are the same
    o2 = run(dev, x, gamma, beta, groups, eps, 1, R.POOL, prec, hilo, want_xr=False, want_mr=False)
    assert torch.equal(o2["hi"], o["hi"]) and (not hilo or torch.equal(o2["lo"], o["lo"]))


@pytest.mark.parametrize("prec,hilo", FORMS)
@pytest.mark.parametrize("case", R.POOL_CASES, ids=R.case_id)
def test_pool_of_a_cell_constant_input_is_the_apply_pass_at_every_other_pixel(dev, case, prec, hilo):
    B, H, W, C, groups = case
    xl, gamma, beta = R.inputs((B, H // 2, W // 2, C, groups), seed=1)
    x = rep(xl).contiguous()
    for act in (1, 0):
        o = run(dev, x, gamma, beta, groups, 1e-5, act, R.POOL, prec, hilo)
        hi, lo, _ = apply16c(dev, o, gamma, beta, groups, 1e-5, act, prec, hilo)
        assert torch.equal(o["hi"], hi[:, ::2, ::2]), "(c) hi plane"
        if hilo:
            assert torch.equal(o["lo"], lo[:, ::2, ::2]), "(c) lo plane"
        assert torch.equal(o["xr"].cpu(), xl), "a mean of four equal values is the value"


@pytest.mark.parametrize("prec,hilo", FORMS)
@pytest.mark.parametrize("case", R.POOL_CASES, ids=R.case_id)
def test_pool_exact_tier(dev, case, prec, hilo):
    dtype = G.dt(prec)
    for kind in "AB":
        p = R.exact_problem(case, kind, dtype)
        o = run(dev, p["x"], p["gamma"], p["beta"], case[4], 0.0, 0, R.POOL, prec, hilo)
        assert torch.equal(o["cs"].cpu(), p["cs"]), f"{kind}: partials"
        assert torch.equal(o["mr"].cpu(), p["mr"]), f"{kind}: mean_rstd"
        assert torch.equal(o["hi"].cpu(), p["hi"]), f"{kind}: (d) hi plane"
        if hilo:
            assert not bool(o["lo"].any()), f"{kind}: lo must be zero"
        assert torch.equal(o["xr"].cpu(), p["xr"]), f"{kind}: xr"


@pytest.mark.parametrize("mode", [R.POOL, R.NEAREST], ids=["pool", "nearest"])
def test_f16_guard_through_this_kernel(dev, mode):
    """gamma[c] = 0, beta[c] = 7e4 with SiLU: the activation of channel c is 7e4 > 65504 at every pixel (and so is its pool): bit NORM in f16,
    an inf in the plane; the same input in bf16 sets nothing. Then a finite run leaves the word at 0."""
    from stedm_amd import ops
    w = ops.f16_guard_enable()
    case = (2, 4, 4, 32, 8)
    x, gamma, beta = R.inputs(case)
    c = 13
    try:
        for prec, g_c, b_c, bits in (("f16", 0.0, 7.0e4, RG.NORM), ("bf16", 0.0, 7.0e4, 0), ("f16", float(gamma[c]), float(beta[c]), 0)):
            gm, bt = gamma.clone(), beta.clone()
            gm[c], bt[c] = g_c, b_c
            torch.cuda.synchronize()
            w.zero_()
            o = run(dev, x, gm, bt, case[4], 1e-5, 1, mode, prec, False)
            got = w.cpu().tolist()
            assert got[0] == bits and got[1:] == [0, 0, 0], f"{prec} beta {b_c}: flag words {got}, expected {bits:#x}"
            plane = o["hi"].view(G.dt(prec)).float()
            if b_c == 7.0e4:
                assert bool(torch.isinf(plane[..., c]).all()) == (prec == "f16")
                assert bool(torch.isfinite(plane[..., :c]).all()) and bool(torch.isfinite(plane[..., c + 1:]).all())
            else:
                assert bool(torch.isfinite(plane).all())
    finally:
        torch.cuda.synchronize()
        w.zero_()


def test_argument_errors_raise_before_any_launch(dev):
    from stedm_amd import ops
    from stedm_amd._lib import StedmHipError
    pr = _prec("bf16", False)

    def f(*s):
        return torch.full(s, SENT, device=dev)

    def call(H, W, C, mode, groups=2, refused=True):
        ns = new_shape((1, H, W, C), mode)
        hi = torch.full(ns, SENT16, dtype=torch.int16, device=dev)
        xr = f(*ns)
        try:
            ops.gn_apply16c_resample(f(1, H, W, C), f(1, 1, C, 2), hi, None, pr, f(C), f(C), mode, 1e-5, groups, 1, xr=xr)
        finally:
            torch.cuda.synchronize()
            if refused:
                assert bool((xr == SENT).all()) and bool((hi == SENT16).all()), "a refused call writes nothing"
            else:
                assert not bool((hi == SENT16).any()), "an accepted call writes every plane word"
    for H, W in ((5, 4), (4, 7)):
        with pytest.raises(StedmHipError, match="even"):
            call(H, W, 8, R.POOL)
    for mode in (R.POOL, R.NEAREST):
        with pytest.raises(StedmHipError, match="C %"):
            call(4, 4, 12, mode)
    with pytest.raises(StedmHipError, match="groups"):
        call(4, 4, 16, R.NEAREST, groups=3)
    with pytest.raises(AssertionError):
        call(4, 4, 8, 3)
    call(3, 5, 8, R.NEAREST, refused=False)      # odd sides are fine for the nearest x2
