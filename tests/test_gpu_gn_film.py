"""GPU tier (-m gpu): stedm_gn_apply16c_film and stedm_gn_bwd_film against tests/refs_gn_film.py, in the two tiers of
tests/test_gpu_gn_exact.py: exact (inputs whose every output is known bit for bit: torch.equal) and bound (normal data, per-element
err / bound < 1 with the bounds derived in the refs docstring; every case prints its worst ratio). The kernel form each case reaches is
asserted in tests/test_gn_film_refs_cpu.py. Every output buffer starts as NaN / FILL16 and must be fully written."""
import pytest
import torch

from tests import refs_gn as RG
from tests import refs_gn_film as RF

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

FILL16 = RF.FILL16
DTYPES = [pytest.param("f16", torch.float16, id="f16"), pytest.param("bf16", torch.bfloat16, id="bf16")]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stedm_amd import _lib
    _lib.lib()  # must load: no fallback
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _clean_guard_word(dev):
    """the fp16 guard's flag word is process-wide state: zero before and after every test of this file"""
    from stedm_amd import ops
    w = ops.f16_guard_enable()
    w.zero_()
    yield
    torch.cuda.synchronize()
    w.zero_()


def _prec(mode, hilo):
    from stedm_amd.ops import Precision
    return Precision.parse(("parity" if mode == "f16" else "parity_bf16") if hilo else mode)


def _run_fwd(dev, case, prob, mode):
    """launch the forward entry on the problem; returns (hi, lo, mr) on the CPU"""
    from stedm_amd import ops
    name, B, H, W, C, groups, hilo, chan, lay = case
    prec = _prec(mode, hilo)
    assert prec.npass == (3 if hilo else 1)
    x = prob["x"].view(B, H, W, C).to(dev)
    hi = torch.full((B, H, W, C), FILL16, dtype=torch.int16, device=dev)
    lo = torch.full((B, H, W, C), FILL16, dtype=torch.int16, device=dev) if hilo else None
    mr = torch.full((B, groups, 2), float("nan"), device=dev)
    ops.gn_apply16c_film(x, prob["cs"].to(dev), hi, lo, prec, prob["gamma"].to(dev), prob["beta"].to(dev), prob["film"].to(dev), prob["off"],
                         prob["bstride"], prob["eps"], groups, prob["act"], mean_rstd=mr)
    torch.cuda.synchronize()
    return hi.cpu().view(B, H * W, C), None if lo is None else lo.cpu().view(B, H * W, C), mr.cpu()


@pytest.mark.parametrize("mode,dtype", DTYPES)
@pytest.mark.parametrize("case", RF.FWD, ids=RF.FWD_IDS)
def test_film_apply_exact(dev, case, mode, dtype):
    prob = RF.fwd_problem(case, True, dtype, 0, 0.0)
    hi, lo, mr = _run_fwd(dev, case, prob, mode)
    assert torch.equal(mr, prob["mr"]), "mean_rstd"
    bad = (hi != prob["hi"]).nonzero()
    assert len(bad) == 0, f"{len(bad)} plane words differ, first at {bad[0].tolist()}"
    if lo is not None:
        assert torch.equal(lo, torch.zeros_like(lo)), "lo plane of exactly representable values must be 0"


@pytest.mark.parametrize("mode,dtype", DTYPES)
@pytest.mark.parametrize("act,eps", [(0, 1e-5), (1, 1e-6)])
@pytest.mark.parametrize("case", RF.FWD, ids=RF.FWD_IDS)
def test_film_apply_within_the_bound(dev, case, act, eps, mode, dtype):
    prob = RF.fwd_problem(case, False, dtype, act, eps)
    hi, lo, mr = _run_fwd(dev, case, prob, mode)
    assert not bool((hi == FILL16).all(-1).any()), "a pixel of the plane was not written"
    r = RF.ratio(RG.planes_value(hi, lo, dtype) - prob["ref"], prob["bound"])
    # the side output: one fp32 rounding of the fp64 fold of the partials the kernel read
    r_mr = RF.ratio(mr.double() - prob["mr64"], 2.0 * RF.U * prob["mr64"].abs() + RF.TINY)
    print(f"[{case[0]} act={act} eps={eps} {mode}] worst err / bound: planes {r:.3f}  mean_rstd {r_mr:.3f}")
    assert r < 1.0 and r_mr < 1.0


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("mode,dtype", DTYPES)
@pytest.mark.parametrize("case", RF.BWD, ids=RF.BWD_IDS)
def test_film_backward_within_the_bounds(dev, case, mode, dtype):
    from stedm_amd import ops
    name, B, H, W, C, groups, form, act, use_add, acc, acc_param, planes = case
    prob = RF.bwd_problem(case, dtype)
    prec = _prec(mode, planes == "hilo")
    sh4 = (B, H, W, C)
    g = lambda t: None if t is None else t.to(dev)
    dx = prob["old"].view(sh4).to(dev).clone() if acc else torch.full(sh4, float("nan"), device=dev)
    hi = torch.full(sh4, FILL16, dtype=torch.int16, device=dev) if planes else None
    lo = torch.full(sh4, FILL16, dtype=torch.int16, device=dev) if planes == "hilo" else None
    dg = prob["dg0"].to(dev).clone() if acc_param else torch.full((C,), float("nan"), device=dev)
    db = prob["db0"].to(dev).clone() if acc_param else torch.full((C,), float("nan"), device=dev)
    dE = prob["dE0"].to(dev).clone()
    ws = torch.full((ops.gn_bwd_ws_floats(B, H * W, C, groups),), float("nan"), device=dev)
    ops.gn_bwd_film(prob["x"].view(sh4).to(dev), prob["mr32"].to(dev), prob["gamma"].to(dev), prob["beta"].to(dev), groups, act,
                    prob["film"].to(dev), prob["off"], prob["bstride"], prob["dA"].view(sh4).to(dev), g(None if prob["add"] is None else prob["add"].view(sh4)),
                    ws, dx, acc, None if hi is None else (hi, lo), prec, dg, db, acc_param, dE, prob["d_off"])
    torch.cuda.synchronize()
    flat = lambda t: None if t is None else t.cpu().view(B, H * W, C)
    out = dict(dx=flat(dx), hi=flat(hi), lo=flat(lo), dgamma=dg.cpu(), dbeta=db.cpu(), dE=dE.cpu())
    r = RF.bwd_ratios(case, prob, out, dtype)
    print(f"[{name} {mode}] worst err / bound", {k: round(v, 3) for k, v in r.items()})
    assert max(r.values()) < 1.0, r


def test_film_backward_is_bitwise_reproducible(dev):
    from stedm_amd import ops
    case = RF.BWD[1]
    name, B, H, W, C, groups, form, act, use_add, acc, acc_param, planes = case
    prob = RF.bwd_problem(case, torch.bfloat16)
    sh4 = (B, H, W, C)
    outs = []
    for _ in range(2):
        dx = torch.full(sh4, float("nan"), device=dev)
        dg, db = torch.full((C,), float("nan"), device=dev), torch.full((C,), float("nan"), device=dev)
        dE = prob["dE0"].to(dev).clone()
        ws = torch.empty((ops.gn_bwd_ws_floats(B, H * W, C, groups),), device=dev)
        ops.gn_bwd_film(prob["x"].view(sh4).to(dev), prob["mr32"].to(dev), prob["gamma"].to(dev), prob["beta"].to(dev), groups, act,
                        prob["film"].to(dev), prob["off"], prob["bstride"], prob["dA"].view(sh4).to(dev), None, ws, dx, False, None,
                        _prec("bf16", False), dg, db, False, dE, prob["d_off"])
        outs.append([t.cpu() for t in (dx, dg, db, dE)])
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ------------------------------------------------------------------------------------------------ fp16 range guard, argument errors
@pytest.mark.parametrize("big", [True, False], ids=["scale_pushes_over", "scale_zero"])
def test_film_scale_alone_sets_the_norm_guard_bit(dev, big):
    """gamma = 1, beta = 0 and raw values of a few units: sqrt(n) |gamma| + |beta| is far inside the fp16 range, so the plain switch stays
    off; 1 + scale = 2^17 on one (sample, channel) takes its +-1 to +-131072 > 65504. The switch must look at the effective affine."""
    from stedm_amd import ops
    case = RF.FWD[1]
    name, B, H, W, C, groups, hilo, chan, lay = case
    prob = RF.fwd_problem(case, True, torch.float16, 0, 0.0)
    prob["gamma"], prob["beta"] = torch.ones(C), torch.zeros(C)
    film = torch.zeros_like(prob["film"])
    if big:
        film[1, prob["off"] + 5] = 131071.0
    prob["film"] = film
    w = ops.f16_guard_enable()
    hi, lo, mr = _run_fwd(dev, case, prob, "f16")
    word = w.cpu().tolist()
    v = hi.view(torch.float16)
    if big:
        assert word[0] == 2, f"flag word {word[0]:#x}, expected STEDM_F16G_NORM"
        assert bool(torch.isinf(v[1, :, 5]).all()) and int(torch.isinf(v).sum()) == H * W
    else:
        assert word[0] == 0, f"flag word {word[0]:#x}, expected 0"
        assert bool((v.abs() == 1.0).all())
    assert word[1:] == [0, 0, 0]


def test_film_argument_errors(dev):
    from stedm_amd import _lib, ops
    L = _lib.lib()
    B, H, W, C, groups = 2, 4, 4, 32, 8
    x = torch.zeros((B, H, W, C), device=dev)
    cs = torch.zeros((B, 1, C, 2), device=dev)
    hi = torch.zeros((B, H, W, C), dtype=torch.int16, device=dev)
    gm, bt = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    film = torch.zeros((B, 2 * C), device=dev)

    def call(x2=None, c2=0, cs2=None, film_ptr=film.data_ptr(), c=C):
        return L.stedm_gn_apply16c_film(x.data_ptr(), c, cs.data_ptr(), 1, x2, c2, cs2, 1 if x2 else 0, 0, gm.data_ptr(), bt.data_ptr(), 1e-5, groups, 1,
                                        B, H * W, hi.data_ptr(), None, None, None, None, film_ptr, 2 * C, 0, _lib.BF16, None)
    assert call() == 0
    assert call(x2=x.data_ptr(), c2=8, cs2=cs.data_ptr()) != 0, "x2 != NULL must be an argument error"
    assert call(film_ptr=None) != 0, "a null film must be an argument error"
    assert call(c=36) != 0, "C % 8 != 0 must be an argument error"
    with pytest.raises(_lib.StedmHipError):
        x36 = torch.zeros((B, H, W, 36), device=dev)
        ops.gn_apply16c_film(x36, torch.zeros((B, 1, 36, 2), device=dev), torch.zeros((B, H, W, 36), dtype=torch.int16, device=dev), None,
                             _prec("bf16", False), torch.ones(36, device=dev), torch.zeros(36, device=dev), torch.zeros((B, 72), device=dev), 0, 72,
                             1e-5, 4, 1)
    torch.cuda.synchronize()
