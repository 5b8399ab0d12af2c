"""GPU tier (-m gpu): the dropout forms of the GroupNorm pass and of its backward - stedm_gn_apply16c_drop / _film_drop and
stedm_gn_bwd_drop / _film_drop - against the mask stream of tests/refs_dropout.py.

Forward. p = 1/2 makes inv_keep exactly 2, so the drop pass's planes are where(keep, 2 * the plain entry's planes, 0) bit for bit
(elements whose doubled word would leave the 16-bit normal range are skipped); p = 0.1: +0 exactly where the mask drops, kept elements
within refs_dropout.drop_apply_bound of the fp64 reference. Shapes: one channel per group (the TINY net's width), a block with a
partial iteration only, one full iteration plus a partial one, hi + lo planes, and the channel-run launch (asserted from
refs_gn.apply16c_geometry).
Backward. stedm_gn_bwd_drop(dA) equals stedm_gn_bwd(dA_eff) bit for bit, dA_eff = keep ? dA * inv_keep : 0 formed by torch as one fp32
multiply; and it stays within the plain backward's bounds of the fp64 closed form on dA_eff. One shape per kernel selection (one-pass,
three-kernel chain). Every output buffer starts as NaN / FILL16 and must be fully written.
Argument errors of the backward FiLM and dropout entries (gn_bwd.hip: one shared check under the entry's name), and p = 0 forwarding to the
plain / FiLM entries bit for bit: test_backward_argument_errors."""
import numpy as np
import pytest
import torch

from tests import refs_dropout as RD
from tests import refs_gn as RG
from tests import refs_gn_film as RF

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

FILL16 = RG.FILL16
DTYPES = [pytest.param("f16", torch.float16, id="f16"), pytest.param("bf16", torch.bfloat16, id="bf16")]
SEED, K, STEP = 0x1234ABCD5678, 5, 7
EPS = 1e-5

# (id, B, H, W, C, groups, hilo)
FWD = [
    ("cpg1_tiny", 2, 16, 16, 32, 32, False),        # pixel runs, one channel per group
    ("tail_only", 3, 5, 5, 96, 8, False),           # 24 quads per block: a partial block iteration and nothing else
    ("full_tail", 3, 32, 32, 640, 32, False),       # 4 pixels x 160 quads per block: one full iteration plus a partial one
    ("hilo", 2, 16, 16, 64, 32, True),              # hi + lo planes (3-product form)
    ("chan_runs", 96, 2, 2, 1024, 32, False),       # channel runs, cb = 128
]
FWD_IDS = [c[0] for c in FWD]
FORMS = [pytest.param(False, id="plain"), pytest.param(True, id="film")]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stedm_amd import _lib
    _lib.lib()  # must load: no fallback
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _clean_guard_word(dev):
    from stedm_amd import ops
    w = ops.f16_guard_enable()
    w.zero_()
    yield
    torch.cuda.synchronize()
    w.zero_()


def _prec(mode, hilo):
    from stedm_amd.ops import Precision
    return Precision.parse(("parity" if mode == "f16" else "parity_bf16") if hilo else mode)


_PROBLEMS = {}


def fwd_problem(case):
    """x [B, HW, C], its channel partials, gamma, beta and a film tensor [B, 2 C] (computed once per case, never modified)"""
    if case[0] not in _PROBLEMS:
        name, B, H, W, C, groups, hilo = case
        x = RG.normal((B, H * W, C), 0, f"drop.{name}.x", std=1.5, mean=0.3)
        _PROBLEMS[name] = dict(x=x, cs=RG.chan_partials(x), gamma=RG.normal((C,), 0, f"drop.{name}.g", std=0.5, mean=1.0),
                               beta=RG.normal((C,), 0, f"drop.{name}.b", std=0.5), film=RG.normal((B, 2 * C), 0, f"drop.{name}.film", std=0.5))
    return _PROBLEMS[case[0]]


def run_fwd(dev, case, mode, film, p=None, step=STEP, step_ptr=None, entry_p0=False):
    """the plain entry (p None), or the drop entry; returns (hi, lo, mr) on the CPU, flat [B, HW, C]"""
    from stedm_amd import ops
    name, B, H, W, C, groups, hilo = case
    prob = fwd_problem(case)
    prec = _prec(mode, hilo)
    x = prob["x"].view(B, H, W, C).to(dev)
    hi = torch.full((B, H, W, C), FILL16, dtype=torch.int16, device=dev)
    lo = torch.full((B, H, W, C), FILL16, dtype=torch.int16, device=dev) if hilo else None
    mr = torch.full((B, groups, 2), float("nan"), device=dev)
    g, b, cs = prob["gamma"].to(dev), prob["beta"].to(dev), prob["cs"].to(dev)
    fl = prob["film"].to(dev) if film else None
    if p is None:
        if film:
            ops.gn_apply16c_film(x, cs, hi, lo, prec, g, b, fl, 0, 2 * C, EPS, groups, 1, mean_rstd=mr)
        else:
            ops.gn_apply16c(x, cs, None, None, hi, lo, prec, g, b, EPS, groups, 1, 0, None, mean_rstd=mr)
    else:
        ops.gn_apply16c_drop(x, cs, hi, lo, prec, g, b, (p, SEED, RD.SITE0 + K, step, step_ptr), EPS, groups, 1, mean_rstd=mr, film=fl,
                             film_off=0, film_bstride=2 * C)
    torch.cuda.synchronize()
    return hi.cpu().view(B, H * W, C), None if lo is None else lo.cpu().view(B, H * W, C), mr.cpu()


def test_the_cases_reach_the_forms_they_name():
    for name, B, H, W, C, groups, hilo in FWD:
        kern, slab, cb, _ = RG.apply16c_geometry(B, H * W, C, 0, groups, hilo, False)
        assert kern == "v8"
        per_block = (cb // 4) * H * W if cb else slab * (C // 4)
        if name == "chan_runs":
            assert cb == 128
        else:
            assert cb == 0
        if name == "tail_only":
            assert per_block < 512
        if name == "full_tail":
            assert per_block > 512 and per_block % 512 != 0


@pytest.mark.parametrize("mode,dtype", DTYPES)
@pytest.mark.parametrize("film", FORMS)
@pytest.mark.parametrize("case", FWD, ids=FWD_IDS)
def test_drop_half_doubles_the_plain_planes_bitwise(dev, case, film, mode, dtype):
    name, B, H, W, C, groups, hilo = case
    hp, lp, mrp = run_fwd(dev, case, mode, film)
    hd, ld, mrd = run_fwd(dev, case, mode, film, p=0.5)
    assert torch.equal(mrp, mrd), "mean_rstd"
    keep = RD.resblock_mask(B, H * W, C, 0.5, SEED, K, STEP)
    ok = RD.doubled_in_range(hp, lp, dtype) | ~keep
    zero = torch.zeros((), dtype=dtype)
    for words_p, words_d, what in ((hp, hd, "hi"), (lp, ld, "lo")):
        if words_p is None:
            continue
        exp = torch.where(keep, words_p.view(dtype) * 2, zero).view(torch.int16)
        bad = ((exp != words_d) & ok).nonzero()
        assert len(bad) == 0, f"{what}: {len(bad)} plane words differ, first at {bad[0].tolist()}"
    print(f"[{name} film={film} {mode}] compared {int(ok.sum())} of {ok.numel()} elements, {int((~keep).sum())} dropped")
    assert int(ok.sum()) > (0.25 if (hilo and mode == "f16") else 0.9) * ok.numel()


@pytest.mark.parametrize("mode,dtype", DTYPES)
@pytest.mark.parametrize("film", FORMS)
@pytest.mark.parametrize("case", FWD, ids=FWD_IDS)
def test_drop_tenth_zeros_and_bound(dev, case, film, mode, dtype):
    name, B, H, W, C, groups, hilo = case
    p = 0.1
    prob = fwd_problem(case)
    hp, lp, _ = run_fwd(dev, case, mode, film)
    hd, ld, mr = run_fwd(dev, case, mode, film, p=p)
    keep = RD.resblock_mask(B, H * W, C, p, SEED, K, STEP)
    # +0 exactly where the mask drops; nonzero wherever it keeps and the plain output is nonzero
    assert bool((hd[~keep] == 0).all()) and (ld is None or bool((ld[~keep] == 0).all()))
    assert bool((hd[keep & (hp.view(dtype) != 0)].view(dtype) != 0).all())
    assert not bool((hd == FILL16).all(-1).any()), "a pixel of the plane was not written"
    x64, g64, b64 = prob["x"].double(), prob["gamma"].double(), prob["beta"].double()
    mr64 = RG.fold(prob["cs"], None, 0, groups, H * W, EPS)
    if film:
        s, sh = RF.film_rows(prob["film"].double(), B, C, 2 * C, 0)
        act = RF.film_group_norm(x64, groups, g64, b64, EPS, 1, s, sh, mean_rstd=mr64)
        plain_bound = RF.film_apply_bound(x64, mr64, g64, b64, s, sh, 1, dtype, hilo)
    else:
        act = RG.group_norm(x64, None, 0, groups, g64, b64, EPS, 1, mean_rstd=mr64)
        plain_bound = RG.apply_bound(x64, mr64, g64, b64, 1, dtype, hilo)
    ref = act * float(RD.inv_keep(p))
    err = (RG.planes_value(hd, ld, dtype) - ref).abs()
    r = RG.ratio(err[keep], RD.drop_apply_bound(plain_bound, ref, p)[keep])
    print(f"[{name} film={film} {mode}] worst err / bound over the kept elements: {r:.3f}")
    assert r < 1.0


@pytest.mark.parametrize("film", FORMS)
def test_step_pointer_adds_to_the_step_and_p0_is_the_plain_entry(dev, film):
    case = FWD[1]
    a = run_fwd(dev, case, "bf16", film, p=0.1, step=7)
    ptr = torch.tensor([2], dtype=torch.int32, device=dev)
    b = run_fwd(dev, case, "bf16", film, p=0.1, step=5, step_ptr=ptr)
    assert all(torch.equal(u, v) for u, v in zip(a, b) if u is not None)
    c = run_fwd(dev, case, "bf16", film, p=0.1, step=5)
    assert not torch.equal(a[0], c[0]), "another step must give another mask"
    # the step wraps modulo 2^32
    ptr.fill_(-1)
    d = run_fwd(dev, case, "bf16", film, p=0.1, step=8, step_ptr=ptr)
    assert torch.equal(a[0], d[0])
    plain = run_fwd(dev, case, "bf16", film)
    zero = run_fwd(dev, case, "bf16", film, p=0.0)
    assert all(torch.equal(u, v) for u, v in zip(plain, zero) if u is not None)


# ------------------------------------------------------------------------------------------------ backward
BWD = [RF.BWD[3], RF.BWD[4]]        # "ragged": the one-pass kernel (3 pixels per thread, dead lanes); "chain": the three-kernel chain
BWD_IDS = [c[0] for c in BWD]


def test_the_backward_cases_select_both_kernel_forms():
    assert [bool(RG.gn_bwd_fused_cb(c[4], 0, c[5], c[2] * c[3])[0]) for c in BWD] == [True, False]


def run_bwd(dev, case, prob, mode, film, dA, drop):
    from stedm_amd import ops
    name, B, H, W, C, groups, form, act, use_add, acc, acc_param, planes = case
    prec = _prec(mode, planes == "hilo")
    sh4 = (B, H, W, C)
    dx = prob["old"].view(sh4).to(dev).clone() if acc else torch.full(sh4, float("nan"), device=dev)
    hi = torch.full(sh4, FILL16, dtype=torch.int16, device=dev) if planes else None
    lo = torch.full(sh4, FILL16, dtype=torch.int16, device=dev) if planes == "hilo" else None
    dg = prob["dg0"].to(dev).clone() if acc_param else torch.full((C,), float("nan"), device=dev)
    db = prob["db0"].to(dev).clone() if acc_param else torch.full((C,), float("nan"), device=dev)
    dE = prob["dE0"].to(dev).clone()
    ws = torch.full((ops.gn_bwd_ws_floats(B, H * W, C, groups),), float("nan"), device=dev)
    x, mr, g, b = prob["x"].view(sh4).to(dev), prob["mr32"].to(dev), prob["gamma"].to(dev), prob["beta"].to(dev)
    add = None if prob["add"] is None else prob["add"].view(sh4).to(dev)
    fl = prob["film"].to(dev)
    d16 = None if hi is None else (hi, lo)
    if drop is not None:
        ops.gn_bwd_drop(x, mr, g, b, groups, act, dA, add, ws, dx, acc, d16, prec, dg, db, acc_param, drop, film=fl if film else None,
                        film_off=prob["off"], film_bstride=prob["bstride"], d_film=dE if film else None, d_film_off=prob["d_off"])
    elif film:
        ops.gn_bwd_film(x, mr, g, b, groups, act, fl, prob["off"], prob["bstride"], dA, add, ws, dx, acc, d16, prec, dg, db, acc_param, dE,
                        prob["d_off"])
    else:
        ops.gn_bwd(x, None, mr, g, b, groups, act, dA, add, ws, dx, acc, None, False, d16, prec, dg, db, acc_param)
    torch.cuda.synchronize()
    flat = lambda t: None if t is None else t.cpu().view(B, H * W, C)
    return dict(dx=flat(dx), hi=flat(hi), lo=flat(lo), dgamma=dg.cpu(), dbeta=db.cpu(), dE=dE.cpu())


@pytest.mark.parametrize("mode,dtype", DTYPES)
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("film", FORMS)
@pytest.mark.parametrize("case", BWD, ids=BWD_IDS)
def test_backward_drop_equals_the_plain_entry_on_the_masked_gradient(dev, case, film, p, mode, dtype):
    name, B, H, W, C, groups, form, act, use_add, acc, acc_param, planes = case
    prob = RF.bwd_problem(case, dtype)
    keep = RD.resblock_mask(B, H * W, C, p, SEED, K, STEP)
    dA = prob["dA"].view(B, H, W, C).to(dev)
    eff = RD.dA_eff(dA, keep.view(B, H, W, C), p)
    got = run_bwd(dev, case, prob, mode, film, dA, (p, SEED, RD.SITE0 + K, STEP - 3, torch.tensor([3], dtype=torch.int32, device=dev)))
    exp = run_bwd(dev, case, prob, mode, film, eff, None)
    for k in ("dx", "hi", "lo", "dgamma", "dbeta") + (("dE",) if film else ()):
        if exp[k] is not None:
            assert not bool(torch.isnan(got[k].float()).any()), k
            assert torch.equal(got[k], exp[k]), f"{k} differs from the plain entry on dA_eff"
    # against the fp64 closed form on dA_eff, within the plain backward's bounds
    eff_c = eff.cpu().view(B, H * W, C)
    if film:
        ref, bounds = RD.film_bwd_reref(case, prob, dtype, eff_c)
        r = RF.bwd_ratios(case, dict(prob, ref=ref, bounds=bounds), got, dtype)
    else:
        out = dict(dx1=got["dx"], hi=got["hi"], lo=got["lo"], dgamma=got["dgamma"], dbeta=got["dbeta"])
        r = RG.bwd_ratios((name, B, H, W, C, 0, groups), prob["x"], None, prob["mr32"], prob["gamma"], prob["beta"], act, eff_c, prob["add"],
                          prob["old"], None, dtype, planes, prob["dg0"] if acc_param else None, prob["db0"] if acc_param else None, out)
    print(f"[{name} film={film} p={p} {mode}] worst err / bound", {k: round(v, 3) for k, v in r.items()})
    assert max(r.values()) < 1.0, r


def test_argument_errors(dev):
    from stedm_amd import _lib
    L = _lib.lib()
    B, H, W, C, groups = 2, 4, 4, 32, 8
    x = torch.zeros((B, H, W, C), device=dev)
    cs = torch.zeros((B, 1, C, 2), device=dev)
    hi = torch.zeros((B, H, W, C), dtype=torch.int16, device=dev)
    gm, bt = torch.ones(C, device=dev), torch.zeros(C, device=dev)

    def call(p=0.1, x2=None, c2=0, cs2=None, raw=None, c=C):
        return L.stedm_gn_apply16c_drop(x.data_ptr(), c, cs.data_ptr(), 1, x2, c2, cs2, 1 if x2 else 0, 0, gm.data_ptr(), bt.data_ptr(), 1e-5, groups, 1,
                                        B, H * W, hi.data_ptr(), None, raw, None, None, _lib.BF16, p, 1, RD.SITE0, 0, None, None)
    assert call() == 0
    assert call(p=1.0) != 0 and call(p=-0.1) != 0, "p outside [0, 1) must be an argument error"
    assert call(x2=x.data_ptr(), c2=8, cs2=cs.data_ptr()) != 0, "x2 != NULL must be an argument error"
    assert call(raw=hi.data_ptr()) != 0, "raw planes must be an argument error"
    assert call(c=36) != 0, "C % 8 != 0 must be an argument error"
    torch.cuda.synchronize()


def test_backward_argument_errors(dev):
    """The C entries stedm_gn_bwd_film / _drop / _film_drop: a valid call returns 0, every bad argument set below is refused on the host
    before any launch, and with p = 0 the drop entries are the plain / FiLM entries bit for bit."""
    from stedm_amd import _lib, ops
    L = _lib.lib()
    B, H, W, C, groups = 2, 4, 4, 32, 8
    x = RG.normal((B, H * W, C), 0, "drop.bwdargs.x", std=1.5, mean=0.3).to(dev)
    dA = RG.normal((B, H * W, C), 0, "drop.bwdargs.dA").to(dev)
    gm, bt = RG.normal((C,), 0, "drop.bwdargs.g", std=0.5, mean=1.0).to(dev), RG.normal((C,), 0, "drop.bwdargs.b", std=0.5).to(dev)
    film = RG.normal((B, 2 * C), 0, "drop.bwdargs.film", std=0.5).to(dev)
    xg = x.view(B, H * W, groups, C // groups).double()
    mean, var = xg.mean((1, 3)), xg.var((1, 3), unbiased=False)
    mr = torch.stack((mean, (var + EPS).rsqrt()), -1).float().contiguous()
    ws = torch.zeros((ops.gn_bwd_ws_floats(B, H * W, C, groups),), device=dev)
    drop_tail = lambda p: (p, SEED, RD.SITE0 + K, STEP, None)

    def outs():
        return dict(dx=torch.full((B, H * W, C), float("nan"), device=dev), hi=torch.full((B, H * W, C), FILL16, dtype=torch.int16, device=dev),
                    dg=torch.full((C,), float("nan"), device=dev), db=torch.full((C,), float("nan"), device=dev),
                    dE=torch.full((B, 2 * C), float("nan"), device=dev))

    def plain(o):
        return L.stedm_gn_bwd(x.data_ptr(), C, None, 0, mr.data_ptr(), gm.data_ptr(), bt.data_ptr(), groups, 1, dA.data_ptr(), None, B, H * W,
                              ws.data_ptr(), o["dx"].data_ptr(), 0, None, 0, o["hi"].data_ptr(), None, _lib.BF16, o["dg"].data_ptr(),
                              o["db"].data_ptr(), 0, None)

    def film_call(o, entry="stedm_gn_bwd_film", film_ptr=film.data_ptr(), film_off=0, d_bs=2 * C, tail=()):
        return getattr(L, entry)(x.data_ptr(), C, mr.data_ptr(), gm.data_ptr(), bt.data_ptr(), groups, 1, film_ptr, 2 * C, film_off, dA.data_ptr(), None,
                                 B, H * W, ws.data_ptr(), o["dx"].data_ptr(), 0, o["hi"].data_ptr(), None, _lib.BF16, o["dg"].data_ptr(),
                                 o["db"].data_ptr(), 0, o["dE"].data_ptr(), d_bs, 0, *tail, None)

    def drop_call(o, p=0.1, x2=None, c=C):
        return L.stedm_gn_bwd_drop(x.data_ptr(), c, x2, 0, mr.data_ptr(), gm.data_ptr(), bt.data_ptr(), groups, 1, dA.data_ptr(), None, B, H * W,
                                   ws.data_ptr(), o["dx"].data_ptr(), 0, None, 0, o["hi"].data_ptr(), None, _lib.BF16, o["dg"].data_ptr(),
                                   o["db"].data_ptr(), 0, *drop_tail(p), None)

    o = outs()
    assert film_call(o) == 0
    assert drop_call(o) == 0
    assert film_call(o, entry="stedm_gn_bwd_film_drop", tail=drop_tail(0.1)) == 0
    assert film_call(o, film_ptr=None) != 0, "gn_bwd_film: a null film must be an argument error"
    assert film_call(o, film_off=2) != 0, "gn_bwd_film: film_off must be a multiple of 4"
    assert film_call(o, d_bs=2 * C - 1) != 0, "gn_bwd_film: a d_film row shorter than d_film_off + 2 C must be an argument error"
    assert drop_call(o, x2=x.data_ptr()) != 0, "gn_bwd_drop: x2 != NULL must be an argument error"
    assert drop_call(o, p=1.0) != 0 and drop_call(o, p=-0.1) != 0, "gn_bwd_drop: p outside [0, 1) must be an argument error"
    assert drop_call(o, c=36) != 0, "gn_bwd_drop: C % 8 != 0 must be an argument error"
    assert film_call(o, entry="stedm_gn_bwd_film_drop", film_ptr=None, tail=drop_tail(0.1)) != 0, "gn_bwd_film_drop: a null film must be an argument error"
    # p = 0: the drop entries forward to the plain / FiLM entries
    a, b = outs(), outs()
    assert plain(a) == 0 and drop_call(b, p=0.0) == 0
    torch.cuda.synchronize()
    for k in ("dx", "hi", "dg", "db"):
        assert not bool(torch.isnan(a[k].float()).any()) and torch.equal(a[k], b[k]), f"gn_bwd_drop(p=0) {k} differs from gn_bwd"
    a, b = outs(), outs()
    assert film_call(a) == 0 and film_call(b, entry="stedm_gn_bwd_film_drop", tail=drop_tail(0.0)) == 0
    torch.cuda.synchronize()
    for k in ("dx", "hi", "dg", "db", "dE"):
        assert not bool(torch.isnan(a[k].float()).any()) and torch.equal(a[k], b[k]), f"gn_bwd_film_drop(p=0) {k} differs from gn_bwd_film"
