"""CPU tier: pins tests/refs_opt.py, the float64 reference and the per-element bounds that tests/test_gpu_opt_exact.py holds the optimizer
kernels to. The reference against torch.optim.AdamW and oracle.train in float64; the bounds from both sides: two honest fp32 evaluations
(torch's own CPU arithmetic through oracle.train, and a fully contracted one) must lie inside them on every element of the designated
inputs, and each of twelve plausible wrong optimizers must leave them on at least one. The largest error-to-bound ratios are printed."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import refs_opt as RO


@pytest.fixture(scope="module")
def data():
    """{case name: (inputs (p, g, m, v, e), scalars, step64, bounds)}: computed once, read-only"""
    out = {}
    for c in RO.CASES:
        x = RO.elements(c, "cpu", RO.CPU_N)
        S = RO.case_scalars(c)
        out[c.name] = (x, S, RO.step64(*x, S), RO.bounds(*x, S))
    return out


# ------------------------------------------------------------------------------------------------ the reference
def _three_step_inputs():
    c = RO.CASE["step1000"]
    tensors = [RO.elements(c, f"torch{i}", n)[0].astype(np.float64) for i, n in enumerate((1, 37, 4097, 9000))]
    grads = [[RO.elements(c, f"torch{i}.g{s}", len(t))[1].astype(np.float64) for i, t in enumerate(tensors)] for s in (1, 2, 3)]
    return tensors, grads


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_reference_is_torch_adamw_and_the_oracle_in_float64(wd):
    """three steps from a fresh state on four tensors: step64 with the bias corrections kept in double (exact_bias, torch's choice) against
    torch.optim.AdamW and against oracle.train.adamw_step / ema_update, all in float64, to 1e-12 of the terms each output is summed from"""
    from oracle import train as otrain
    tensors, grads = _three_step_inputs()
    S0 = RO.scalars(1, 1e-3, wd, 0.9999, exact_bias=True)
    tp = [torch.nn.Parameter(torch.from_numpy(t.copy())) for t in tensors]
    opt = torch.optim.AdamW(tp, lr=S0.lr, betas=(S0.b1, S0.b2), eps=S0.eps, weight_decay=S0.wd)
    st = [dict(p=t.copy(), m=np.zeros_like(t), v=np.zeros_like(t), e=t.copy()) for t in tensors]
    orc = [[torch.from_numpy(t.copy()), torch.zeros(len(t), dtype=torch.float64), torch.zeros(len(t), dtype=torch.float64),
            torch.from_numpy(t.copy())] for t in tensors]
    for s in (1, 2, 3):
        S = RO.scalars(s, 1e-3, wd, 0.9999, exact_bias=True)
        for q, g in zip(tp, grads[s - 1]):
            q.grad = torch.from_numpy(g.copy())
        opt.step()
        for i, g in enumerate(grads[s - 1]):
            prev = st[i]
            st[i] = RO.step64(prev["p"], g, prev["m"], prev["v"], prev["e"], S)
            o = orc[i]
            otrain.adamw_step(o[0], torch.from_numpy(g.copy()), o[1], o[2], s, S.lr, S.b1, S.b2, S.eps, S.wd)
            otrain.ema_update(o[3], o[0], 1.0 - S.omd)
            mag = {"m": np.abs(prev["m"]) + np.abs(g), "v": np.abs(prev["v"]) + g * g, "p": np.abs(prev["p"]) + 10 * S.lr,
                   "e": np.abs(prev["e"]) + np.abs(prev["p"]) + 10 * S.lr}
            tstate = opt.state[tp[i]]
            for k, got in (("p", tp[i].detach()), ("m", tstate["exp_avg"]), ("v", tstate["exp_avg_sq"])):
                assert (np.abs(got.numpy() - st[i][k]) <= 1e-12 * mag[k]).all(), ("torch", s, i, k)
            for k, got in (("p", o[0]), ("m", o[1]), ("v", o[2]), ("e", o[3])):
                assert (np.abs(got.numpy() - st[i][k]) <= 1e-12 * mag[k]).all(), ("oracle", s, i, k)


def test_rounded_bias_corrections_move_the_step_by_what_the_bound_charges():
    """the entry points round bc1 and sqrt(bc2) to fp32; against the double ones the update k q moves by at most (1 + 1.5) u relative"""
    for c in RO.CASES:
        x = RO.elements(c, "cpu", 4096)
        a, b = RO.case_scalars(c), RO.case_scalars(c, exact_bias=True)
        assert a.bc1 == float(np.float32(b.bc1)) and abs(a.bc2s - b.bc2s) <= 1.5 * RO.U * b.bc2s
        ta, tb = RO._trace64(*x, a), RO._trace64(*x, b)
        kq = np.abs(tb["k"] * tb["q"])
        assert (np.abs(ta["p"] - tb["p"]) <= 2.5 * RO.U * kq * RO.SLACK + 1e-15 * np.abs(tb["p"])).all(), c.name


def test_scalars_are_the_fp32_values_the_entry_points_form():
    S = RO.scalars(1000, 1e-3, 0.01, 0.9999, 0.5, 0.37)
    assert S.lr == float(np.float32(1e-3)) and S.b1 == float(np.float32(0.9)) and S.eps == float(np.float32(1e-8))
    assert S.gs == float(np.float32(np.float32(0.5) * np.float32(0.37)))
    assert S.bc2s == float(np.sqrt(np.float32(1.0 - float(np.float32(0.999)) ** 1000)))
    # the fp32 difference is exact and 1.66e-4 above the double one (refs_opt's docstring: mutant 12)
    assert S.omd == 1.0 - float(np.float32(0.9999)) and abs(S.omd / (1.0 - 0.9999) - 1.0) > 1.6e-4
    assert RO.scalars(1, 1e-3, 0.01, 0.9999, 0.5, 1.0).gs == 0.5          # a coefficient of exactly 1 leaves the scale's bits
    assert RO.sched_row(S) == [S.bc1, S.bc2s, float(np.float32(0.9999)), S.lr]


# ------------------------------------------------------------------------------------------------ exact fp32 arithmetic
def _rn32(x: Fraction) -> np.float32:
    """round a rational to fp32, nearest even, by exact comparison with the neighbours"""
    f = np.float32(float(x))
    cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    best = min(cands, key=lambda c: (abs(Fraction(float(c)) - x), int(np.float32(c).view(np.int32)) & 1))
    return np.float32(best)


def test_fma32_is_one_rounding():
    from stedm_amd.utils import prng
    # 1 + 2^-23 + (1 + 2^-23)(1 - 2^-23) 2^-24 lies 2^-70 below the midpoint of 1 + 2^-23 and 1 + 2^-22: the float64 sum IS the midpoint, and
    # rounding it again would tie to the even 1 + 2^-22
    a, b, c = np.float32(1 + 2.0 ** -23), np.float32((1 - 2.0 ** -23) * 2.0 ** -24), np.float32(1 + 2.0 ** -23)
    assert np.float32(np.float64(a) * np.float64(b) + np.float64(c)) == np.float32(1 + 2.0 ** -22)
    assert RO.fma32(a, b, c) == c and RO.fma32(a, -b, -c) == -c
    u = prng.uniform(RO.SEED, "opt.fma", (3, 400), -1.0, 1.0).numpy()
    A, B = u[0], u[1] * np.float32(2.0 ** -24)
    Cc = np.where(np.arange(400) % 2 == 0, u[2], np.float32(1.0) + np.round(u[2] * 8).astype(np.float32) * np.float32(2.0 ** -23))
    got = RO.fma32(A, B, Cc)
    for i in range(400):
        assert got[i] == _rn32(Fraction(float(A[i])) * Fraction(float(B[i])) + Fraction(float(Cc[i]))), i


def test_ema_candidates_are_the_two_roundings():
    c = RO.CASE["step1000"]
    p, _, _, _, e = RO.elements(c, "cand", 300)
    S = RO.case_scalars(c)
    unf, fus = RO.ema_candidates(e, p, S)
    omd = Fraction(S.omd)
    for i in range(300):
        d = _rn32(Fraction(float(e[i])) - Fraction(float(p[i])))
        assert fus[i] == _rn32(Fraction(float(e[i])) - omd * Fraction(float(d))), i
        assert unf[i] == _rn32(Fraction(float(e[i])) - Fraction(float(_rn32(omd * Fraction(float(d)))))), i
    assert (np.abs(unf.astype(np.float64) - RO.ema64(e, p, S)) <= 3 * RO.U * np.abs(e.astype(np.float64)) + 2 * RO.U * S.omd * np.abs(p.astype(np.float64))).all()


# ------------------------------------------------------------------------------------------------ the designated inputs
def test_designated_inputs_cover_what_they_claim(data):
    tiny = float(np.finfo(np.float32).tiny)
    for c in RO.CASES:
        (p, g, m, v, e), S, ref, _ = data[c.name]
        assert all(a.dtype == np.float32 and a.size == RO.CPU_N < 20000 for a in (p, g, m, v, e))
        nz = np.abs(g[g != 0]).astype(np.float64)
        assert nz.min() * S.gs >= 1e-15 and nz.min() < 1e-9 and nz.max() > 1.0 and (g < 0).any() and (g > 0).any()
        assert (g == 0).any() and (m == 0).any() and (v == 0).any() and ((g == 0) & (m == 0) & (v == 0)).any() and (p == 0).any() and (e == 0).any()
        t = RO._trace64(p, g, m, v, e, S)
        for k in ("gp", "m", "v", "s", "q", "pn", "p", "d", "e"):
            a = np.abs(t[k])
            assert np.isfinite(a).all() and (a[a != 0] > 1e3 * tiny).all() and a.max() < 1e30, (c.name, k)
        c2g = (1.0 - S.b2) * np.abs(t["gp"])
        assert (c2g[c2g != 0] > 1e3 * tiny).all() and ((c2g * np.abs(t["gp"]))[c2g != 0] > 1e3 * tiny).all()
        # g = m = v = 0: the moments stay exactly 0 and the update is exactly the decay
        z = (g == 0) & (m == 0) & (v == 0)
        assert (ref["m"][z] == 0).all() and (ref["v"][z] == 0).all() and (ref["p"][z] == p[z].astype(np.float64) * (1.0 - S.lr * S.wd)).all()
        if c.state == "fresh":
            assert not m.any() and not v.any() and c.step == 1
        if c.state == "tiny_v":
            assert (v[m != 0] <= 1e-11 * m[m != 0].astype(np.float64) ** 2).all()
    assert {c.wd for c in RO.CASES} == {0.0, 0.01} and {c.lr for c in RO.CASES} == {1e-3, 2e-4}
    assert {c.grad_scale for c in RO.CASES} == {1.0, 0.5, 1.0 / 3.0} and {c.step for c in RO.CASES} == {1, 2, 1000, 100000}
    assert {c.decay for c in RO.CASES} == {2.0 / 11.0, 0.9999} and {c.clip_coef for c in RO.CASES} == {None, 1.0, 0.37}


# ------------------------------------------------------------------------------------------------ the bounds, from both sides
EVALS = [("oracle fp32", RO.step32_oracle), ("contracted fp32", RO.step32_contracted)]


def test_honest_fp32_evaluations_lie_inside_the_bounds(data):
    worst = {name: dict.fromkeys(RO.OUTS, 0.0) for name, _ in EVALS}
    for c in RO.CASES:
        x, S, ref, bnd = data[c.name]
        for name, fn in EVALS:
            got = fn(*x, S)
            r = RO.ratios(got, ref, bnd)
            for k in RO.OUTS:
                worst[name][k] = max(worst[name][k], r[k])
            assert all(v <= 1.0 for v in r.values()), (c.name, name, r)
            z = (x[1] == 0) & (x[2] == 0) & (x[3] == 0)
            assert not got["m"][z].any() and not got["v"][z].any()
    for name, w in worst.items():
        print(f"[opt bounds, CPU] {name}: largest error / bound  " + "  ".join(f"{k} {w[k]:.3f}" for k in RO.OUTS))
    # a tensor without a shadow: the same three outputs, no fourth
    x, S, ref, bnd = data["step1000"]
    got = RO.step32_contracted(*x[:4], None, S)
    assert set(got) == set(RO.step64(*x[:4], None, S)) == set(RO.bounds(*x[:4], None, S)) == {"m", "v", "p"}
    assert all(np.array_equal(got[k], RO.step32_contracted(*x, S)[k]) for k in got)


def test_every_mutant_leaves_the_bounds(data):
    assert len(RO.MUTANTS) == 12
    for mut in RO.MUTANTS:
        caught = []
        for c in RO.CASES:
            x, S, ref, bnd = data[c.name]
            got = mut(*x, S)
            out = {k: int((~(np.abs(got[k] - ref[k]) <= bnd[k])).sum()) for k in RO.OUTS}
            if any(out.values()):
                caught.append((c.name, out))
        print(f"[opt mutants] {mut.__name__}: " + ("caught in " + "; ".join(f"{n} " + " ".join(f"{k}:{v}" for k, v in o.items() if v) for n, o in caught)
                                                    if caught else "NOT CAUGHT"))
        assert caught, f"mutant {mut.__name__} stays inside the bounds on every designated element"
