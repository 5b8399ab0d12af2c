"""References and bounds for the optimizer kernels (stedm_adamw_ema and its _clip / _sched / _pack forms, stedm_ema_update;
include/stedm_hip.h). CPU only, numpy. Written from oracle/train.py (adamw_step, ema_update: torch.optim.AdamW and LitEma) and the header, not
from the kernel bodies. Shared by tests/test_opt_refs_cpu.py (pins everything here: the reference against torch.optim.AdamW in float64, the
bounds against two honest fp32 evaluations, the mutants against the bounds) and tests/test_gpu_opt_exact.py (pins the kernels).

THE STEP (step64). Inputs are the fp32 tensors and the fp32 scalars the host passes (scalars()), every operation exact to float64:
    g' = g * gs                                   gs = grad_scale, or fl(grad_scale * clip_coef) for the _clip forms (one fp32 product)
    m' = b1 m + (1 - b1) g'
    v' = b2 v + (1 - b2) g'^2
    p' = p (1 - lr wd) - (lr / bc1) * m' / (sqrt(v') / bc2s + eps)
    e' = e - omd (e - p')
    bc1 = fl(1 - b1^step) (the power in double), bc2s = sqrtf(fl(1 - b2^step)), omd = fl(1.0f - fl(decay)).
omd is the FP32 difference: LitEma keeps `decay` as a float32 buffer and forms `1.0 - decay` by tensor arithmetic (ema.py:25-44), and the kernels
take the decay as a C float and subtract in fp32. For decay 0.9999 that difference is exact (fl(0.9999) is a multiple of 2^-24 below 1), so
omd = 1.000166e-4, not the 1e-4 that `1.0 - 0.9999` gives in double: 1.66e-4 relative apart, which is mutant 12.

THE BOUNDS (bounds). u = 2^-24. Every fp32 operation of an honest implementation is correctly rounded (the build sets no fast-math flag: division
and sqrtf included), so it perturbs its result x by at most u |x|; each perturbation is carried to the outputs through the partial derivative of
the step (first order), magnitudes taken from the float64 reference, and the sum is multiplied by SLACK = 1 + 2^-10 for the second-order terms
(relative 2^-24 of what is kept) and the reference's own float64 rounding. A fused multiply-add removes a rounding and adds none, so counting the
rounding of every product AND every sum holds for every contraction the compiler may choose. Rounding points, [n] = the u-multiple charged:
    g'    [1]  the product g * gs
    c1    [1]  the constant 1.0f - b1               c2  [1]  the constant 1.0f - b2
    m'    b1 m [1], c1 g' [1], the sum [1]                                      Bm = u (|b1 m| + 3 |c1 g'| + |m'|)       (g', c1, c1 g' -> 3)
    v'    b2 v [1], c2 g' [1], (c2 g') g' [1], the sum [1]; g' enters twice      Bv = u (b2 v + 5 c2 g'^2 + v')           (2 g', c2, two products -> 5)
    s     = sqrtf(v') [1]                                                       Bs = Bv / (2 s) + u s                    (Bv = 0 where v' = 0)
    d1    = s / bc2s [1], bc2s itself [2.5, see below]                          Bd1 = Bs / bc2s + 3.5 u d1
    den   = d1 + eps [1]                                                        Bden = Bd1 + u den
    q     = m' / den [1]                                                        Bq = Bm / den + |q| Bden / den + u |q|
    cw    = 1.0f - lr * wd: the product [1] and the difference [1]              Bcw = u (lr wd + cw)
    pn    = p * cw [1]                                                          Bpn = u |pn| + |p| Bcw
    k     = lr / bc1 [1], bc1 itself [1, see below]; k * q [1]; the difference [1]
                                                                                Bp = Bpn + k Bq + 3 u |k q| + u |p'|
    e'    d = e - p' [1], omd * d [1], the difference [1]; omd is exact by definition
                                                                                Be = omd Bp + 2 u omd |d| + u |e'|
The two "see below": the kernels receive bc1 and bc2s as computed above, so for them those are exact. torch.optim.AdamW (and oracle.train.adamw_step)
keep 1 - b^step in double and round lr / bc1 and sqrt(bc2) to fp32 once, another honest choice: its k differs from ours by the rounding of bc1 (u)
and its divisor by the roundings of bc2 (u / 2 after the root), of sqrtf (u) and of its own (u), 2.5 u. The bound admits both, so that it can be
checked against an implementation that shares no code with the kernels. No constant here was fitted to any output; the CPU tier prints how much
of the bound the honest evaluations use and requires every mutant below to leave it."""
from __future__ import annotations

from collections import namedtuple
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
OUTS = ("m", "v", "p", "e")

Scalars = namedtuple("Scalars", "lr b1 b2 eps wd gs bc1 bc2s omd decay step")


def f32(x) -> np.float32:
    return np.float32(x)


def scalars(step: int, lr: float, wd: float, decay: float, grad_scale: float = 1.0, clip_coef: Optional[float] = None, beta1: float = 0.9,
            beta2: float = 0.999, eps: float = 1e-8, exact_bias: bool = False) -> Scalars:
    """The scalars of one step as the entry points form them, each an fp32 value held in a Python float. exact_bias: bc1 and bc2s stay in
    double (torch.optim.AdamW's choice; for the float64 comparison with it). `decay` keeps the caller's double for mutant 12."""
    b1, b2 = float(f32(beta1)), float(f32(beta2))
    gs = f32(grad_scale)
    if clip_coef is not None:
        gs = f32(gs * f32(clip_coef))             # __fmul_rn(grad_scale, *clip_coef)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    if exact_bias:
        bc1, bc2s = bc1, float(np.sqrt(bc2))
    else:
        bc1, bc2s = float(f32(bc1)), float(np.sqrt(f32(bc2)))
    omd = float(f32(1.0) - f32(decay))
    return Scalars(float(f32(lr)), b1, b2, float(f32(eps)), float(f32(wd)), float(gs), bc1, bc2s, omd, float(decay), int(step))


def sched_row(S: Scalars) -> List[float]:
    """{bc1, sqrt(bc2), ema_decay, lr}: the row of the device schedule that states the same step (stedm_adamw_ema_sched)"""
    return [S.bc1, S.bc2s, float(f32(S.decay)), S.lr]


def _d(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def _trace64(p, g, m, v, e, S: Scalars) -> Dict[str, np.ndarray]:
    p, g, m, v, e = _d(p), _d(g), _d(m), _d(v), _d(e)
    t = {}
    t["gp"] = g * S.gs
    t["m"] = S.b1 * m + (1.0 - S.b1) * t["gp"]
    t["v"] = S.b2 * v + (1.0 - S.b2) * t["gp"] * t["gp"]
    t["s"] = np.sqrt(t["v"])
    t["d1"] = t["s"] / S.bc2s
    t["den"] = t["d1"] + S.eps
    t["q"] = t["m"] / t["den"]
    t["cw"] = 1.0 - S.lr * S.wd
    t["pn"] = p * t["cw"]
    t["k"] = S.lr / S.bc1
    t["p"] = t["pn"] - t["k"] * t["q"]
    if e is not None:
        t["d"] = e - t["p"]
        t["e"] = e - S.omd * t["d"]
    return t


def step64(p, g, m, v, e, S: Scalars) -> Dict[str, np.ndarray]:
    """One AdamW + EMA step in float64 -> {"m", "v", "p", "e"} (no "e" for a tensor without a shadow: e None)"""
    t = _trace64(p, g, m, v, e, S)
    return {k: t[k] for k in OUTS if k in t}


def ema64(e, p, S: Scalars) -> np.ndarray:
    """LitEma.forward alone in float64"""
    e, p = _d(e), _d(p)
    return e - S.omd * (e - p)


def bounds(p, g, m, v, e, S: Scalars) -> Dict[str, np.ndarray]:
    """Per-element bound on |fp32 implementation - step64| for each output (module docstring)"""
    t = _trace64(p, g, m, v, e, S)
    p, m, v = _d(p), _d(m), _d(v)
    c1, c2 = 1.0 - S.b1, 1.0 - S.b2
    ag = np.abs(t["gp"])
    Bm = U * (np.abs(S.b1 * m) + 3.0 * c1 * ag + np.abs(t["m"]))
    Bv = U * (S.b2 * np.abs(v) + 5.0 * c2 * ag * ag + t["v"])
    s = t["s"]
    with np.errstate(divide="ignore", invalid="ignore"):
        Bs = np.where(s > 0, Bv / (2.0 * s), 0.0) + U * s
    Bd1 = Bs / S.bc2s + 3.5 * U * t["d1"]
    Bden = Bd1 + U * t["den"]
    aq = np.abs(t["q"])
    Bq = Bm / t["den"] + aq * Bden / t["den"] + U * aq
    lw = S.lr * S.wd
    Bpn = U * np.abs(t["pn"]) + np.abs(p) * U * (lw + t["cw"])
    Bp = Bpn + t["k"] * Bq + 3.0 * U * t["k"] * aq + U * np.abs(t["p"])
    out = {"m": Bm * SLACK, "v": Bv * SLACK, "p": Bp * SLACK}
    if e is not None:
        out["e"] = (S.omd * Bp + 2.0 * U * S.omd * np.abs(t["d"]) + U * np.abs(t["e"])) * SLACK
    return out


def ratios(got: Dict[str, np.ndarray], ref: Dict[str, np.ndarray], bnd: Dict[str, np.ndarray]) -> Dict[str, float]:
    """largest |got - ref| / bound per output; an error where the bound is 0, a NaN or an inf counts as inf"""
    out = {}
    for k in ref:
        err = np.abs(_d(got[k]) - ref[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / bnd[k])
        r = np.where(np.isfinite(r), r, np.inf)
        out[k] = float(r.max()) if r.size else 0.0
    return out


# ------------------------------------------------------------------------------------------------ exact fp32 arithmetic through float64
def fma32(a, b, c) -> np.ndarray:
    """fl32(a * b + c) with ONE rounding, a, b, c fp32. The product of two fp32 values is exact in float64; the float64 sum r and its exact
    residue (TwoSum) say on which side of r the true value lies, which matters only where r is the midpoint of two fp32 neighbours: between
    any other double and the true value there is no fp32 midpoint, because a midpoint is itself a double and r is the nearest one."""
    a, b, c = _d(a), _d(b), _d(c)
    x = a * b
    r = x + c
    bb = r - x
    res = (x - (r - bb)) + (c - bb)
    f = r.astype(np.float32)
    fd = f.astype(np.float64)
    lo = np.where(fd <= r, f, np.nextafter(f, f32(-np.inf)))
    hi = np.where(lo.astype(np.float64) == r, lo, np.nextafter(lo, f32(np.inf)))
    mid = 0.5 * (lo.astype(np.float64) + hi.astype(np.float64))
    fix = (mid == r) & (lo != hi) & (res != 0) & np.isfinite(r)
    return np.where(fix, np.where(res > 0, hi, lo), f).astype(np.float32)


def _a32(x):
    return np.asarray(x, dtype=np.float32)


def ema_candidates(e, p, S: Scalars) -> Tuple[np.ndarray, np.ndarray]:
    """The two fp32 roundings of s - omd (s - p): (every operation rounded, the last multiply-subtract fused)"""
    e, p = _a32(e), _a32(p)
    omd = f32(S.omd)
    d = e - p
    return e - omd * d, fma32(-omd, d, e)


def step32_contracted(p, g, m, v, e, S: Scalars) -> Dict[str, np.ndarray]:
    """An honest fp32 step with every a * b + c fused (one rounding), the other operations rounded one by one"""
    p, g, m, v = _a32(p), _a32(g), _a32(m), _a32(v)
    lr, b1, b2, eps, wd, gs, bc1, bc2s, omd = (f32(x) for x in (S.lr, S.b1, S.b2, S.eps, S.wd, S.gs, S.bc1, S.bc2s, S.omd))
    one = f32(1.0)
    gp = g * gs
    cw = fma32(-lr, wd, one)
    pn = p * cw
    m1 = fma32(b1, m, (one - b1) * gp)
    v1 = fma32((one - b2) * gp, gp, b2 * v)
    den = np.sqrt(v1) / bc2s + eps
    p1 = fma32(-(lr / bc1), m1 / den, pn)
    out = {"m": m1, "v": v1, "p": p1}
    if e is not None:
        e = _a32(e)
        out["e"] = fma32(-omd, e - p1, e)
    return out


def step32_oracle(p, g, m, v, e, S: Scalars) -> Dict[str, np.ndarray]:
    """oracle.train.adamw_step / ema_update on float32 tensors (torch's CPU arithmetic): the gradient scaled in fp32 first, the betas, lr, wd
    and decay handed over as the doubles that hold their fp32 values. It forms bc1 and sqrt(bc2) in double itself."""
    import torch
    from oracle import train as otrain
    tp, tm, tv = (torch.from_numpy(_a32(x).copy()) for x in (p, m, v))
    tg = torch.from_numpy(_a32(g) * f32(S.gs))
    otrain.adamw_step(tp, tg, tm, tv, S.step, S.lr, S.b1, S.b2, S.eps, S.wd)
    out = {"m": tm.numpy(), "v": tv.numpy(), "p": tp.numpy()}
    if e is not None:
        te = torch.from_numpy(_a32(e).copy())
        assert 1.0 - (1.0 - S.omd) == S.omd             # the oracle forms 1.0 - decay in double: hand it the decay that gives omd back
        otrain.ema_update(te, tp, 1.0 - S.omd)
        out["e"] = te.numpy()
    return out


# ------------------------------------------------------------------------------------------------ mutants
def _mutant(kind: str) -> Callable:
    def step(p, g, m, v, e, S: Scalars):
        p, g, m, v, e = _d(p), _d(g), _d(m), _d(v), _d(e)
        gm = gv = g * S.gs
        if kind == "scale_not_in_v":
            gv = g
        if kind == "coupled_decay":
            gm = gv = gm + S.wd * p
        m1 = S.b1 * m + (1.0 - S.b1) * gm
        v1 = S.b2 * v + (1.0 - S.b2) * gv * gv
        if kind == "scale_once_in_v":
            v1 = S.b2 * v + (1.0 - S.b2) * g * g * S.gs
        with np.errstate(divide="ignore", invalid="ignore"):
            if kind == "eps_in_sqrt":
                den = np.sqrt(v1 + S.eps) / S.bc2s
            elif kind == "eps_before_bc2":
                den = (np.sqrt(v1) + S.eps) / S.bc2s
            elif kind == "eps_missing":
                den = np.sqrt(v1) / S.bc2s
            elif kind == "bc2_unrooted":
                den = np.sqrt(v1) / (S.bc2s * S.bc2s) + S.eps
            else:
                den = np.sqrt(v1) / S.bc2s + S.eps
            k = S.lr if kind == "bc1_missing" else S.lr / S.bc1
            cw = 1.0 - S.lr * S.wd
            if kind == "coupled_decay":
                p1 = p - k * (m1 / den)
            elif kind == "decay_after_update":
                p1 = (p - k * (m1 / den)) * cw
            else:
                p1 = p * cw - k * (m1 / den)
        out = {"m": m1, "v": v1, "p": p1}
        if e is not None:
            omd = 1.0 - S.decay if kind == "omd_in_double" else S.omd
            if kind == "ema_of_old_p":
                out["e"] = e - omd * (e - p)
            elif kind == "decay_swapped":
                out["e"] = e - (1.0 - omd) * (e - p1)
            else:
                out["e"] = e - omd * (e - p1)
        return out
    step.__name__ = kind
    return step


MUTANTS = [_mutant(k) for k in (
    "eps_in_sqrt",               # 1  sqrt(v' + eps) / bc2s
    "eps_before_bc2",            # 2  (sqrt(v') + eps) / bc2s
    "eps_missing",               # 3
    "coupled_decay",             # 4  g += wd p, no decoupled decay (Adam with L2, not AdamW)
    "decay_after_update",        # 5  (p - k q) (1 - lr wd)
    "bc1_missing",               # 6
    "bc2_unrooted",              # 7  sqrt(v') / bc2
    "scale_not_in_v",            # 8  grad_scale reaches m only
    "scale_once_in_v",           # 9  v' = b2 v + c2 gs g^2
    "ema_of_old_p",              # 10
    "decay_swapped",             # 11 e - decay (e - p')
    "omd_in_double",             # 12 1.0 - decay in double (what a Python-float decay gives)
)]


# ------------------------------------------------------------------------------------------------ designated inputs
SEED = 41
Case = namedtuple("Case", "name state step lr wd grad_scale decay clip_coef")


def _cases() -> List[Case]:
    from oracle import train as otrain
    d1 = otrain.ema_decay(1)          # 2 / 11: the first update's decay, small
    return [
        Case("fresh", "fresh", 1, 1e-3, 0.01, 1.0, d1, None),
        Case("step2", "running", 2, 2e-4, 0.0, 0.5, d1, None),
        Case("step1000", "running", 1000, 1e-3, 0.01, 1.0 / 3.0, 0.9999, None),
        Case("step100000", "running", 100000, 2e-4, 0.01, 1.0, 0.9999, None),
        Case("tiny_v", "tiny_v", 1000, 1e-3, 0.0, 0.5, 0.9999, None),
        Case("clip_one", "running", 2, 1e-3, 0.01, 1.0, 0.9999, 1.0),
        Case("clip", "running", 1000, 2e-4, 0.01, 0.5, 0.9999, 0.37),
    ]


CASES = _cases()
CASE = {c.name: c for c in CASES}
CPU_N = 16384            # elements per case in the CPU tier (the GPU tier cuts its tensors from the same recipe)


def case_scalars(c: Case, **kw) -> Scalars:
    return scalars(c.step, c.lr, c.wd, c.decay, c.grad_scale, c.clip_coef, **kw)


def elements_long(c: Case, tag: str, n: int):
    """elements() for a tensor of any length (a convolution weight of the fused-pack table), drawn in pieces of at most CPU_N elements"""
    parts = [elements(c, f"{tag}.{o}", min(CPU_N, n - o)) for o in range(0, n, CPU_N)]
    return tuple(np.concatenate([q[k] for q in parts]) for k in range(5))


def elements(c: Case, tag: str, n: int):
    """-> (p, g, m, v, e) fp32 arrays of n elements, keyed by (case, tag). Magnitudes are log-uniform: |g| over 1e-10 .. 1e2, |p| over
    1e-6 .. 1. State: "fresh" m = v = 0; "running" a history magnitude h over 1e-9 .. 1e2 with m = +-h [0.1, 1], v = h^2 [0.5, 2] and half
    of the gradients near h (the other half unrelated to it); "tiny_v" v = 1e-12 m^2. Shadows: equal to p, next to p, 0.01 p, -p, or
    unrelated (a shadow far from p is what separates the fp32 and the double 1 - decay). Exact zeros by position i mod 16:
    3 g; 5 m; 7 v; 9 g, m and v (the update is exactly the decay); 11 g and v (denominator eps alone); 13 p; 15 e. Every non-zero
    intermediate stays normal: |g gs| >= 1e-11, c2 g'^2 >= 1e-25, v >= 1e-32."""
    from stedm_amd.utils import prng
    assert 0 < n < 20000
    u = prng.uniform(SEED, f"opt.{c.name}.{tag}", (12, n), 0.0, 1.0).numpy().astype(np.float64)
    sgn = lambda r: np.where(r < 0.5, -1.0, 1.0)
    g = sgn(u[1]) * 10.0 ** (-10.0 + 12.0 * u[0])
    h = 10.0 ** (-9.0 + 11.0 * u[2])
    if c.state == "fresh":
        m = np.zeros(n)
        v = np.zeros(n)
    else:
        m = sgn(u[3]) * h * (0.1 + 0.9 * u[4])
        v = h * h * (0.5 + 1.5 * u[5]) if c.state == "running" else 1e-12 * m * m
        g = np.where(u[10] < 0.5, sgn(u[1]) * h * (0.3 + 2.7 * u[0]), g)
    p = sgn(u[7]) * 10.0 ** (-6.0 + 6.0 * u[6])
    e = np.select([u[8] < 0.3, u[8] < 0.5, u[8] < 0.7, u[8] < 0.85], [p, p * (1.0 + 1e-3 * (2.0 * u[9] - 1.0)), 0.01 * p, -p],
                  sgn(u[11]) * 10.0 ** (-6.0 + 6.0 * u[9]))
    j = np.arange(n) % 16
    g = np.where((j == 3) | (j == 9) | (j == 11), 0.0, g)
    m = np.where((j == 5) | (j == 9), 0.0, m)
    v = np.where((j == 7) | (j == 9) | (j == 11), 0.0, v)
    p = np.where(j == 13, 0.0, p)
    p32 = p.astype(np.float32)
    e = np.where(u[8] < 0.3, p32.astype(np.float64), e)          # "equal to p": to the fp32 p, bit for bit
    e = np.where(j == 15, 0.0, e)
    return p32, g.astype(np.float32), m.astype(np.float32), v.astype(np.float32), e.astype(np.float32)
