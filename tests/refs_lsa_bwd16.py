"""The numerics contract of stedm_lsa_bwd16 (csrc/lsa_bwd16.hip) written out in fp64 torch: refs_svit_bwd.lsa_bwd with exactly three
roundings R (round to nearest even into the mode's 16-bit format):

    dOr = R(s dO)               s: one power of two per call from amax |dO| (`do_scale`), divided out of the outputs exactly
    Pd  = R(P keep / (1 - p))   operand of dV = Pd^T dOr
    dS  = R(dS)                 operand of dQ = dS K and dK = dS^T Q

Everything else stays unrounded: the statistics and D come from the unrounded P and dP, d temperature from the unrounded dS."""
import math

import torch

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453


def R(x: torch.Tensor, mode: str) -> torch.Tensor:
    if mode == "f16":
        return x.float().half().to(x.dtype)
    if mode == "bf16":
        return x.float().bfloat16().to(x.dtype)
    raise ValueError(mode)


def do_scale(d_att: torch.Tensor) -> float:
    """s = 2^(clamp(264 - e, 1, 253) - 127), e the biased fp32 exponent of amax |dO|: s amax in [2^10, 2^11). amax == 0: 1."""
    amax = float(d_att.float().abs().max())
    if amax == 0.0:
        return 1.0
    e = max(math.frexp(amax)[1] - 1 + 127, 0)
    return 2.0 ** (min(max(264 - e, 1), 253) - 127)


def lsa_bwd16_planes(qp, k, v, qscale: float, d_att, keep, p: float, mode: str):
    """qp [.., T, 64]: the forward's q plane (q exp(temperature) log2 e, 16-bit values), k, v [.., T, 64] 16-bit values, d_att [.., T, 64]
    -> dq (with respect to the unscaled q), dk, dv, d temperature; all fp64."""
    qp, k, v, d_att = qp.double(), k.double(), v.double(), d_att.double()
    T = qp.shape[-2]
    s = do_scale(d_att)
    dor = R(d_att * s, mode)
    x = qp @ k.transpose(-1, -2)                                           # log2-domain logits
    eye = torch.eye(T, dtype=torch.bool)
    xm = x.masked_fill(eye, -torch.finfo(x.dtype).max)
    e = torch.exp2(xm - xm.max(-1, keepdim=True).values)
    prob = (e / e.sum(-1, keepdim=True)).masked_fill(eye, 0.0)
    ks = torch.ones_like(prob) if keep is None or p <= 0 else keep.to(prob.dtype) / (1.0 - p)
    pd = prob * ks
    dpd = dor @ v.transpose(-1, -2)
    D = (pd * dpd).sum(-1, keepdim=True)
    dS = (prob * (ks * dpd - D)).masked_fill(eye, 0.0)
    dv = R(pd, mode).transpose(-1, -2) @ dor / s
    dSr = R(dS, mode)
    dq = dSr @ k * (qscale * LN2) / s
    dk = dSr.transpose(-1, -2) @ qp * LN2 / s
    dtemp = (dS * x.masked_fill(eye, 0.0)).sum() * LN2 / s
    return dq, dk, dv, dtemp


def lsa_bwd16(q, k, v, temperature, d_att, keep=None, p: float = 0.0, mode: str = "f16"):
    """refs_svit_bwd.lsa_bwd's signature (unscaled, unrounded q, k, v): the planes are rounded as the forward's pack rounds them."""
    qscale = float(temperature.exp()) * LOG2E
    return lsa_bwd16_planes(R(q.double() * qscale, mode), R(k.double(), mode), R(v.double(), mode), qscale, d_att, keep, p, mode)
