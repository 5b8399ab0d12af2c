"""GPU tier (-m gpu): ops.lsa_bwd (csrc/svit_bwd.hip) against torch fp64 autograd on the SAME 16-bit-rounded q / k / v: the planes
stedm_qkv_pack wrote are read back, widened (hi, or hi + lo) and differentiated in fp64.

  T in {6, 66, 130, 258}: one partial tile, two past a 64-row tile, two past the 128-row pad, two pads plus a tail;
  heads in {1, 3}, B in {1, 2}, p in {0, 0.1}, hi-only (f16, one product) and hi + lo (parity) planes.

Bound (max-abs error over max-abs reference, per tensor): 8 x the case's fp32-against-fp64 figure - the same function differentiated by
torch autograd in fp32 and in fp64 on the CPU. dq, dk, dv: the tensor's own figure. d temperature, a single scalar whose fp32 error can be
accidentally tiny: the largest figure of the case's four tensors. The factor covers the hardware exp2 and a different but fixed summation
order. Each case prints its errors, its figures and its bounds.

Measured on the MI355X: the case with the worst ratio error / bound of the 64, per tensor

    tensor error      bound      ratio  case
    dq     7.40e-07   3.55e-06   0.21   T=130 heads=3 B=2 p=0.1 f16
    dk     9.91e-07   4.13e-06   0.24   T=130 heads=3 B=2 p=0.1 f16
    dv     2.34e-07   7.31e-07   0.32   T=6 heads=1 B=2 p=0.0 f16
    dtemp  8.95e-07   1.90e-06   0.47   T=6 heads=1 B=2 p=0.1 f16

A first form that summed d temperature in fp32 and took the probabilities
from exp2(s - LSE) missed the d temperature bound at T = 130 (9.0e-06 against 4.8e-06): the sum cancels (every row of dS sums to zero) and is carried in
fp64 now, and P = exp2(s - max) / sum keeps the exponential's relative accuracy.

Two runs are bit-identical; rows / columns >= T of the padded planes, filled with large finite values, do not change a bit."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED, SITE = 0x5EED00D5, 9
LOG2E = 1.4426950408889634
TEMP = math.log(64 ** -0.5) + 0.05


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stedm_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _rng(name, shape, std=1.0):
    from stedm_amd.utils import prng
    return prng.normal(34, name, shape, std=std)


def _planes(dev, B, T, heads, mode, tag):
    """qkv rows -> the forward's operand planes (stedm_qkv_pack), as the encoder's forward builds them"""
    from stedm_amd import ops
    prec = ops.Precision.parse(mode)
    Tp = (T + 127) // 128 * 128
    qkv = _rng(f"lsa.qkv.{tag}", (B, T, 3 * heads * 64)).to(dev)
    lo = prec.npass == 3
    mk = lambda shp: (torch.zeros(shp, dtype=torch.int16, device=dev), torch.zeros(shp, dtype=torch.int16, device=dev) if lo else None)
    q, k, vt = mk((B * heads, Tp, 64)), mk((B * heads, Tp, 64)), mk((B * heads, 64, Tp))
    qscale = math.exp(TEMP) * LOG2E
    ops.qkv_pack(qkv, qscale, q, k, vt, B, T, Tp, heads, prec)
    return prec, Tp, qscale, q, k, vt


def _widen(pl):
    f = lambda t: t.cpu().view(torch.float16).double()
    return f(pl[0]) + (f(pl[1]) if pl[1] is not None else 0.0)


def _reference(qp, kp, v, dO, keep, p, dtype):
    """qp (scaled by exp(TEMP) log2 e), kp, v [BH, T, 64]; dO [BH, T, 64] -> dq (w.r.t. the unscaled q), dk, dv, d temperature by autograd"""
    qscale = math.exp(TEMP) * LOG2E
    q = (qp / qscale).to(dtype).detach().clone().requires_grad_(True)
    k = kp.to(dtype).detach().clone().requires_grad_(True)
    vv = v.to(dtype).detach().clone().requires_grad_(True)
    temp = torch.tensor(TEMP, dtype=dtype, requires_grad=True)
    with torch.enable_grad():
        dots = (q @ k.transpose(-1, -2)) * temp.exp()
        T = dots.shape[-1]
        dots = dots.masked_fill(torch.eye(T, dtype=torch.bool), -torch.finfo(dots.dtype).max)
        prob = dots.softmax(-1)
        if p > 0:
            prob = prob * (keep.to(dtype) / (1.0 - p))
        ((prob @ vv) * dO.to(dtype)).sum().backward()
    return q.grad, k.grad, vv.grad, temp.grad.reshape(1)


def _rel(a, ref):
    return float((a.double() - ref.double()).abs().max() / ref.double().abs().max())


def _run(dev, prec, q, k, vt, dO, qscale, B, T, Tp, heads, p):
    from stedm_amd import ops
    nan = float("nan")
    dqkv = torch.full((B * T, 3 * heads * 64), nan, device=dev)
    dtemp = torch.full((1,), nan, device=dev)
    ops.lsa_bwd(q, k, vt, dO, dqkv, dtemp, qscale, B, T, Tp, heads, prec, p=p, seed=SEED, site=SITE)
    torch.cuda.synchronize()
    return dqkv, dtemp


CASES = [(T, heads, B, p, mode) for T in (6, 66, 130, 258) for heads in (1, 3) for B in (1, 2) for p in (0.0, 0.1) for mode in ("f16", "parity")]


@pytest.mark.parametrize("T,heads,B,p,mode", CASES)
def test_lsa_bwd_against_fp64_autograd(dev, T, heads, B, p, mode):
    from oracle import dropmask
    tag = f"{T}.{heads}.{B}"
    prec, Tp, qscale, q, k, vt = _planes(dev, B, T, heads, mode, tag)
    BH = B * heads
    dO = _rng(f"lsa.dO.{tag}", (B, T, heads * 64))
    qp, kp = _widen(q)[:, :T], _widen(k)[:, :T]
    v = _widen(vt)[:, :, :T].transpose(1, 2)
    dOh = dO.reshape(B, T, heads, 64).permute(0, 2, 1, 3).reshape(BH, T, 64).double()
    keep = torch.from_numpy(dropmask.keep_attention(BH, T, p, SEED, SITE).copy()) if p > 0 else None
    ref = _reference(qp, kp, v, dOh, keep, p, torch.float64)
    r32 = _reference(qp, kp, v, dOh, keep, p, torch.float32)
    figs = [_rel(a, b) for a, b in zip(r32, ref)]              # the case's fp32-against-fp64 figures: dq, dk, dv, d temperature
    bounds = {"dq": 8.0 * figs[0], "dk": 8.0 * figs[1], "dv": 8.0 * figs[2], "dtemp": 8.0 * max(figs)}
    dqkv, dtemp = _run(dev, prec, q, k, vt, dO.reshape(B * T, heads * 64).contiguous().to(dev), qscale, B, T, Tp, heads, p)
    assert bool(torch.isfinite(dqkv).all()) and bool(torch.isfinite(dtemp).all())
    g = dqkv.cpu().reshape(B, T, 3, heads, 64).permute(2, 0, 3, 1, 4).reshape(3, BH, T, 64)
    errs = {"dq": _rel(g[0], ref[0]), "dk": _rel(g[1], ref[1]), "dv": _rel(g[2], ref[2]), "dtemp": _rel(dtemp.cpu(), ref[3])}
    print(f"lsa_bwd T={T} heads={heads} B={B} p={p} {mode}: " + " ".join(f"{n} {e:.2e} / {bounds[n]:.2e}" for n, e in errs.items()))
    for n, e in errs.items():
        assert e <= bounds[n], f"{n}: {e:.3e} > {bounds[n]:.3e}"


@pytest.mark.parametrize("T,p,mode", [(66, 0.1, "f16"), (130, 0.0, "parity"), (258, 0.1, "parity")])
def test_lsa_bwd_deterministic_and_pad_blind(dev, T, p, mode):
    B, heads = 2, 3
    prec, Tp, qscale, q, k, vt = _planes(dev, B, T, heads, mode, f"det.{T}")
    dO = _rng(f"lsa.dO.det.{T}", (B * T, heads * 64)).to(dev)
    a = _run(dev, prec, q, k, vt, dO, qscale, B, T, Tp, heads, p)
    b = _run(dev, prec, q, k, vt, dO, qscale, B, T, Tp, heads, p)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "two runs differ"
    big = 0x7BFF      # 65504 as fp16 bits: large and finite
    for pl in (q, k):
        for t in pl:
            if t is not None:
                t[:, T:, :] = big
    for t in vt:
        if t is not None:
            t[:, :, T:] = big
    c = _run(dev, prec, q, k, vt, dO, qscale, B, T, Tp, heads, p)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]), "the pad rows / columns of the planes influence the result"
