"""GPU tier (-m gpu): ops.lsa_bwd16 (csrc/lsa_bwd16.hip), the LSA backward on the 16-bit matrix pipe, against torch fp64 autograd on the
SAME 16-bit planes stedm_qkv_pack wrote (read back and widened), with the keep bits of oracle.dropmask.keep_attention.

  T in {6, 66, 130, 258}: one partial tile, two past a 64 tile, two past the 128 pad, two pads plus a tail;
  heads in {1, 3}, B in {1, 2}, p in {0, 0.1}, f16 and bf16.

Bound (max-abs error over max-abs reference, per tensor): 3 x the same case's figure of the contract's fp64 emulation
(tests/refs_lsa_bwd16.py: R(s dO), R(Pd), R(dS) and nothing else) against the fp64 reference. d temperature, a single scalar whose figure
can be accidentally tiny: the largest of the case's four figures. The factor covers the hardware exp2 and another fixed summation order; a
misplaced rounding or a wrong keep bit lands far outside it. Each case prints error / figure / bound.

Measured on the MI355X: the case with the worst ratio error / bound of the 64, per tensor. Every case's error equals its emulation
figure to two or three digits (ratio 0.33): the kernel and the emulation round the same values.

    tensor error      bound      ratio  case
    dq     3.13e-03   9.35e-03   0.33   T=66 heads=3 B=2 p=0.1 bf16
    dk     4.55e-04   1.36e-03   0.33   T=258 heads=3 B=2 p=0.0 f16
    dv     3.45e-03   1.03e-02   0.33   T=258 heads=3 B=1 p=0.1 bf16
    dtemp  6.15e-04   1.84e-03   0.33   T=258 heads=1 B=1 p=0.0 f16

Against the fp32 form with the mask construction below (T = 130, p = 0.1, f16): dq 3.25e-04 / 9.77e-04, dk 3.59e-04 / 1.07e-03,
dv 2.24e-04 / 6.70e-04.

Further: two runs are bit-identical and the planes' pad rows / columns (filled with large finite values) change no bit; dO 2^-30 gives
2^-30 times the outputs bit for bit (the scale s absorbs it: no gradient is lost to fp16 subnormals); an all-zero dO gives exact zeros;
with all-ones v and one-hot dO rows (every dV element the sum of two or three kept probabilities: one wrong keep bit moves it by tens of
percent) the fp32 form and this one agree inside the bound; bad arguments raise and launch nothing."""
import math

import pytest
import torch

from tests import refs_lsa_bwd16 as E

pytestmark = pytest.mark.gpu

SEED, SITE = 0x5EED00D5, 9
LOG2E = 1.4426950408889634
TEMP = math.log(64 ** -0.5) + 0.05
QSCALE = math.exp(TEMP) * LOG2E


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from stedm_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _rng(name, shape, std=1.0):
    from stedm_amd.utils import prng
    return prng.normal(35, name, shape, std=std)


def _planes(dev, B, T, heads, mode, tag, Tp=None, ones_v=False):
    from stedm_amd import ops
    prec = ops.Precision.parse(mode)
    Tp = (T + 127) // 128 * 128 if Tp is None else Tp
    qkv = _rng(f"lsa16.qkv.{tag}", (B, T, 3 * heads * 64))
    if ones_v:
        qkv[..., 2 * heads * 64:] = 1.0
    mk = lambda shp: (torch.zeros(shp, dtype=torch.int16, device=dev), None)
    q, k, vt = mk((B * heads, Tp, 64)), mk((B * heads, Tp, 64)), mk((B * heads, 64, Tp))
    ops.qkv_pack(qkv.to(dev), QSCALE, q, k, vt, B, T, Tp, heads, prec)
    return prec, Tp, q, k, vt


def _widen(pl, mode):
    return pl[0].cpu().view(torch.float16 if mode == "f16" else torch.bfloat16).double()


def _reference(qp, kp, v, dO, keep, p):
    """fp64 autograd: qp (scaled by exp(TEMP) log2 e), kp, v, dO [BH, T, 64] -> dq (w.r.t. the unscaled q), dk, dv, d temperature"""
    q = (qp / QSCALE).detach().clone().requires_grad_(True)
    k = kp.detach().clone().requires_grad_(True)
    vv = v.detach().clone().requires_grad_(True)
    temp = torch.tensor(TEMP, dtype=torch.float64, requires_grad=True)
    with torch.enable_grad():
        dots = (q @ k.transpose(-1, -2)) * temp.exp()
        T = dots.shape[-1]
        prob = dots.masked_fill(torch.eye(T, dtype=torch.bool), -torch.finfo(dots.dtype).max).softmax(-1)
        if p > 0:
            prob = prob * (keep.double() / (1.0 - p))
        ((prob @ vv) * dO).sum().backward()
    return q.grad, k.grad, vv.grad, temp.grad.reshape(1)


def _rel(a, ref):
    return float((a.double() - ref.double()).abs().max() / ref.double().abs().max())


def _run(dev, prec, q, k, vt, dO, B, T, Tp, heads, p, fn="lsa_bwd16"):
    from stedm_amd import ops
    nan = float("nan")
    dqkv = torch.full((B * T, 3 * heads * 64), nan, device=dev)
    dtemp = torch.full((1,), nan, device=dev)
    getattr(ops, fn)(q, k, vt, dO, dqkv, dtemp, QSCALE, B, T, Tp, heads, prec, p=p, seed=SEED, site=SITE)
    torch.cuda.synchronize()
    return dqkv, dtemp


def _split(dqkv, B, T, heads):
    return dqkv.cpu().reshape(B, T, 3, heads, 64).permute(2, 0, 3, 1, 4).reshape(3, B * heads, T, 64)


def _case(dev, B, T, heads, p, mode, tag, dO, ones_v=False):
    """-> (planes, fp64 reference, the four emulation figures)"""
    from oracle import dropmask
    prec, Tp, q, k, vt = _planes(dev, B, T, heads, mode, tag, ones_v=ones_v)
    BH = B * heads
    qp, kp = _widen(q, mode)[:, :T], _widen(k, mode)[:, :T]
    v = _widen(vt, mode)[:, :, :T].transpose(1, 2)
    dOh = dO.reshape(B, T, heads, 64).permute(0, 2, 1, 3).reshape(BH, T, 64).double()
    keep = torch.from_numpy(dropmask.keep_attention(BH, T, p, SEED, SITE).copy()) if p > 0 else None
    ref = _reference(qp, kp, v, dOh, keep, p)
    emu = E.lsa_bwd16_planes(qp, kp, v, QSCALE, dOh, keep, p, mode)
    figs = [_rel(a.reshape(b.shape), b) for a, b in zip(emu, ref)]
    return (prec, Tp, q, k, vt), ref, figs


CASES = [(T, heads, B, p, mode) for T in (6, 66, 130, 258) for heads in (1, 3) for B in (1, 2) for p in (0.0, 0.1) for mode in ("f16", "bf16")]


@pytest.mark.parametrize("T,heads,B,p,mode", CASES)
def test_lsa_bwd16_against_fp64_autograd(dev, T, heads, B, p, mode):
    tag = f"{T}.{heads}.{B}"
    dO = _rng(f"lsa16.dO.{tag}", (B, T, heads * 64))
    (prec, Tp, q, k, vt), ref, figs = _case(dev, B, T, heads, p, mode, tag, dO)
    assert all(f > 0 for f in figs)
    bounds = {"dq": 3.0 * figs[0], "dk": 3.0 * figs[1], "dv": 3.0 * figs[2], "dtemp": 3.0 * max(figs)}
    dqkv, dtemp = _run(dev, prec, q, k, vt, dO.reshape(B * T, heads * 64).contiguous().to(dev), B, T, Tp, heads, p)
    assert bool(torch.isfinite(dqkv).all()) and bool(torch.isfinite(dtemp).all())
    g = _split(dqkv, B, T, heads)
    errs = {"dq": _rel(g[0], ref[0]), "dk": _rel(g[1], ref[1]), "dv": _rel(g[2], ref[2]), "dtemp": _rel(dtemp.cpu(), ref[3])}
    fg = dict(zip(("dq", "dk", "dv", "dtemp"), figs))
    print(f"lsa_bwd16 T={T} heads={heads} B={B} p={p} {mode}: " + " ".join(f"{n} {e:.2e} / {fg[n]:.2e} / {bounds[n]:.2e}" for n, e in errs.items()))
    for n, e in errs.items():
        assert e <= bounds[n], f"{n}: {e:.3e} > {bounds[n]:.3e}"


@pytest.mark.parametrize("T,p,mode", [(66, 0.1, "f16"), (130, 0.0, "bf16"), (258, 0.1, "bf16")])
def test_lsa_bwd16_deterministic_and_pad_blind(dev, T, p, mode):
    B, heads = 2, 3
    prec, Tp, q, k, vt = _planes(dev, B, T, heads, mode, f"det.{T}")
    dO = _rng(f"lsa16.dO.det.{T}", (B * T, heads * 64)).to(dev)
    a = _run(dev, prec, q, k, vt, dO, B, T, Tp, heads, p)
    b = _run(dev, prec, q, k, vt, dO, B, T, Tp, heads, p)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "two runs differ"
    big = 0x7BFF if mode == "f16" else 0x7F00      # 65504 (f16) / 2^127 (bf16): large and finite
    q[0][:, T:, :] = big
    k[0][:, T:, :] = big
    vt[0][:, :, T:] = big
    c = _run(dev, prec, q, k, vt, dO, B, T, Tp, heads, p)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]), "the pad rows / columns of the planes influence the result"


@pytest.mark.parametrize("mode", ["f16", "bf16"])
def test_lsa_bwd16_scale_exact(dev, mode):
    B, heads, T, p = 2, 3, 66, 0.1
    prec, Tp, q, k, vt = _planes(dev, B, T, heads, mode, "scale")
    dO = _rng("lsa16.dO.scale", (B * T, heads * 64)).to(dev)
    a = _run(dev, prec, q, k, vt, dO, B, T, Tp, heads, p)
    b = _run(dev, prec, q, k, vt, dO * 2.0 ** -30, B, T, Tp, heads, p)
    assert float(a[0].abs().max()) > 0
    assert torch.equal(a[0] * 2.0 ** -30, b[0]) and torch.equal(a[1] * 2.0 ** -30, b[1])


@pytest.mark.parametrize("mode,p", [("f16", 0.1), ("bf16", 0.0)])
def test_lsa_bwd16_zero_dO(dev, mode, p):
    B, heads, T = 2, 3, 66
    prec, Tp, q, k, vt = _planes(dev, B, T, heads, mode, "zero")
    dqkv, dtemp = _run(dev, prec, q, k, vt, torch.zeros((B * T, heads * 64), device=dev), B, T, Tp, heads, p)
    assert bool((dqkv == 0).all()) and bool((dtemp == 0).all())


@pytest.mark.parametrize("mode", ["f16"])
def test_lsa_bwd16_same_mask_as_the_fp32_form(dev, mode):
    B, heads, T, p = 2, 3, 130, 0.1
    dO = torch.zeros(B, T, heads, 64)
    dO[:, torch.arange(T), :, torch.arange(T) % 64] = 1.0            # one-hot rows: channel i % 64 of query i
    dO = dO.reshape(B, T, heads * 64)
    (prec, Tp, q, k, vt), ref, figs = _case(dev, B, T, heads, p, mode, "mask", dO, ones_v=True)
    dOd = dO.reshape(B * T, heads * 64).contiguous().to(dev)
    a = _run(dev, prec, q, k, vt, dOd, B, T, Tp, heads, p, fn="lsa_bwd")
    b = _run(dev, prec, q, k, vt, dOd, B, T, Tp, heads, p)
    ga, gb = _split(a[0], B, T, heads), _split(b[0], B, T, heads)
    for i, n in enumerate(("dq", "dk", "dv")):
        e = _rel(gb[i], ga[i])
        print(f"lsa_bwd16 against lsa_bwd {n}: {e:.2e} / {3.0 * figs[i]:.2e}")
        assert e <= 3.0 * figs[i], f"{n}: {e:.3e} > {3.0 * figs[i]:.3e}"
    assert _rel(b[1].cpu(), a[1].cpu()) <= 3.0 * max(figs)


def test_lsa_bwd16_argument_errors_launch_nothing(dev):
    from stedm_amd import ops
    from stedm_amd._lib import StedmHipError
    prec = ops.Precision.parse("f16")
    B, heads = 1, 1
    nan = float("nan")

    def attempt(T, Tp, off=0):
        mk = lambda shp: torch.zeros(shp, dtype=torch.int16, device=dev)
        q, k, vt = mk((B * heads, Tp, 64)), mk((B * heads, Tp, 64)), mk((B * heads, 64, Tp))
        n = B * T * heads * 64
        dO = torch.ones((n + 4,), device=dev)[off:off + n]
        dqkv = torch.full((B * T, 3 * heads * 64), nan, device=dev)
        dtemp = torch.full((1,), nan, device=dev)
        ws = torch.zeros((1 << 20,), dtype=torch.uint8, device=dev)
        with pytest.raises(StedmHipError):
            ops.lsa_bwd16(q, k, vt, dO, dqkv, dtemp, QSCALE, B, T, Tp, heads, prec, ws=ws)
        torch.cuda.synchronize()
        assert bool(torch.isnan(dqkv).all()) and bool(torch.isnan(dtemp).all()) and int(ws.sum()) == 0

    attempt(1, 128)            # T = 1: no key but the masked diagonal
    attempt(6, 64)             # Tp % 128 != 0
    attempt(6, 128, off=1)     # d_out 4 bytes off a 16-byte boundary
