"""CPU tier: the exact DDIM restatement of tests/refs_ddim.py. fma32 is pinned against rational arithmetic (ties and near-ties included:
one wrong rounding there would make the GPU tier's torch.equal meaningless), and the restatement against oracle/ddim.py's cfg_combine /
ddim_update in both geometries and both combine spellings, at the tolerance tests/test_gpu_ddim_rows.py holds the kernel to."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import ddim as od
from stedm_amd.utils import prng
from tests import refs_ddim as rd
from tests.test_ddim_options_oracle import ddim_update_opts, drop_scale, keep_mask
from tests.test_gpu_kernels import rel_err

torch.set_grad_enabled(False)
F32 = np.float32


def _round_f32(fr: Fraction) -> float:
    """a rational in float32's normal range -> the nearest float32, ties to even, in integer arithmetic"""
    if fr == 0:
        return 0.0
    sign, fr = (-1.0 if fr < 0 else 1.0), abs(fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    if Fraction(2) ** e > fr:
        e -= 1                                             # 2^e <= fr < 2^(e + 1)
    assert -126 <= e < 127
    q = fr / Fraction(2) ** (e - 23)                       # 2^23 <= q < 2^24
    m, rest = divmod(q.numerator, q.denominator)
    twice = 2 * rest
    if twice > q.denominator or (twice == q.denominator and m & 1):
        m += 1
    return sign * float(m) * 2.0 ** (e - 23)               # m <= 2^24: exact in float64


def _tie_triples(g, n):
    """a b + c on or next to a float32 tie of c's binade: a b = +-half an ulp of c times 1 (an exact tie), 1 - 2^-40 (just below: a float64
    sum rounds it ONTO the tie) or 1 + 2^-19 + 2^-40 (just above, with a bit a float64 sum drops)"""
    c = (g.standard_normal(n) * 8).astype(F32)
    c[c == 0] = F32(1.0)
    half = (np.spacing(np.abs(c)) / 2).astype(F32)         # a power of two
    kind = g.integers(0, 3, n)
    lo, hi = F32(1.0 - 2.0 ** -20), F32(1.0 + 2.0 ** -20)
    a = np.where(kind == 0, F32(1.0), hi).astype(F32)
    b = (np.where(kind == 0, F32(1.0), np.where(kind == 1, lo, hi)) * half).astype(F32)
    sh = g.integers(-8, 9, n)
    a, b = np.ldexp(a, sh).astype(F32), np.ldexp(b, -sh).astype(F32)
    return a, (b * g.choice(np.array([-1.0, 1.0], dtype=F32), n)).astype(F32), c


def test_fma32_equals_rational_arithmetic():
    g = np.random.default_rng(20260)
    n = 10000
    a = (g.standard_normal(n) * np.exp2(g.integers(-6, 7, n))).astype(F32)
    b = (g.standard_normal(n) * np.exp2(g.integers(-6, 7, n))).astype(F32)
    c = (-(a.astype(np.float64) * b) * (1 + g.standard_normal(n) * np.exp2(-g.integers(0, 30, n).astype(np.float64)))).astype(F32)   # cancellation
    c[::2] = (g.standard_normal(n // 2) * 4).astype(F32)
    ta, tb, tc = _tie_triples(g, n)
    a, b, c = np.concatenate([a, ta]), np.concatenate([b, tb]), np.concatenate([c, tc])
    got = rd.fma32(a, b, c)
    assert got.dtype == F32
    naive_wrong = 0
    for i in range(2 * n):
        want = _round_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert float(got[i]) == want, (i, float(a[i]), float(b[i]), float(c[i]), float(got[i]), want)
        naive_wrong += float(F32(float(a[i]) * float(b[i]) + float(c[i]))) != want
    assert naive_wrong > 100          # the cases do tell a double rounding through float64 from one rounding


def _operands(shape, seed=7):
    x = prng.normal(seed, "dd.x", shape)
    ec = prng.normal(seed, "dd.ec", shape)
    eu = prng.normal(seed, "dd.eu", shape) * 0.8 + 0.1 * ec
    nz = prng.normal(seed, "dd.nz", shape)
    return x, ec, eu, nz


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("family", ["scalar", "rows"])
@pytest.mark.parametrize("shape", [(2, 4, 16, 16), (2, 3, 40, 40), (5, 4, 8, 8)])
def test_restatement_matches_the_oracle(shape, family, fused):
    x, ec, eu, nz = _operands(shape)
    form = (rd.scalar_form(shape[1] * shape[2], shape[3]) if family == "scalar" else rd.ROWS)._replace(fused=fused)
    for eta in (0.0, 1.0):
        ds = od.DDIMSchedule(od.Schedule(), 20, eta)
        row = ds.scalars(10)
        noise = nz if eta else None
        for e_u, s in ((None, 1.0), (eu, 1.5), (eu, 5.0)):
            xp, x0, e = rd.ddim_step_ref(x, ec, e_u, row, s, form, noise=noise)
            e_ref = ec if e_u is None else od.cfg_combine(ec, eu, s)
            xp_ref, x0_ref = od.ddim_update(x, e_ref, *row, noise=noise)
            errs = rel_err(e, e_ref), rel_err(x0, x0_ref), rel_err(xp, xp_ref)
            assert max(errs) < 2e-5, (eta, s, errs)


def test_per_row_scales_and_the_options_path():
    shape = (5, 4, 8, 8)
    x, ec, eu, nz = _operands(shape)
    scales = [1.0, 3.0, 5.0, 1.5, 7.5]
    ds = od.DDIMSchedule(od.Schedule(), 20, 1.0)
    row = ds.scalars(10)
    xp, x0, e = rd.ddim_step_ref(x, ec, eu, row, scales, rd.ROWS, noise=nz)
    assert torch.equal(e[0], ec[0])                        # the scale-1 row is the unguided update: e_u does not enter
    for b, s in enumerate(scales):
        r = slice(b, b + 1)
        one = rd.ddim_step_ref(x[r], ec[r], None if s == 1.0 else eu[r], row, s, rd.ROWS, noise=nz[r])
        assert torch.equal(xp[r], one[0]) and torch.equal(x0[r], one[1])
        e_ref = ec[r] if s == 1.0 else od.cfg_combine(ec[r], eu[r], s)
        xp_ref, _ = od.ddim_update(x[r], e_ref, *row, noise=nz[r])
        assert rel_err(xp[r], xp_ref) < 2e-5
    # temperature and dropout: every operation of the noise term rounded, as the oracle's torch expression does
    T, p = 0.7, 0.25
    keep = torch.from_numpy(keep_mask(3, range(5), 4 * 8 * 8, 9, p)).view(shape)
    ks = keep.float() * drop_scale(p)
    form = rd.scalar_form(4 * 8, 8)
    got, _, e = rd.ddim_step_ref(x, ec, eu, row, 1.5, form, noise=nz, ext=dict(temperature=T, ks=ks))
    ref, _ = ddim_update_opts(x, od.cfg_combine(ec, eu, 1.5), *row, noise=nz, temperature=T, keep=keep, p=p)
    assert rel_err(got, ref) < 2e-5
    base, _, _ = rd.ddim_step_ref(x, ec, eu, row, 1.5, form)
    sigma = torch.tensor(row[2])
    assert torch.equal(got, base + ((sigma * nz) * T) * ks)
