"""An fp32 restatement of the DDIM update (stedm_ddim_step, stedm_ddim_step_ex, stedm_ddim_step_rows; sampler.hip) that reproduces the
kernel's bits: every operation is rounded where the kernel rounds it, every fused multiply-add is one rounding, and the sums of the
rescale statistic run in the kernel's order. Written in numpy from the kernel's description; nothing of stedm_amd is imported. Shared by
tests/test_ddim_refs_cpu.py (pins fma32 against rational arithmetic and the restatement against oracle/ddim.py) and
tests/test_gpu_ddim_exact.py (pins the kernels against the restatement with torch.equal).

The restatement's parameters are a `Form`:
  parts  the number of threads that share a column. Thread (col, part) sums its rows r = part, part + parts, ... of the C H rows
         sequentially from 0.0; the column total is the sequential sum of the partial sums over part = 0 .. parts - 1. The scalar entries
         run 256 // W parts (scalar_form), the per-row entry 16 (ROWS). (`cols`, the number of columns a workgroup holds - W or 16 - is
         kept for the record: columns are independent, so it does not enter the arithmetic.)
  fused  the guided combine e = (e_w ratio) phi + (1 - phi) e_c: False - both products rounded, then the sum (the scalar entries);
         True - fma(e_w ratio, phi, (1 - phi) e_c) (the per-row entry).
  dir_fused  dir = sqrt(1 - a_prev - sigma^2): True - sqrt(fma(-sigma, sigma, 1 - a_prev)) (the scalar entries); False - sigma sigma
         rounded, then subtracted from 1 - a_prev (the per-row entry). One value per launch; the two agree whenever sigma = 0.
  swap01 the centred squares of a thread's FIRST TWO rows enter in swapped order, q = fma(d0, d0, d1 d1) instead of fma(d1, d1, d0 d0):
         True in the register-held forms of the scalar entries (R = 4, 8, 16 rows per thread), the pairing their squares pass has always
         had; False in the looped scalar form and everywhere in the per-row entry.
Everything else is common:
  e_w   = fma(s, e_c - e_u, e_u)
  mean  = total / CH;  q = fma(d, d, q) over the same rows with d = value - mean;  ratio = sqrt(vc / (CH - 1)) / sqrt(vw / (CH - 1))
  x0    = fma(-sq1m, e, x) / sqrt(a_t)
  base  = sqrt(a_prev) x0 + dir e, both products rounded, then the sum
  noise : x_prev = fma(sigma, z, base);  with the options (temperature, dropout, eps_out or noise_out of stedm_ddim_step_ex)
          x_prev = base + ((sigma z) T) ks, every operation rounded
The divisions and square roots are IEEE (correctly rounded), which numpy's float32 gives.
A sequence of scales selects the per-row semantics: row b with scales[b] == 1 (or e_u None) is unguided, e = e_c."""
from collections import namedtuple

import numpy as np
import torch

F32 = np.float32
Form = namedtuple("Form", "parts cols fused dir_fused swap01")
ROWS = Form(16, 16, True, False, False)


def scalar_form(CH, W):
    """the form of stedm_ddim_step / stedm_ddim_step_ex for C H rows of width W: register-held when the 256 threads tile the sample
    exactly with 4, 8 or 16 rows each, looped otherwise"""
    parts = 256 // W
    reg = 256 % W == 0 and CH % parts == 0 and CH // parts in (4, 8, 16)
    return Form(parts, W, False, True, reg)


def fma32(a, b, c):
    """fl32(a b + c) with ONE rounding, for float32 arrays: the product is exact in float64 (48 bits); TwoSum gives the float64 sum and its
    exact residual; where the residual is not zero the sum is moved to the neighbour with an odd last bit (round to odd), which float32's
    24 bits then round as they would round the exact value (53 >= 24 + 2). Finite values away from float64's range limits only."""
    a, b, c = (np.asarray(v, dtype=F32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where((err != 0) & even, np.nextafter(s, toward), s)
    return s.astype(F32)


def _column_stat(v, parts, mean=None, swap01=False):
    """v [B][CH][W] fp32 -> the column totals [B][W] in the kernel's order: sums of v (mean None) or of (v - mean)^2 by fma"""
    B, CH, W = v.shape
    per = -(-CH // parts)
    acc = np.zeros((B, parts, W), dtype=F32)
    for j in ([1, 0] + list(range(2, per)) if swap01 and mean is not None else range(per)):
        rows = v[:, j * parts:(j + 1) * parts]
        n = rows.shape[1]                                   # the last round may hold fewer than `parts` rows: those parts skip it
        if mean is None:
            acc[:, :n] = acc[:, :n] + rows
        else:
            d = rows - mean[:, None, :]
            acc[:, :n] = fma32(d, d, acc[:, :n])
    tot = np.zeros((B, W), dtype=F32)
    for p in range(parts):
        tot = tot + acc[:, p]
    return tot


def guided_eps(e_c, e_u, s, phi, form):
    """[B][CH][W] fp32, one scale: the rescaled classifier-free combine (ddim.py:179-184) in the kernel's arithmetic"""
    CH = e_c.shape[1]
    s, phi = F32(s), F32(phi)
    ew = fma32(s, e_c - e_u, e_u)
    n, n1 = F32(CH), F32(CH - 1)
    mc = _column_stat(e_c, form.parts) / n
    mw = _column_stat(ew, form.parts) / n
    vc = _column_stat(e_c, form.parts, mc, form.swap01)
    vw = _column_stat(ew, form.parts, mw, form.swap01)
    ratio = (np.sqrt(vc / n1) / np.sqrt(vw / n1))[:, None, :]
    keep = (F32(1.0) - phi) * e_c
    if form.fused:
        return fma32(ew * ratio, phi, keep)
    return (ew * ratio) * phi + keep


def ddim_step_ref(x, e_c, e_u, row, scale, form, phi=0.7, noise=None, ext=None):
    """x, e_c, e_u (or None), noise (or None): torch fp32 [B, C, H, W] on the CPU; row = (a_t, a_prev, sigma, sq1m), the table row the kernel
    reads; scale: a float (the scalar entries: guided whenever e_u is given) or a sequence of B floats (the per-row entry).
    ext: None, or dict(temperature, ks) for the options path of stedm_ddim_step_ex, ks a [B, C, H, W] fp32 tensor of keep * drop_scale
    (None: 1). Returns (x_prev, pred_x0, eps) as torch fp32 tensors."""
    B, C, H, W = x.shape
    r3 = lambda t: t.detach().cpu().numpy().astype(F32).reshape(B, C * H, W)
    xv, ec = r3(x), r3(e_c)
    a_t, a_prev, sigma, sq1m = (F32(v) for v in row)
    e = ec.copy()
    if e_u is not None:
        eu = r3(e_u)
        if np.ndim(scale) == 0:
            e = guided_eps(ec, eu, scale, phi, form)
        else:
            assert len(scale) == B
            for b, s in enumerate(scale):
                if F32(s) != F32(1.0):
                    e[b:b + 1] = guided_eps(ec[b:b + 1], eu[b:b + 1], s, phi, form)
    x0 = fma32(-sq1m, e, xv) / np.sqrt(a_t)
    dir_c = np.sqrt(fma32(-sigma, sigma, F32(1.0) - a_prev) if form.dir_fused else (F32(1.0) - a_prev) - sigma * sigma)
    xp = np.sqrt(a_prev) * x0 + dir_c * e
    if noise is not None:
        z = r3(noise)
        if ext is None:
            xp = fma32(sigma, z, xp)
        else:
            ks = F32(1.0) if ext.get("ks") is None else r3(ext["ks"])
            xp = xp + ((sigma * z) * F32(ext["temperature"])) * ks
    out = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=F32)).view(B, C, H, W)
    return out(xp), out(x0), out(e)
