"""Plain torch restatement of stedm_gn_apply16c_resample (stedm_amd/csrc/resample.hip; include/stedm_hip.h), the front of ResBlock(up / down):
GroupNorm + activation of x [B][H][W][C], resampled 2 x 2 into 16-bit planes, and the same resampling of raw x. On top of tests/refs_gn.py
(statistics, apply-tier bound) and tests/refs_resample.py (the pool's order of additions, the replicate). No GPU. Pinned against
F.avg_pool2d(F.silu(F.group_norm(x))) / F.interpolate in tests/test_updown_refs_cpu.py; tests/test_gpu_updown_kernel.py holds the kernel to it.

The pass, per source element and in the inputs' dtype (fp32: the kernel's order; fp64: the reference):
  a = act((x - m) * (r * gamma) + beta), m / r = {mean, rstd} of the element's (sample, group), GIVEN       (the 8-wide apply kernel's order)
  mode 1 (pool):    y = 0.25 * (((a00 + a01) + a10) + a11), xr the same expression on x
  mode 2 (nearest): y = a at the four positions (2y + dy, 2x + dx), xr = x there

BOUND of a stored pool value against the fp64 restatement on the same statistics (apply tier of refs_gn), derived:
  each of the four a carries the apply tier's PRE-rounding bound E_k (refs_gn.apply_bound without its final-rounding terms);
  the three additions are a recursive sum of four computed terms: |fl(sum) - sum a| <= sum E_k + gamma_3 (sum |a_k| + sum E_k); the quarter
  is exact. So E_pool = mean(E_k) (1 + gamma_3) + gamma_3 mean|a_k|;
  final rounding to T: u_T (|y| + E_pool) + the format's floor; hi + lo: u_T^2 (|y| + E_pool) + the floor (refs_gn's split residual).
The nearest mode stores the apply kernel's own value four times: refs_gn.apply_bound as it stands."""
import torch

from tests import refs_bwd as RB
from tests import refs_gn as G
from tests import refs_resample as RS

POOL, NEAREST = 1, 2

# (B, H, W, C, groups) of x. Pool: one output row / one octet; odd batch, non-square, groups of 3 channels that cut an octet; several
# channel blocks (C = 1024); the input's statistics in five 256-pixel slots (40 x 32); a ragged last slot (18 x 16 = 288 pixels)
POOL_CASES = [(2, 4, 4, 32, 8), (1, 2, 2, 8, 2), (3, 6, 10, 96, 32), (2, 4, 4, 1024, 32), (2, 40, 32, 64, 32), (1, 18, 16, 16, 4)]
# Nearest: odd sides (3 x 5); 320 input pixels: a ragged second slot; one pixel of one octet; several channel blocks
NEAREST_CASES = [(2, 4, 4, 32, 8), (3, 3, 5, 96, 32), (2, 20, 16, 64, 32), (1, 1, 1, 8, 2), (2, 2, 2, 1024, 32)]


def case_id(c):
    return "x".join(str(v) for v in c[:4])


def inputs(case, seed=0):
    """x [B, H, W, C], gamma, beta (fp32) in the distributions of refs_gn.fwd_inputs"""
    B, H, W, C, groups = case
    s = RB.case_seed("updown" + case_id(case)) + seed
    return (G.normal((B, H, W, C), s, "x", 1.7, 0.3), G.normal((C,), s, "gamma", 0.3, 1.0), G.normal((C,), s, "beta", 0.2))


def affine_act(x, mr, groups, gamma, beta, act):
    """a [B, H, W, C] in x's dtype: act((x - m) * (r * gamma) + beta) with the statistics mr [B, groups, 2] given"""
    B, H, W, C = x.shape
    mr = mr.to(x.dtype)
    m = G.per_channel(mr[..., 0], C).view(B, 1, 1, C)
    r = G.per_channel(mr[..., 1], C).view(B, 1, 1, C)
    a = (x - m) * (r * gamma.to(x.dtype)) + beta.to(x.dtype)
    return RB.silu(a) if act else a


def resample(v, mode):
    return RS.avgpool2x2(v) if mode == POOL else RS.replicate2x2(v)


def gn_resample(x, mr, groups, gamma, beta, act, mode):
    """(y, xr) of the pass in x's dtype, before the 16-bit split"""
    return resample(affine_act(x, mr, groups, gamma, beta, act), mode), resample(x, mode)


def planes(y32, dtype, hilo):
    """the int16 words of the planes: hi = T(y), lo = T(y - hi) (refs_gn._split)"""
    return G._split(y32, dtype, hilo)


def pre_bound(x64, mr64, groups, gamma64, beta64, act):
    """(a, E): the fp64 value of the activation [B, H, W, C] and the apply tier's bound of the kernel's fp32 value BEFORE the 16-bit rounding
    (the lines of refs_gn.apply_bound up to its final-rounding terms, statistics given)"""
    B, H, W, C = x64.shape
    mean = G.per_channel(mr64[..., 0], C).view(B, 1, 1, C)
    rstd = G.per_channel(mr64[..., 1], C).view(B, 1, 1, C)
    D = (x64 - mean).abs()
    ypre = (x64 - mean) * rstd * gamma64 + beta64
    E = gamma64.abs() * rstd * (G.U * mean.abs() + 4.0 * G.U * D) * (1.0 + 8.0 * G.U) + G.U * ypre.abs()
    y = ypre
    if act:
        y = RB.silu(ypre)
        E = 1.1 * E + RB.silu_bound(ypre.abs() + E, y.abs() + 1.1 * E)
    return y, E


def pool_bound(x64, mr64, groups, gamma64, beta64, act, dtype, hilo):
    """(y, bound) [B, H/2, W/2, C] of the pool mode's stored value (module docstring)"""
    a, E = pre_bound(x64, mr64, groups, gamma64, beta64, act)
    y = RS.avgpool2x2(a)
    Ep = RS.avgpool2x2(E) * (1.0 + G.gam(3)) + G.gam(3) * RS.avgpool2x2(a.abs())
    ut = G.u_T(dtype)
    return y, Ep + (ut * ut if hilo else ut) * (y.abs() + Ep) + G.floor_T(dtype) + G.TINY


def nearest_bound(x64, mr64, groups, gamma64, beta64, act, dtype, hilo):
    B, H, W, C = x64.shape
    a, _ = pre_bound(x64, mr64, groups, gamma64, beta64, act)
    b = G.apply_bound(x64.view(B, H * W, C), mr64, gamma64, beta64, act, dtype, hilo).view(B, H, W, C)
    return RS.replicate2x2(a), RS.replicate2x2(b)


def exact_problem(case, kind, dtype):
    """the exact tier of refs_gn on this pass, pool mode, act = 0, eps = 0: x = m_g +- a_g, dyadic gamma / beta, so every a is +-gamma + beta,
    the quarter of a sum of four such values has at most 7 significant bits and every plane word is known: dict(x, gamma, beta, cs, mr, hi)"""
    B, H, W, C, groups = case
    x1, _, sign, mr = G.exact_pattern(B, H * W, C, 0, 0, groups, kind)
    gamma, beta = G.dyadic_affine(C)
    x = x1.view(B, H, W, C)
    y, xr = gn_resample(x, mr, groups, gamma, beta, 0, POOL)
    assert torch.equal(y.double(), gn_resample(x.double(), mr.double(), groups, gamma.double(), beta.double(), 0, POOL)[0]), "exact in fp32"
    assert torch.equal(y.to(dtype).float(), y), "exact in the 16-bit format"
    return dict(x=x, gamma=gamma, beta=beta, cs=G.chan_partials(x1.double()).float(), mr=mr, hi=y.to(dtype).contiguous().view(torch.int16), xr=xr)
