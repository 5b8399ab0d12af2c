"""Plain torch restatements of the GroupNorm family (stedm_amd/csrc/gn.hip, gn_fold / gn_bwd in gn_bwd.hip), their derived per-element error
bounds, inputs whose outputs are known bit for bit, and fp32 emulations of the kernels with switchable defects. No GPU. Shared by
tests/test_gn_refs_cpu.py (pins the references against torch, holds the honest emulations inside both tiers and every seeded defect
outside one) and tests/test_gpu_gn_exact.py (holds the kernels to the same two tiers).

Tensors are NHWC; every function here flattens them to [B, HW, C]. u = 2^-24 (fp32 unit roundoff), gamma_k = k u / (1 - k u) (the
standard bound of a k-term recursive sum), u_T = 2^-11 (f16) or 2^-8 (bf16).

TIERS
  exact       inputs built so that every fp32 partial, the folded {mean, rstd} and every plane value is a short dyadic number: torch.equal.
  apply       statistics GIVEN: the stored value against group_norm(..., mean_rstd = fold(the partials the kernel itself read)).
              Rounding points of a stored value y = act((x - m) r g + b), m = float(mean), r = float(rstd), D = |x - mean|:
                float(mean): u |mean| on the difference;  x - m: u (D + u |mean|);
                quad kernel  ((x - m) * r) * g + b: float(rstd) u, two products 2u, the sum u |y|
                8-wide / octet kernels  (x - m) * (r * g) + b from the LDS table: float(rstd) u, r * g u, one product u, the sum u |y|
              both orders carry three relative roundings on the product besides the subtraction's, so one formula serves both (a fused
              multiply-add only removes one):
                E_pre = |g| rstd (u |mean| + 4u D) (1 + 8u) + u |y_pre|
              silu_f: |silu'| <= 1.1 carries E_pre through, plus refs_bwd.silu_bound at the reference (arguments widened by E_pre).
              final rounding: u_T |y| + the subnormal half-step of the format (2^-25 for f16); for hi + lo the residual of the split,
              u_T^2 |y| + the same half-step (lo rounds y - hi, and |y - hi| <= u_T |y|).
  statistics  end to end against group_norm on the true inputs: the apply terms plus what the fp32 partials move {mean, rstd} by.
              gn_chan_stats_kernel: a lane adds ceil(slab_px / npl) pixels in a chain (npl = 256 / QB pixel lanes for QB channel quads per
              block), one thread then adds the npl lane partials from LDS: k = ceil(slab_px / npl) + npl terms (k + 1 for the squares:
              the rounded product). The fold is fp64 (its own error, n 2^-53, is added as FOLD64):
                em = gamma_k sum|x| / n,  eq = gamma_(k+1) sum x^2 / n,  dvar = eq + 2 |mean| em + em^2 + FOLD64
                var' in [max(var - dvar, 0), var + dvar] (the clamp), so |d rstd| <= max((max(var - dvar, 0) + eps)^-1/2 - rstd,
                rstd - (var + dvar + eps)^-1/2)
                E_stat = |g| (em (rstd + drstd) + D drstd)
              sum x^2 / n = var + mean^2, so dvar / var grows like 1 + (mean / std)^2: the bound states the conditioning of the one-pass
              variance. gn_stats_kernel: the same form with k = ceil(slab / npl) (gn_stats_k: at most 32 terms - short fp32 runs, fp64 above them).
              gn_scale_shift_kernel: centred two passes in fp32 - see scale_shift_bound; its error does not grow with the offset beyond
              u |mean|.
  backward    see gn_bwd_bounds."""
import torch

from tests import refs_bwd as RB

U = 2.0 ** -24
TINY = 2.0 ** -126
FILL16 = 0x7e7e


def u_T(dtype):
    return 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8


def floor_T(dtype):
    """half the subnormal step of the 16-bit format"""
    return 2.0 ** -25 if dtype == torch.float16 else 2.0 ** -134


def gam(k):
    return k * U / (1.0 - k * U)


def flat(x):
    return None if x is None else x.reshape(x.shape[0], -1, x.shape[-1])


def concat(x1, x2, bmod=0):
    """the virtual concat [x1 | x2] as [B, HW, C]; x2 rows at b % bmod"""
    x1 = flat(x1)
    if x2 is None:
        return x1
    x2 = flat(x2)
    B = x1.shape[0]
    idx = torch.arange(B) % bmod if bmod > 0 else torch.arange(B)
    return torch.cat([x1, x2[idx]], -1)


# ------------------------------------------------------------------------------------------------ references (run in the inputs' dtype; fp64 for a reference)
def slab_px(HW, nslab):
    """pixels per slot: the default partition is 256-pixel runs, any other slot count cuts the sample into ceil(HW / nslab) runs"""
    return 256 if nslab == (HW + 255) // 256 else (HW + nslab - 1) // nslab


def chan_partials(x, nslab=None):
    """x [B, .., C] -> [B, nslab, C, 2] = {sum, sum of squares} per slot; trailing slots of an over-allocated partition are zero"""
    x = flat(x)
    B, HW, C = x.shape
    if not nslab:
        nslab = (HW + 255) // 256
    sp = slab_px(HW, nslab)
    out = x.new_zeros((B, nslab, C, 2))
    for k in range(nslab):
        seg = x[:, min(HW, k * sp):min(HW, (k + 1) * sp)]
        out[:, k, :, 0] = seg.sum(1)
        out[:, k, :, 1] = (seg * seg).sum(1)
    return out


def fold(cs1, cs2, bmod, groups, HW, eps, clamp=True):
    """{mean, rstd} [B, groups, 2] from GIVEN partials (each tensor with its own slot count; cs2 rows at b % bmod), var = q / n - mean^2
    clamped at 0"""
    B = cs1.shape[0]
    s = cs1.double().sum(1)
    if cs2 is not None:
        idx = torch.arange(B) % bmod if bmod > 0 else torch.arange(B)
        s = torch.cat([s, cs2.double().sum(1)[idx]], 1)
    C = s.shape[1]
    cpg = C // groups
    n = float(cpg * HW)
    sg = s.view(B, groups, cpg, 2).sum(2)
    mean = sg[..., 0] / n
    var = sg[..., 1] / n - mean * mean
    if clamp:
        var = var.clamp_min(0.0)
    return torch.stack([mean, 1.0 / torch.sqrt(var + eps)], -1)


def stats_of(x, groups, eps):
    """centred {mean, rstd} [B, groups, 2] and var of the flat concat x [B, HW, C]"""
    B, HW, C = x.shape
    xg = x.view(B, HW, groups, C // groups)
    mean = xg.mean((1, 3))
    var = ((xg - mean.view(B, 1, groups, 1)) ** 2).mean((1, 3))
    return torch.stack([mean, 1.0 / torch.sqrt(var + eps)], -1), var


def per_channel(v, C):
    """[B, groups] -> [B, 1, C]"""
    return v.repeat_interleave(C // v.shape[1], 1).unsqueeze(1)


def group_norm(x1, x2, bmod, groups, gamma, beta, eps, act, mean_rstd=None):
    """act(GroupNorm([x1 | x2])) [B, HW, C]; with mean_rstd [B, groups, 2] given, those statistics are applied"""
    x = concat(x1, x2, bmod)
    C = x.shape[-1]
    mr = stats_of(x, groups, eps)[0] if mean_rstd is None else mean_rstd.to(x.dtype)
    y = (x - per_channel(mr[..., 0], C)) * per_channel(mr[..., 1], C) * gamma + beta
    return RB.silu(y) if act else y


def group_norm_bwd(x, mean_rstd, groups, gamma, beta, act, dA, add=None, old=None):
    """closed form for out = act(GN(x)), x the flat concat [B, HW, C], statistics given (exact ones make it the true gradient):
    dy = dA act'(y); dxh = gamma dy; dx = rstd (dxh - mean_g(dxh) - xh mean_g(dxh xh)) (+ add) (+ old); dgamma = sum dy xh; dbeta = sum dy.
    Returns (dx, dgamma, dbeta)."""
    B, HW, C = x.shape
    cpg = C // groups
    mean, rstd = per_channel(mean_rstd[..., 0], C), per_channel(mean_rstd[..., 1], C)
    xh = (x - mean) * rstd
    dy = RB.silu_grad(xh * gamma + beta, dA) if act else dA
    dxh = dy * gamma
    m1 = dxh.view(B, HW, groups, cpg).mean((1, 3))
    m2 = (dxh * xh).view(B, HW, groups, cpg).mean((1, 3))
    dx = rstd * (dxh - per_channel(m1, C) - xh * per_channel(m2, C))
    if add is not None:
        dx = dx + add
    if old is not None:
        dx = dx + old
    return dx, (dy * xh).sum((0, 1)), dy.sum((0, 1))


def scale_shift(x1, x2, bmod, groups, gamma, beta, eps):
    """scale = gamma rstd, shift = beta - mean scale, [B, C] each"""
    x = concat(x1, x2, bmod)
    C = x.shape[-1]
    mr = stats_of(x, groups, eps)[0]
    sc = per_channel(mr[..., 1], C)[:, 0] * gamma
    return sc, beta - per_channel(mr[..., 0], C)[:, 0] * sc


# ------------------------------------------------------------------------------------------------ launch geometry (gn.hip, restated)
def chan_stats_qbs(B, nslab, Q):
    qbs = 64
    while qbs > 8 and B * nslab * ((Q + qbs - 1) // qbs) < 1024:
        qbs >>= 1
    return qbs


def chan_stats_k(B, C, HW, nslab):
    """the longest summation chain of one partial: lane run + LDS sum, over the block widths of the launch (the last block may be narrower)"""
    Q = C // 4
    if not nslab:
        nslab = (HW + 255) // 256
    qbs = chan_stats_qbs(B, nslab, Q)
    sp = min(slab_px(HW, nslab), HW)
    k = 0
    for QB in {min(qbs, Q - q0) for q0 in range(0, Q, qbs)}:
        npl = 256 // QB
        k = max(k, (sp + npl - 1) // npl + npl)
    return k


def gn_stats_k(C, HW):
    Q = C // 4
    slab = max(1, min(HW, (16384 + C - 1) // C))
    npl = 256 // Q if Q <= 256 else 1
    return (slab + npl - 1) // npl


def apply16c_geometry(B, HW, c1, c2, groups, hilo, x16):
    """(kernel, slab, cb, pair) of gn_apply16c_launch: kernel in {quad, v8, o8}; slab = pixels per pixel-run block; cb = channels per
    channel-run block (0: pixel runs). The X16 entry (single-product only, c1 and C multiples of 8 by its argument check) takes the octet
    kernel, every other 8-wide shape the quad-pair kernel."""
    C = c1 + c2
    want = (128 * 256 + C - 1) // C
    per_sample = max((HW + want - 1) // want, (768 + B - 1) // B)
    per_sample = min(per_sample, HW)
    slab = max(1, min(HW, (HW + per_sample - 1) // per_sample))
    gy = (HW + slab - 1) // slab
    if not (C % 8 == 0 and c1 % 8 == 0 and 3 * C * 4 <= 48 * 1024):
        return "quad", slab, 0, False
    cb = 0
    if gy > 1 and HW <= 256:
        cpg = C // groups
        unit = cpg
        while unit % 8:
            unit *= 2
        for t in range(unit, C // 2 + 1, unit):
            if C % t == 0 and c1 % t == 0 and t >= 128 and B * (C // t) >= 768:
                cb = t
        if cb and (C % cb or c1 % cb or cb % unit or cb // cpg > 64):
            cb = 0
    if x16:
        assert not hilo and cb % 8 == 0
        return "o8", slab, cb, C % 16 == 0 and c1 % 16 == 0 and (cb == 0 or cb % 16 == 0)
    return "v8", slab, cb, False


def gn_bwd_fused_cb(c1, c2, groups, HW):
    """(cb, ppt) of the one-pass backward, (0, 0) for the chain"""
    C = c1 + c2
    cpg = C // groups
    unit = cpg
    while unit % 4:
        unit *= 2

    def ppt_of(cb):
        npl = 512 // (cb // 4)
        return (HW + npl - 1) // npl if npl > 0 else 1 << 20
    best = 0
    for p in range(2):
        if best:
            break
        for cb in range(unit, 289, unit):
            if c1 % cb or (c2 and c2 % cb) or cb < (32 if p == 0 else 16) or ppt_of(cb) > (4 if p == 0 else 8):
                continue
            best = cb
    return (best, ppt_of(best)) if best else (0, 0)


def gn_bwd_ws_floats(B, HW, C, groups):
    return B * ((HW + 63) // 64) * C * 2 + B * C * 2 + B * groups * 2


# ------------------------------------------------------------------------------------------------ bounds
def planes_value(hi, lo, dtype):
    """int16 words -> the fp64 value the planes carry"""
    v = hi.view(dtype).double()
    return v if lo is None else v + lo.view(dtype).double()


def apply_bound(x64, mr64, gamma64, beta64, act, dtype, hilo, em=None, drstd=None):
    """per-element bound [B, HW, C] of the apply tier (module docstring); em / drstd [B, groups]: what the statistics tier adds"""
    C = x64.shape[-1]
    mean, rstd = per_channel(mr64[..., 0], C), per_channel(mr64[..., 1], C)
    D = (x64 - mean).abs()
    r_up = rstd if drstd is None else rstd + per_channel(drstd, C)
    ypre = (x64 - mean) * rstd * gamma64 + beta64
    E = gamma64.abs() * r_up * (U * mean.abs() + 4.0 * U * D) * (1.0 + 8.0 * U) + U * ypre.abs()
    if em is not None:
        E = E + gamma64.abs() * (per_channel(em, C) * r_up + D * per_channel(drstd, C))
        E = E * (1.0 + 8.0 * U)
    y = ypre
    if act:
        y = RB.silu(ypre)
        E = 1.1 * E + RB.silu_bound(ypre.abs() + E, y.abs() + 1.1 * E)
    ut = u_T(dtype)
    return E + (ut * ut if hilo else ut) * (y.abs() + E) + floor_T(dtype) + TINY


FOLD64_C = 2.0 ** -52     # per term of the fp64 fold (sum, the product with 1 / n, the subtraction)


def stats_shift(x64, groups, eps, k, fold_terms=1):
    """(em, drstd) [B, groups]: how far fp32 partials with k-term chains (k + 1 for the squares) move {mean, rstd} (module docstring)"""
    B, HW, C = x64.shape
    cpg = C // groups
    xg = x64.view(B, HW, groups, cpg)
    mr, var = stats_of(x64, groups, eps)
    mean, rstd = mr[..., 0], mr[..., 1]
    em = gam(k) * xg.abs().mean((1, 3))
    msq = (xg * xg).mean((1, 3))
    f64 = FOLD64_C * (fold_terms + 3)
    dvar = gam(k + 1) * msq + 2.0 * mean.abs() * em + em * em + f64 * (msq + mean * mean)
    em = em + f64 * mean.abs()
    up = 1.0 / torch.sqrt((var - dvar).clamp_min(0.0) + eps) - rstd
    dn = rstd - 1.0 / torch.sqrt(var + dvar + eps)
    return em, torch.maximum(up, dn)


def _group_sums(cs1, cs2, bmod, groups):
    """[B, groups, 2]: the partials summed over slots and the group's channels, fp64"""
    B = cs1.shape[0]
    s = cs1.double().sum(1)
    if cs2 is not None:
        idx = torch.arange(B) % bmod if bmod > 0 else torch.arange(B)
        s = torch.cat([s, cs2.double().sum(1)[idx]], 1)
    return s.view(B, groups, s.shape[1] // groups, 2).sum(2)


def mean_rstd_bound(cs1, cs2, bmod, groups, HW, eps):
    """the {mean, rstd} output [B, groups, 2] of a fold against fold() of the SAME partials: the fp64 fold's own error (FOLD64 per term,
    through the cancellation of var = q / n - mean^2) and one float rounding each"""
    mr = fold(cs1, cs2, bmod, groups, HW, eps)
    c2 = 0 if cs2 is None else cs2.shape[2]
    C = cs1.shape[2] + c2
    n = float((C // groups) * HW)
    terms = max(cs1.shape[1], 0 if cs2 is None else cs2.shape[1]) * (C // groups)
    sg = _group_sums(cs1, cs2, bmod, groups) / n
    mabs = _group_sums(cs1.abs(), None if cs2 is None else cs2.abs(), bmod, groups)[..., 0] / n
    f = FOLD64_C * (terms + 3)
    mean, rstd = mr[..., 0], mr[..., 1]
    dvar = f * (sg[..., 1] + 2.0 * mabs * mabs)
    var_eps = 1.0 / (rstd * rstd)
    up = torch.where(var_eps - dvar > 0, 1.0 / torch.sqrt((var_eps - dvar).clamp_min(TINY)), torch.full_like(rstd, float("inf"))) - rstd
    return torch.stack([U * mean.abs() + f * mabs + TINY, U * (rstd + up) + up], -1)


def scale_shift_bound(x64, groups, gamma64, beta64, eps, vec4):
    """gn_scale_shift_kernel, (scale bound, shift bound) [B, C]. A thread adds ceil(n / 256) elements in a chain (VEC4: ceil(n / 1024)
    quads, each a two-level sum: + 2), wave_sum 6 butterfly steps, 3 adds for the four waves: k = chain + 9.
      mean:  em = gamma_k mean|x| + 2u |mean|                     (sum; float(n), the division)
      var:   d = x - mean' rounded, d * d rounded: 4u on a square; sum gamma_k; / n u; a shifted centre adds em^2:
             relative ev = gamma_(k + 5) + em^2 / (var + eps)
      rstd:  var + eps u, sqrtf 1 ulp = 2u, 1 / . u:  er = ev / 2 + 4u  (first order in ev; the bound carries (1 + ev))
      scale = gamma * rstd: u.   shift = beta - mean' * scale: |mean| e_scale + em |scale| + u |mean scale| + u |shift|"""
    B, HW, C = x64.shape
    cpg = C // groups
    n = cpg * HW
    k = ((n + 1023) // 1024 + 2 if vec4 else (n + 255) // 256) + 9
    xg = x64.view(B, HW, groups, cpg)
    mr, var = stats_of(x64, groups, eps)
    mean, rstd = mr[..., 0], mr[..., 1]
    em = gam(k) * xg.abs().mean((1, 3)) + 2.0 * U * mean.abs()
    ev = gam(k + 5) + em * em / (var + eps)
    er = (ev / 2.0 + 4.0 * U) * (1.0 + ev)
    rs = per_channel(rstd, C)[:, 0]
    mc = per_channel(mean, C)[:, 0]
    sc = rs * gamma64
    e_sc = sc.abs() * (per_channel(er, C)[:, 0] + U) + TINY
    sh = beta64 - mc * sc
    e_sh = mc.abs() * e_sc + per_channel(em, C)[:, 0] * (sc.abs() + e_sc) + U * (mc * sc).abs() + U * sh.abs() + TINY
    return e_sc, e_sh


def gn_bwd_bounds(x64, mr64, groups, gamma64, beta64, act, dA64, add64, old64, k, B_terms, dtype=None, hilo=False):
    """stedm_gn_bwd against group_norm_bwd on the SAME fp32 {mean, rstd} (they are an input of the kernel). In the manner of
    refs_bwd.ln_bwd_dx_bound; k = terms of one (sample, channel) sum: one-pass form PPT + npl (a lane's PPT pixels, the npl lane partials
    from LDS), chain ceil(64 / npl) + npl + nslab (64-pixel slabs, then the slabs in fp32).
      xh = (x - m) r:            exh = 2u |xh|
      y = xh g + b:              ey = |g| exh + 2u (|xh g| + |b|)
      dy = dA silu'(y):          edy = silu_grad_bound(y, dA) + 0.5 |dA| ey          (|silu''| <= 0.5);  act = 0: edy = 0
      u_c = sum_p dy, w_c = sum_p dy xh:  gamma_k sum|terms| + sum of the terms' own errors (edy;  edy |xh| + |dy| exh + u |dy xh|)
      m1 = float(sum_c (u_c g_c) / n), m2 likewise:  e1 = (gamma_k + 3u) mean|g dy| + mean(|g| edy);  e2 likewise with the terms of w
      dx = r (g dy - m1 - xh m2):  |err| <= r [ 4u S + |g| edy + e1 + |m2| exh + (|xh| + exh) e2 ],  S = |g dy| + |m1| + |xh m2|
      + add, + old: u (|dx| + |add|), u (|dx + add| + |old|)
      16-bit planes: u_T |dx| (hi alone), u_T^2 |dx| (hi + lo), + the subnormal half-step
      dgamma / dbeta: worst-case column sums over B * HW terms: the (sample, channel) bounds above summed over samples, plus the
      sample sum's own chain gamma_(ceil(B / 16) + 17) (a lane walks every 16th sample, 16 lanes join; + 1 for the accumulate).
    Returns (e_dx [B, HW, C], e_plane or None, e_dgamma [C], e_dbeta [C])."""
    B, HW, C = x64.shape
    cpg = C // groups
    mean, rstd = per_channel(mr64[..., 0], C), per_channel(mr64[..., 1], C)
    xh = (x64 - mean) * rstd
    exh = 2.0 * U * xh.abs()
    if act:
        y = xh * gamma64 + beta64
        ey = gamma64.abs() * exh + 2.0 * U * ((xh * gamma64).abs() + beta64.abs())
        dy = RB.silu_grad(y, dA64)
        edy = RB.silu_grad_bound(y, dA64) + 0.5 * dA64.abs() * ey
    else:
        dy = dA64
        edy = torch.zeros_like(dA64)
    t2 = dy * xh
    et2 = edy * xh.abs() + (dy.abs() + edy) * exh + U * t2.abs()
    e_u = gam(k) * dy.abs().sum(1) + edy.sum(1)             # [B, C]
    e_w = gam(k + 1) * t2.abs().sum(1) + et2.sum(1)
    n = float(cpg * HW)
    ga = gamma64.abs()
    e1 = ((e_u * ga + 3.0 * U * dy.abs().sum(1) * ga).view(B, groups, cpg).sum(2)) / n
    e2 = ((e_w * ga + 3.0 * U * t2.abs().sum(1) * ga).view(B, groups, cpg).sum(2)) / n
    dxh = dy * gamma64
    m1 = per_channel(dxh.view(B, HW, groups, cpg).mean((1, 3)), C)
    m2 = per_channel((dxh * xh).view(B, HW, groups, cpg).mean((1, 3)), C)
    S = dxh.abs() + m1.abs() + (xh * m2).abs()
    e = rstd * (4.0 * U * S + ga * edy + per_channel(e1, C) + m2.abs() * exh + (xh.abs() + exh) * per_channel(e2, C))
    dx = rstd * (dxh - m1 - xh * m2)
    if add64 is not None:
        e = e + U * (dx.abs() + add64.abs() + e)
        dx = dx + add64
    if old64 is not None:
        e = e + U * (dx.abs() + old64.abs() + e)
        dx = dx + old64
    e = e + TINY
    ep = None
    if dtype is not None:
        ut = u_T(dtype)
        ep = e + (ut * ut if hilo else ut) * (dx.abs() + e) + floor_T(dtype)
    kb = (B_terms + 15) // 16 + 17
    e_dg = e_w.sum(0) + gam(kb) * t2.abs().sum((0, 1)) + TINY
    e_db = e_u.sum(0) + gam(kb) * dy.abs().sum((0, 1)) + TINY
    return e, ep, e_dg, e_db


def gn_bwd_k(c1, c2, groups, HW):
    cb, ppt = gn_bwd_fused_cb(c1, c2, groups, HW)
    if cb:
        return ppt + 512 // (cb // 4)
    Q = (c1 + c2) // 4
    k = 0
    for QB in {min(64, Q - q0) for q0 in range(0, Q, 64)}:
        npl = 256 // QB
        k = max(k, (64 + npl - 1) // npl + npl)
    return k + (HW + 63) // 64


# ------------------------------------------------------------------------------------------------ inputs
def normal(shape, seed, name, std=1.0, mean=0.0):
    return RB.normal(shape, seed, "gn." + name, std=std, mean=mean)


def dyadic_affine(C):
    """per-channel gamma in {1/2, 1, 2, -1}, beta in {-1, 0, 1/4, 3}: +-gamma + beta has at most 5 significant bits"""
    c = torch.arange(C)
    gamma = torch.tensor([0.5, 1.0, 2.0, -1.0])[(c * 3 + 1) % 4]
    beta = torch.tensor([-1.0, 0.0, 0.25, 3.0])[(c // 2 + c) % 4]
    return gamma.float(), beta.float()


def pattern_ma(B, groups, per_sample):
    """m [B, groups] (multiples of 1/8 in [-15/8, 15/8]) and a [groups] (2^-2 .. 2^2): distinct (m, a) for neighbouring groups and samples"""
    g = torch.arange(groups).view(1, groups)
    b = torch.arange(B).view(B, 1) if per_sample else torch.zeros(B, 1, dtype=torch.long)
    m = (((g * 7 + b * 11 + 3) % 31) - 15).double() / 8.0
    a = 2.0 ** ((torch.arange(groups) % 5) - 2).double()
    return m, a


def exact_pattern(B, HW, c1, c2, bmod, groups, kind):
    """x1 [B, HW, c1], x2 [B2, HW, c2] fp32 (x2 None when c2 == 0), sign [B, HW, C] and the {mean, rstd} [B, groups, 2] they must fold to.
    x = m_g + s a_g with as many s = +1 as s = -1 in every channel.
      kind 'A': s = (-1)^(pixel + channel), m_g the same for every sample;
      kind 'B': s from a fixed shuffle of the pixels (no symmetry, the slots' partials all differ), m_g distinct per sample.
    A group that touches x2 takes m of sample b % bmod (x2 has only bmod rows). HW must be even."""
    assert HW % 2 == 0
    C = c1 + c2
    cpg = C // groups
    B2 = bmod if (bmod > 0 and c2) else B
    m, a = pattern_ma(B, groups, kind == "B")
    if bmod > 0 and c2:
        touches = (torch.arange(groups) + 1) * cpg > c1
        m = torch.where(touches.view(1, groups), m[torch.arange(B) % bmod], m)
    p = torch.arange(HW).view(HW, 1)
    c = torch.arange(C).view(1, C)
    if kind == "A":
        s = 1.0 - 2.0 * ((p + c) % 2).double()
    else:
        perm = torch.randperm(HW, generator=torch.Generator().manual_seed(HW))
        s = torch.ones(HW, dtype=torch.float64)
        s[perm[:HW // 2]] = -1.0
        s = s.view(HW, 1).expand(HW, C)
    x = per_channel(m, C) + s.unsqueeze(0) * per_channel(a.view(1, groups).expand(B, groups), C)
    x = x.float()
    x1 = x[..., :c1].contiguous()
    x2 = x[:B2, :, c1:].contiguous() if c2 else None
    mr = torch.stack([m, (1.0 / a).view(1, groups).expand(B, groups)], -1)
    return x1, x2, s.unsqueeze(0).expand(B, HW, C), mr.float()


def exact_planes(sign, gamma, beta, dtype):
    """the plane words of the exact pattern: +-gamma_c + beta_c, exactly"""
    y = sign.float() * gamma + beta
    assert torch.equal(y.to(dtype).float(), y)
    return y.to(dtype).contiguous().view(torch.int16)


def exact_bwd(sign, mr, groups, gamma, B, HW, C):
    """dA = d_c + e_c s (dyadic d, e per channel) on the exact pattern, act = 0: xh = s, so sum_p dy = HW d_c, sum_p dy xh = HW e_c,
    m1 = mean_c(g d), m2 = mean_c(g e) over the group, dx = (1 / a) (g (d + e s) - m1 - s m2): every sum is exact in fp32 in any order; the
    two group means are one float rounding of an exact fp64 quotient (exact when cpg is a power of two) and the last two subtractions
    round once each, the same with or without fused multiply-adds (xh = +-1 makes xh m2 exact).
    Returns dA fp32 [B, HW, C], and the expected (dx, dgamma, dbeta) fp32."""
    c = torch.arange(C)
    d = (((c * 5 + 2) % 9) - 4).float() / 4.0
    e = (((c * 3 + 1) % 7) - 3).float() / 8.0
    s = sign.float()
    dA = d + e * s
    cpg = C // groups
    n = float(cpg * HW)
    m1 = ((gamma.double() * d.double() * HW).view(groups, cpg).sum(1) / n).float()
    m2 = ((gamma.double() * e.double() * HW).view(groups, cpg).sum(1) / n).float()
    m1c, m2c = m1.repeat_interleave(cpg), m2.repeat_interleave(cpg)
    rstd = per_channel(mr[..., 1], C)
    dx = rstd * ((gamma * dA - m1c) - s * m2c)
    return dA.contiguous(), dx, B * HW * e, B * HW * d


# ------------------------------------------------------------------------------------------------ fp32 emulations (order of operations of the kernels)
def emu_chan_stats(x32, nslab=None, defects=()):
    """gn_chan_stats_kernel: [B, nslab, C, 2] fp32; lane tp of a block adds pixels px0 + tp, + npl, ... in a chain, then the lanes in order.
    defect 'stats_tail': the last pixel of a ragged last slot is not read"""
    x = flat(x32)
    B, HW, C = x.shape
    Q = C // 4
    if not nslab:
        nslab = (HW + 255) // 256
    sp = slab_px(HW, nslab)
    qbs = chan_stats_qbs(B, nslab, Q)
    out = torch.zeros((B, nslab, C, 2), dtype=torch.float32)
    nfull = Q // qbs
    # blocks of one width run the same lane schedule: the full blocks are emulated together, the narrower last block on its own
    for QB, cs in ((qbs, slice(0, nfull * qbs * 4)), (Q - nfull * qbs, slice(nfull * qbs * 4, C))):
        if QB == 0 or cs.start == cs.stop:
            continue
        npl = 256 // QB
        for k in range(nslab):
            p0, p1 = min(HW, k * sp), min(HW, (k + 1) * sp)
            if "stats_tail" in defects and p1 == HW and (p1 - p0) % sp:
                p1 -= 1
            su = torch.zeros((B, cs.stop - cs.start), dtype=torch.float32)
            sq = torch.zeros_like(su)
            for tp in range(min(npl, max(p1 - p0, 0))):      # (lanes beyond the slot's pixels add 0)
                s = torch.zeros_like(su)
                q = torch.zeros_like(su)
                for pix in range(p0 + tp, p1, npl):
                    v = x[:, pix, cs]
                    s = s + v
                    q = q + v * v
                su = su + s
                sq = sq + q
            out[:, k, cs, 0] = su
            out[:, k, cs, 1] = sq
    return out


def emu_fold(cs1, cs2, bmod, groups, HW, eps, defects=()):
    """the fold of the apply kernels and of gn_fold_kernel: fp64 sums of the fp32 partials, {float(mean), float(rstd)}.
    defects: 'fold_last_slot' (the last slot of each tensor left out), 'cs2_row' (cs2 read at b), 'nslab1_both' (cs2 walked with cs1's slot
    count), 'no_clamp'"""
    B = cs1.shape[0]
    if cs2 is not None:
        if "cs2_row" in defects:
            cs2 = cs2[torch.arange(B).clamp_max(cs2.shape[0] - 1)]      # (rows past the tensor stand in as its last row)
            bmod = 0
        if "nslab1_both" in defects and cs2.shape[1] != cs1.shape[1]:
            n1 = cs1.shape[1]
            cs2 = cs2[:, :n1] if cs2.shape[1] > n1 else torch.cat([cs2, cs2[:, :1].expand(-1, n1 - cs2.shape[1], -1, -1)], 1)
    if "fold_last_slot" in defects:
        cs1 = cs1[:, :max(1, cs1.shape[1] - 1)] if cs1.shape[1] > 1 else cs1 * 0.5
        if cs2 is not None:
            cs2 = cs2[:, :cs2.shape[1] - 1] if cs2.shape[1] > 1 else cs2
    return fold(cs1, cs2, bmod, groups, HW, eps, clamp="no_clamp" not in defects).float()


def _split(w32, dtype, hilo, lo_unrounded=False):
    hi = w32.to(dtype)
    if not hilo:
        return hi.contiguous().view(torch.int16), None
    lo = (w32 - (w32 if lo_unrounded else hi.float())).to(dtype)
    return hi.contiguous().view(torch.int16), lo.contiguous().view(torch.int16)


def emu_apply16c(x1, x2, bmod, mr32, groups, gamma, beta, act, dtype, hilo, geom, c1, x16_raw=None, want_raw=False, defects=()):
    """the three gn_apply16c bodies in fp32. geom = apply16c_geometry(...). x16_raw: int16 raw plane [B, HW, C] whose [0, c1) half is the
    source (X16 form; x1 is then ignored). Returns dict(hi, lo, raw, raw_lo) of int16 [B, HW, C] (None where not produced).
    defects: 'quad_group' (a quad's channels all take the group of its first channel), 'cut_table' (a channel-run block builds its table
    from group g instead of g_lo + g), 'lo_unrounded', 'tail' (the partial last iteration of a block run is not stored),
    'x16_rewrite' (the [0, c1) half of the raw plane rewritten), 'x16_skip' (the [c1, C) half of the raw plane not written)"""
    kernel, slab, cb, pair = geom
    if x16_raw is not None:
        x1 = x16_raw.view(dtype)[..., :c1].float()
    x = concat(x1, x2, bmod).float()
    B, HW, C = x.shape
    cpg = C // groups
    ch = torch.arange(C)
    gidx = ch // cpg
    if "quad_group" in defects and kernel == "quad":
        gidx = (ch // 4 * 4) // cpg
    if "cut_table" in defects and cb > 0:
        gidx = (ch % cb) // cpg
    m = mr32[..., 0][:, gidx].unsqueeze(1)
    r = mr32[..., 1][:, gidx].unsqueeze(1)
    if kernel == "quad":
        w = ((x - m) * r) * gamma + beta
    else:
        w = (x - m) * (r * gamma) + beta
    if act:
        w = w * torch.sigmoid(w)
    hi, lo = _split(w, dtype, hilo, "lo_unrounded" in defects)
    raw = raw_lo = None
    if want_raw or x16_raw is not None:
        raw, raw_lo = _split(x, dtype, hilo and x16_raw is None)
        if x16_raw is not None:
            raw = raw.clone()
            raw[..., :c1] = x16_raw[..., :c1]
            if "x16_rewrite" in defects:
                raw[..., :c1] = 0
            if "x16_skip" in defects:
                raw[..., c1:] = x16_raw[..., c1:]
    if "tail" in defects and cb == 0 and kernel != "quad":
        unit = 8 if kernel == "o8" else 4
        step = 256 if kernel == "o8" else 512
        per = C // unit
        hi = hi.clone().view(B, HW * per, unit)
        for p0 in range(0, HW, slab):
            total = (min(HW, p0 + slab) - p0) * per
            hi[:, p0 * per + total // step * step:p0 * per + total] = FILL16
        hi = hi.view(B, HW, C)
    return dict(hi=hi, lo=lo, raw=raw, raw_lo=raw_lo)


def emu_gn_stats_fold(x1, x2, bmod, groups, eps):
    """gn_stats + the fold of gn_apply16: fp32 runs of gn_stats_k(C, HW) pixels under fp64 sums -> float {mean, rstd}"""
    x = concat(x1, x2, bmod)
    B, HW, C = x.shape
    k = gn_stats_k(C, HW)
    xs = x.float()
    s = torch.zeros((B, C), dtype=torch.float64)
    q = torch.zeros((B, C), dtype=torch.float64)
    for p0 in range(0, HW, k):          # runs of k pixels in fp32, joined in fp64
        s32 = torch.zeros((B, C), dtype=torch.float32)
        q32 = torch.zeros((B, C), dtype=torch.float32)
        for pix in range(p0, min(HW, p0 + k)):
            s32 = s32 + xs[:, pix]
            q32 = q32 + xs[:, pix] * xs[:, pix]
        s += s32.double()
        q += q32.double()
    cs = torch.stack([s, q], -1).unsqueeze(1)
    return fold(cs, None, 0, groups, HW, eps).float()


def emu_scale_shift(x1, x2, bmod, groups, gamma, beta, eps):
    """gn_scale_shift_kernel in fp32: centred two passes (torch's fp32 sums stand for the block's tree)"""
    x = concat(x1, x2, bmod).float()
    B, HW, C = x.shape
    cpg = C // groups
    xg = x.view(B, HW, groups, cpg)
    n = float(cpg * HW)
    mean = xg.sum((1, 3)) / n
    d = xg - mean.view(B, 1, groups, 1)
    var = (d * d).sum((1, 3)) / n
    rstd = 1.0 / torch.sqrt(var + eps)
    sc = per_channel(rstd, C)[:, 0] * gamma
    return sc, beta - per_channel(mean, C)[:, 0] * sc


def emu_gn_bwd(x1, x2, mr32, groups, gamma, beta, act, dA, add, old1, old2, acc1, acc2, dtype, planes, dgamma0, dbeta0, acc_param, defects=()):
    """stedm_gn_bwd in fp32 torch. planes in {None, 'hi', 'hilo'}. Returns dict(dx1, dx2, hi, lo, dgamma, dbeta).
    defects: 'acc2' (acc2 ignored: acc1 decides both halves), 'acc_param' (ignored: always overwrites), 'add_planes' (add missing from the
    16-bit planes), 'x2_means' (the x2 half's group means divided by c2 * HW instead of cpg * HW)"""
    x = concat(x1, x2, 0).float()
    B, HW, C = x.shape
    c1 = flat(x1).shape[-1]
    cpg = C // groups
    mean, rstd = per_channel(mr32[..., 0], C), per_channel(mr32[..., 1], C)
    xh = (x - mean) * rstd
    dA = flat(dA).float()
    if act:
        y = xh * gamma + beta
        s = torch.sigmoid(y)
        dy = dA * (s * (1.0 + y * (1.0 - s)))
    else:
        dy = dA
    u = dy.sum(1)
    w = (dy * xh).sum(1)
    n = torch.full((C,), float(cpg * HW), dtype=torch.float64)
    if "x2_means" in defects and C > c1:
        n[c1:] = float((C - c1) * HW)
    ng = n.view(groups, cpg)[:, -1]
    m1 = ((u * gamma).double().view(B, groups, cpg).sum(2) / ng).float()
    m2 = ((w * gamma).double().view(B, groups, cpg).sum(2) / ng).float()
    r = rstd * ((gamma * dy - per_channel(m1, C)) - xh * per_channel(m2, C))
    if add is not None:
        r = r + flat(add).float()
    a2 = acc1 if "acc2" in defects else acc2
    full = r.clone()
    if acc1:
        full[..., :c1] = r[..., :c1] + flat(old1)
    if a2 and C > c1:
        full[..., c1:] = r[..., c1:] + flat(old2)
    hi = lo = None
    if planes:
        src = full - (flat(add).float() if ("add_planes" in defects and add is not None) else 0.0)
        hi, lo = _split(src, dtype, planes == "hilo")
    accp = acc_param and "acc_param" not in defects
    dg = (dgamma0 if accp else 0.0) + w.sum(0)
    db = (dbeta0 if accp else 0.0) + u.sum(0)
    return dict(dx1=full[..., :c1].contiguous(), dx2=full[..., c1:].contiguous() if C > c1 else None, hi=hi, lo=lo, dgamma=dg, dbeta=db)


# ------------------------------------------------------------------------------------------------ cases shared by the CPU and the GPU tier
# forward: (id, B, H, W, c1, c2, bmod, groups, form, ns1_mult, ns2_mult); form in {f32, hilo, x16}; ns*_mult: slot count of cs1 / cs2 as a
# multiple of the default (the convolution epilogues write 4x). The branch each case takes by the rules of gn_apply16c_launch (768-block
# arithmetic: per sample max(ceil(HW / ceil(32768 / C)), ceil(768 / B)) blocks, at most HW), asserted by test_geometry_names_every_form:
FWD = [
    # c1 % 8 != 0 -> the quad kernel (gn_apply16c_kernel). cpg = 2: a quad spans two groups (per-element lookup); 1-pixel blocks
    ("quad_cpg2", 2, 8, 8, 36, 28, 0, 32, "f32", 1, 1),
    # cpg = 6: quads straddle groups at every third quad; hi + lo; cs2 in 4 slots against cs1's one
    ("quad_cpg6", 2, 10, 10, 36, 12, 0, 8, "hilo", 1, 4),
    # c1 = 4 (one quad before the seam), cpg = 4: the `cpg % 4 == 0` arm; 2-pixel blocks over 400 pixels (ragged second slot), cs1 in 8 slots of 50
    ("quad_cpg4_c1_4", 3, 20, 20, 4, 60, 0, 16, "f32", 4, 1),
    # 64 groups: L = 256 / 64 = 4 fold lanes per group, cpg = 4
    ("quad_g64", 2, 8, 8, 132, 124, 0, 64, "hilo", 1, 1),
    # B = 1, HW = 1024: 768 blocks per sample -> 2-pixel runs of 769 quads = 1538 > 1024: the block loop runs twice (second load_batch, the
    # cursors advance and wrap, the last cursors of the second pass are dead); cpg = 769 (per-element lookup), c1 = 1540 = 8 * 192 + 4
    ("quad_two_passes", 1, 32, 32, 1540, 1536, 0, 4, "f32", 1, 1),
    # C = 96, c1 = 64 multiples of 8 -> the 8-wide kernel; HW = 400 > 256 -> pixel runs of 2 pixels: 48 quads < 512, the tail body alone
    ("v8_pixel_tail_only", 2, 20, 20, 64, 32, 0, 8, "f32", 1, 4),
    # B = 3: 256 blocks per sample of 1024 pixels -> 4-pixel runs x 128 quads = 512: one full iteration, no tail
    ("v8_pixel_notail", 3, 32, 32, 384, 128, 0, 32, "f32", 1, 1),
    # the same with C = 640: 4 x 160 = 640 quads = one full iteration + a tail of 128
    ("v8_pixel_full_tail", 3, 32, 32, 512, 128, 0, 32, "f32", 4, 1),
    # hi + lo planes through the 8-wide kernel (lane pairs exchange four quads); HW = 256, B * C / t >= 768 for no run t -> 1-pixel runs
    ("v8_hilo", 2, 16, 16, 512, 128, 0, 32, "hilo", 4, 1),
    # one group: L = 256 fold lanes, cpg = 16
    ("v8_g1", 2, 8, 8, 8, 8, 0, 1, "hilo", 1, 1),
    # cpg = 5 (the table is per channel: no quad / group alignment needed); C = 40, c1 = 24: multiples of 8, not of 16
    ("v8_cpg5", 2, 8, 8, 24, 16, 0, 8, "f32", 1, 1),
    # HW = 64 <= 256, C = 512, cpg = 16: t = 128 gives 200 * 4 = 800 >= 768 blocks -> cb = 128: four channel-run blocks of 8 groups per sample
    ("v8_chan", 200, 8, 8, 256, 256, 0, 32, "f32", 1, 1),
    ("v8_chan_bmod", 200, 8, 8, 256, 256, 100, 32, "hilo", 1, 1),
    # stedm_gn_apply16c_x16 -> the octet kernel. C = 2048, c1 = 1024 multiples of 16, HW = 64, cpg = 64: t = 128 gives 48 * 16 = 768 -> cb = 128, PAIR
    ("x16_pair_chan", 48, 8, 8, 1024, 1024, 24, 32, "x16", 4, 1),
    # HW = 1024 > 256 -> pixel runs (3 pixels x 32 octets = 96 < 256: tail only); C = 256, c1 = 128 multiples of 16 -> PAIR
    ("x16_pair_pixel", 2, 32, 32, 128, 128, 0, 32, "x16", 4, 1),
    # 4 pixels x 64 octets = 256: one full iteration, no tail
    ("x16_pixel_notail", 3, 32, 32, 256, 256, 0, 32, "x16", 4, 1),
    # c1 = 136 is a multiple of 8 but not of 16 -> no PAIR (C = 256 keeps 32 groups)
    ("x16_unpaired", 2, 8, 8, 136, 120, 0, 32, "x16", 1, 1),
    # c2 == 0 (unet.py:592): every channel from the 16-bit source, no fp32 load, no raw store
    ("x16_c2_0", 2, 10, 10, 64, 0, 0, 8, "x16", 4, 1),
    # 1024 + 512, cpg = 48: group 21 straddles the seam; no channel run divides both halves -> 1-pixel runs, PAIR
    ("x16_straddle", 1, 8, 8, 1024, 512, 0, 32, "x16", 4, 1),
    # 64 groups, bmod = 2 with B = 3
    ("x16_g64", 3, 8, 8, 128, 128, 2, 64, "x16", 1, 1),
]
FWD_IDS = [c[0] for c in FWD]

# backward: (id, B, H, W, c1, c2, groups). gn_bwd_fused_cb: the widest run cb of whole groups (<= 288 channels, dividing c1 and c2) with
# ppt = ceil(HW / (512 / (cb / 4))) <= 4 and cb >= 32, else <= 8 and cb >= 16, else the chain
BWD = [
    ("fused_ppt2", 2, 8, 8, 64, 64, 8),              # cb = 64: 32 pixel lanes, ppt = 2 -> <T, 2>
    ("fused_ppt4", 2, 16, 16, 128, 128, 32),         # cb = 32: 64 lanes, ppt = 4 -> <T, 4>
    ("fused_ppt8", 2, 16, 16, 48, 0, 8),             # cb = 48 (only 6-channel multiples divide): 42 lanes, ppt = 7 -> <T, 8>
    ("fused_ragged", 3, 10, 10, 64, 0, 32),          # HW = 100: a ragged second 64-pixel slab; cb = 64, ppt = 4 with dead pixels in the last pass
    ("fused_g64", 2, 8, 8, 256, 256, 64),            # 64 groups (cpg = 8), cb = 128
    ("chain_c1536", 1, 8, 8, 1024, 512, 32),         # cpg = 48: no multiple of 48 divides 1024 -> the chain
    ("chain_64x64", 1, 64, 64, 64, 64, 32),          # HW = 4096: ppt > 8 at every cb -> the chain, 64 slabs
    ("chain_ragged_cpg6", 2, 10, 10, 36, 12, 8),     # cpg = 6: quads straddle groups (the per-element arm of the apply kernel); ragged slab
]
BWD_IDS = [c[0] for c in BWD]

# gn_chan_stats on its own: (B, C, H, W, slot count as a multiple of the default, extra trailing slots). Block widths qbs (chan_stats_qbs):
# 8, 8 (ragged last slot), 64, 32, 16, 8 (C = 1536), 8 (caller-chosen partition: 50-pixel runs), 8 (over-allocated: trailing zero slots)
CHAN_STATS = [(2, 4, 8, 8, 1, 0), (2, 64, 20, 20, 1, 0), (1024, 256, 6, 6, 1, 0), (512, 256, 6, 6, 1, 0), (256, 256, 6, 6, 1, 0),
              (1, 1536, 16, 16, 1, 0), (2, 64, 20, 20, 4, 0), (2, 64, 8, 8, 1, 3)]

OFFSETS = [0.0, 4.0, 32.0, 256.0, 2048.0]
# (id, B, H, W, C, groups): cpg * HW = 128 and 49152
SWEEP = [("narrow", 2, 4, 4, 64, 8), ("wide", 1, 64, 64, 96, 8)]


def dt(prec):
    return torch.float16 if prec in ("f16", "parity") else torch.bfloat16


def fwd_inputs(case, seed=0):
    name, B, H, W, c1, c2, bmod, groups, form, _, _ = case
    s = RB.case_seed(name) + seed
    x1 = normal((B, H * W, c1), s, "x1", 1.7, 0.3)
    x2 = normal((bmod or B, H * W, c2), s, "x2", 0.6, -0.2) if c2 else None
    gamma = normal((c1 + c2,), s, "gamma", 0.3, 1.0)
    beta = normal((c1 + c2,), s, "beta", 0.2)
    return x1, x2, gamma, beta


def bwd_inputs(case):
    name, B, H, W, c1, c2, groups = case
    s = RB.case_seed(name)
    C = c1 + c2
    x1 = normal((B, H * W, c1), s, "bx1", 1.5, 0.3)
    x2 = normal((B, H * W, c2), s, "bx2", 0.7, -0.4) if c2 else None
    gamma = normal((C,), s, "bgamma", 0.3, 1.0)
    beta = normal((C,), s, "bbeta", 0.2)
    dA = normal((B, H * W, C), s, "bdA")
    add = normal((B, H * W, C), s, "badd")
    old = normal((B, H * W, C), s, "bold")
    return x1, x2, gamma, beta, dA, add, old


# ------------------------------------------------------------------------------------------------ the checks both tiers of tests run
def forms(case):
    """the case in every plane mode its entry accepts: the X16 entry is single-product only, stedm_gn_apply16c takes both"""
    return [case] if case[8] == "x16" else [case[:8] + (f,) + case[9:] for f in ("f32", "hilo")]


def case_dims(case):
    name, B, H, W, c1, c2, bmod, groups, form, m1, m2 = case
    HW = H * W
    d = (HW + 255) // 256
    return B, HW, c1, c2, bmod, groups, form, d * m1, d * m2


def fwd_exact_problem(case, kind, dtype):
    """inputs and the bit-exact expectation of one forward case on the exact pattern (eps = 0, act = 0)"""
    B, HW, c1, c2, bmod, groups, form, ns1, ns2 = case_dims(case)
    x1, x2, sign, mr = exact_pattern(B, HW, c1, c2, bmod, groups, kind)
    gamma, beta = dyadic_affine(c1 + c2)
    raw = concat(x1, x2, bmod)
    assert torch.equal(raw.to(dtype).float(), raw)
    hi = exact_planes(sign, gamma, beta, dtype)
    z = torch.zeros_like(hi)
    return dict(x1=x1, x2=x2, gamma=gamma, beta=beta, cs1=chan_partials(x1.double(), ns1).float(),
                cs2=None if x2 is None else chan_partials(x2.double(), ns2).float(), mr=mr, hi=hi, lo=z,
                raw=raw.to(dtype).contiguous().view(torch.int16), raw_lo=z)


def exact_mismatches(exp, out, keys=("cs1", "cs2", "mr", "hi", "lo", "raw", "raw_lo")):
    """names of the outputs present in `out` that are not bit-equal to the expectation (with the count of differing elements)"""
    bad = []
    for k in keys:
        if out.get(k) is None:
            continue
        e, o = exp[k].reshape(-1), out[k].reshape(-1)
        if e.shape != o.shape or e.dtype != o.dtype:
            bad.append(f"{k}: shape / dtype")
        elif not torch.equal(e, o):
            nd = (e != o) | (e.isnan() != o.isnan()) if e.is_floating_point() else e != o
            bad.append(f"{k}: {int(nd.sum())} of {e.numel()} differ, first at {int(nd.nonzero()[0])}")
    return bad


def ratio(err, bound):
    """worst err / bound; NaN or inf in err counts as inf"""
    r = err / bound
    r = torch.where(torch.isfinite(err), r, torch.full_like(r, float("inf")))
    r = torch.where((err == 0) & ~torch.isfinite(bound), torch.zeros_like(r), r)
    return float(r.max())


def partials_ratio(x, cs, B_launch=None):
    """fp32 partials [B, nslab, C, 2] against the fp64 ones, bound gamma_k sum|x| / gamma_(k+1) sum x^2 per slot"""
    x = flat(x).double()
    B, HW, C = x.shape
    ns = cs.shape[1]
    k = chan_stats_k(B_launch or B, C, HW, ns)
    ref = chan_partials(x, ns)
    refa = chan_partials(x.abs(), ns)
    bound = torch.stack([gam(k) * refa[..., 0], gam(k + 1) * ref[..., 1]], -1) + TINY
    return ratio((cs.double() - ref).abs(), bound)


def fwd_ratios(case, x1, x2, gamma, beta, eps, act, dtype, out, stats_k=None):
    """worst err / bound of every output of a forward case: 'cs' (partials), 'mr' (the fold against fold() of the same partials), 'apply'
    (planes, statistics given), 'stats' (planes end to end). out: cs1, cs2, mr (or None), hi, lo (or None), x16 (the 16-bit x1 values
    as fp64, X16 form). stats_k overrides the chain length of the partials (default: gn_chan_stats_kernel's)."""
    B, HW, c1, c2, bmod, groups, form, ns1, ns2 = case_dims(case)
    hilo = form == "hilo"
    g64, b64 = gamma.double(), beta.double()
    r = {}
    cs1, cs2 = out["cs1"], out.get("cs2")
    r["cs"] = max(partials_ratio(x1, cs1), 0.0 if cs2 is None else partials_ratio(x2, cs2))
    mr_own = fold(cs1, cs2, bmod, groups, HW, eps)
    if out.get("mr") is not None:
        r["mr"] = ratio((out["mr"].double() - mr_own).abs(), mean_rstd_bound(cs1, cs2, bmod, groups, HW, eps))
    xa1 = out["x16"] if form == "x16" else flat(x1).double()
    x2d = None if x2 is None else flat(x2).double()
    xa = concat(xa1, x2d, bmod)
    got = planes_value(out["hi"], out.get("lo"), dtype)
    ref = group_norm(xa1, x2d, bmod, groups, g64, b64, eps, act, mean_rstd=mr_own)
    r["apply"] = ratio((got - ref).abs(), apply_bound(xa, mr_own, g64, b64, act, dtype, hilo))
    xt = concat(flat(x1).double(), x2d, bmod)
    mr_true = stats_of(xt, groups, eps)[0]
    k = stats_k or max(chan_stats_k(B, c1, HW, ns1), chan_stats_k(x2.shape[0], c2, HW, ns2) if c2 else 0)
    em, drstd = stats_shift(xt, groups, eps, k, fold_terms=max(ns1, ns2) * ((c1 + c2) // groups))
    ref2 = group_norm(xa1, x2d, bmod, groups, g64, b64, eps, act, mean_rstd=mr_true)
    r["stats"] = ratio((got - ref2).abs(), apply_bound(xa, mr_true, g64, b64, act, dtype, hilo, em, drstd))
    return r


def bwd_ratios(case, x1, x2, mr32, gamma, beta, act, dA, add, old1, old2, dtype, planes, dg0, db0, out):
    """worst err / bound of dx, the 16-bit planes, dgamma, dbeta of a backward case against group_norm_bwd on the given fp32 statistics"""
    name, B, H, W, c1, c2, groups = case
    HW = H * W
    x = concat(x1, x2, 0).double()
    old = None
    if old1 is not None or old2 is not None:
        old = torch.zeros_like(x)
        if old1 is not None:
            old[..., :c1] = flat(old1).double()
        if old2 is not None:
            old[..., c1:] = flat(old2).double()
    a64 = None if add is None else flat(add).double()
    dx, dg, db = group_norm_bwd(x, mr32.double(), groups, gamma.double(), beta.double(), act, flat(dA).double(), a64, old)
    e, ep, e_dg, e_db = gn_bwd_bounds(x, mr32.double(), groups, gamma.double(), beta.double(), act, flat(dA).double(), a64, old,
                                      gn_bwd_k(c1, c2, groups, HW), B, dtype if planes else None, planes == "hilo")
    got = torch.cat([flat(out["dx1"])] + ([flat(out["dx2"])] if c2 else []), -1).double()
    r = {"dx": ratio((got - dx).abs(), e)}
    if planes:
        r["planes"] = ratio((planes_value(out["hi"], out.get("lo"), dtype) - dx).abs(), ep)
    if dg0 is not None:
        dg, db = dg + dg0.double(), db + db0.double()
        e_dg, e_db = e_dg + U * dg.abs(), e_db + U * db.abs()
    r["dgamma"] = ratio((out["dgamma"].double() - dg).abs(), e_dg)
    r["dbeta"] = ratio((out["dbeta"].double() - db).abs(), e_db)
    return r


def x16_words(x1, dtype):
    """the 16-bit words a producing convolution's epilogue leaves for x1: torch's round-to-nearest-even cast"""
    return flat(x1).to(dtype).contiguous().view(torch.int16)


def emu_forward(case, x1, x2, gamma, beta, eps, act, dtype, defects=()):
    """gn_chan_stats (x2) -> fold -> the apply kernel of the case's form, all emulated: the outputs a GPU run of the case produces"""
    B, HW, c1, c2, bmod, groups, form, ns1, ns2 = case_dims(case)
    cs1 = emu_chan_stats(x1, ns1, defects)
    cs2 = emu_chan_stats(x2, ns2, defects) if c2 else None
    mr = emu_fold(cs1, cs2, bmod, groups, HW, eps, defects)
    geom = apply16c_geometry(B, HW, c1, c2, groups, form == "hilo", form == "x16")
    raw16 = None
    if form == "x16":
        raw16 = torch.full((B, HW, c1 + c2), FILL16, dtype=torch.int16)
        raw16[..., :c1] = x16_words(x1, dtype)
    out = emu_apply16c(x1, x2, bmod, mr, groups, gamma, beta, act, dtype, form == "hilo", geom, c1, x16_raw=raw16, want_raw=True, defects=defects)
    out.update(cs1=cs1, cs2=cs2, mr=mr, x16=x16_words(x1, dtype).view(dtype).double() if form == "x16" else None)
    return out


def sweep_inputs(sw, mu):
    """x [B, HW, C] = mu + z (sigma = 1); in sample 0, group 0 is all zero, group 1 the dyadic constant 1.5, group 2 the constant 1234.567"""
    name, B, H, W, C, groups = sw
    x = normal((B, H * W, C), RB.case_seed(name), "sweep") + float(mu)
    cpg = C // groups
    x[0, :, 0:cpg] = 0.0
    x[0, :, cpg:2 * cpg] = 1.5
    x[0, :, 2 * cpg:3 * cpg] = 1234.567
    gamma = normal((C,), 5, "sweep.gamma", 0.3, 1.0)
    beta = normal((C,), 5, "sweep.beta", 0.2)
    return x, gamma, beta


def sweep_ratio(sw, x, gamma, beta, eps, dtype, hi, lo, k):
    """(worst err / statistics-tier bound over everything, the same over the random groups alone, worst |err| of a normalised value there,
    all-zero and dyadic-constant group exact?) for planes produced from x"""
    name, B, H, W, C, groups = sw
    x64 = x.double()
    mr = stats_of(x64, groups, eps)[0]
    em, drstd = stats_shift(x64, groups, eps, k, fold_terms=C // groups * 64)
    g64, b64 = gamma.double(), beta.double()
    ref = group_norm(x64, None, 0, groups, g64, b64, eps, 0, mean_rstd=mr)
    got = planes_value(hi, lo, dtype)
    err = (got - ref).abs()
    bound = apply_bound(x64, mr, g64, b64, 0, dtype, lo is not None, em, drstd)
    r = ratio(err, bound)
    cpg = C // groups
    rr = ratio(err[:, :, 3 * cpg:], bound[:, :, 3 * cpg:])
    nerr = float((err / g64.abs())[:, :, 3 * cpg:].max())
    bh, bl = _split(beta[:2 * cpg].float(), dtype, lo is not None)       # the all-zero and the dyadic-constant group: y = beta, exactly
    const_ok = torch.equal(got[0, :, :2 * cpg], planes_value(bh, bl, dtype).expand(H * W, 2 * cpg))
    return r, rr, nerr, const_ok
