"""Plain torch restatements of the FiLM (use_scale_shift_norm) GroupNorm kernels - stedm_gn_apply16c_film (gn.hip: the FILM instantiation
of gn_apply16c_v8_kernel, arithmetic in gn_fold.hpp: gn_film / gn_build_table_film) and stedm_gn_bwd_film (gn_bwd.hip) - with their
derived per-element bounds, exact inputs and fp32 emulations with switchable defects. No GPU. Builds on tests/refs_gn.py (same
conventions: tensors flattened to [B, HW, C], u = 2^-24, gamma_k, u_T). Shared by tests/test_gn_film_refs_cpu.py and
tests/test_gpu_gn_film.py.

FORWARD  out = act(z), z = GroupNorm(x) (1 + s) + sh, s / sh [B, C] = film[b * bstride + off + c], film[b * bstride + off + C + c]
  (openaimodel.py:280-284: scale, shift = th.chunk(emb_out, 2, dim=1)). The kernel's order, fp32:
      v = (x - m) * (r * g) + b        the table rows and order of the plain 8-wide kernel: refs_gn's E_pre bounds it,
                                       E_v = |g| rstd (u |mean| + 4u D) (1 + 8u) + u |v|
      p = fl(1 + s)                    one rounding when the table is built: u |1 + s|
      z = v * p + sh                   one product, one sum (a fused multiply-add removes the product's rounding)
  so  E_z = (E_v |1 + s| + 2u |v (1 + s)|) (1 + 8u) + u |z|
  then silu_f and the final 16-bit rounding exactly as in refs_gn.apply_bound (1.1 E_z + silu_bound; u_T |y| or u_T^2 |y| + half-step).
  exact tier: on refs_gn.exact_pattern v = +-g + b is a 5-bit dyadic number; with p in {1/2, 1, 3/2, 2} and sh a multiple of 1/4
  (film_dyadic) z = v p + sh has at most 8 significant bits above 2^-5: exact in fp32 in either contraction and in bf16 / f16, lo == 0.

BACKWARD  with u_ = xh g + b, z = u_ p + sh, dy = dA silu'(z), G = g p (per sample), per (sample, channel) sums U = sum_p dy, W = sum_p dy xh:
      dx = rstd (G dy - m1 - xh m2), m1 / m2 the group means of G dy and G dy xh             (the GroupNorm backward with G for g)
      dshift[b, c] = U;  dscale[b, c] = g W + b U  (dz/ds = u_);  dgamma[c] = sum_b p W;  dbeta[c] = sum_b p U
  film_group_norm_bwd states this in closed form for GIVEN {mean, rstd} (they are an input of the kernel); with exact statistics it
  is the gradient torch.autograd gives through F.group_norm(x) * (1 + s) + sh -> SiLU (pinned in the CPU test).
  Bounds (film_bwd_bounds), in the manner of refs_gn.gn_bwd_bounds, k = refs_gn.gn_bwd_k terms per (sample, channel) sum:
      xh: exh = 2u |xh|;  u_: eu = |g| exh + 2u (|xh g| + |b|);  z: ez = |p| eu + 3u (|u_ p| + |sh|)   (fl(1 + s), product, sum)
      dy: edy = silu_grad_bound(z, dA) + 0.5 |dA| ez;  U, W: gamma_k sum|terms| + the terms' own errors, as in gn_bwd_bounds
      G = fl(g fl(1 + s)): 2u |G|, so the 3u of the group means becomes 5u and the 4u S of dx 6u S
      dshift: e_U;  dscale: |g| e_W + |b| e_U + 3u (|g W| + |b U|)
      dgamma: sum_b |p| (e_W + 2u |W|) + gamma_kb sum_b |p W| (kb = ceil(B / 16) + 17, the sample walk of the parameter kernel); dbeta alike."""
import torch

from tests import refs_bwd as RB
from tests import refs_gn as RG

U, TINY, FILL16 = RG.U, RG.TINY, RG.FILL16


# ------------------------------------------------------------------------------------------------ addressing
def film_rows(film, B, C, bstride, off, defects=()):
    """(scale, shift) [B, 1, C] from the flat fp32 tensor `film`. defects: 'row0' (sample 0's row for every sample), 'swap' (the halves
    swapped), 'no_off' (film_off ignored)"""
    f = film.reshape(-1)
    if "no_off" in defects:
        off = 0
    rows = torch.arange(B) * (0 if "row0" in defects else bstride)
    idx = rows.view(B, 1) + off + torch.arange(C).view(1, C)
    s, sh = f[idx], f[idx + C]
    if "swap" in defects:
        s, sh = sh, s
    return s.unsqueeze(1), sh.unsqueeze(1)


def film_dyadic(B, C, wide=0, off=0):
    """film [B, wide or 2 C] fp32 with scale in {-1/2, 0, 1/2, 1} and shift a multiple of 1/4 in [-1, 1], distinct per sample and channel;
    the columns outside [off, off + 2 C) hold 1000 (a kernel that reads them cannot stay exact)"""
    b = torch.arange(B).view(B, 1)
    c = torch.arange(C).view(1, C)
    s = (((c * 3 + b * 5 + 1) % 4) - 1).float() / 2.0
    sh = (((c * 5 + b * 3 + 2) % 9) - 4).float() / 4.0
    w = wide or 2 * C
    film = torch.full((B, w), 1000.0)
    film[:, off:off + C] = s
    film[:, off + C:off + 2 * C] = sh
    return film.contiguous()


# ------------------------------------------------------------------------------------------------ references (fp64 for a reference)
def film_group_norm(x, groups, gamma, beta, eps, act, s, sh, mean_rstd=None):
    """act(GroupNorm(x) (1 + s) + sh) [B, HW, C]; x flat [B, HW, C], s / sh [B, 1, C]"""
    v = RG.group_norm(x, None, 0, groups, gamma, beta, eps, 0, mean_rstd)
    z = v * (1.0 + s) + sh
    return RB.silu(z) if act else z


def film_group_norm_bwd(x, mean_rstd, groups, gamma, beta, act, s, sh, dA, add=None, old=None):
    """closed form (module docstring). Returns (dx, dgamma [C], dbeta [C], dscale [B, C], dshift [B, C])."""
    B, HW, C = x.shape
    cpg = C // groups
    mean, rstd = RG.per_channel(mean_rstd[..., 0], C), RG.per_channel(mean_rstd[..., 1], C)
    xh = (x - mean) * rstd
    p = 1.0 + s
    z = (xh * gamma + beta) * p + sh
    dy = RB.silu_grad(z, dA) if act else dA
    dxh = dy * gamma * p
    m1 = dxh.view(B, HW, groups, cpg).mean((1, 3))
    m2 = (dxh * xh).view(B, HW, groups, cpg).mean((1, 3))
    dx = rstd * (dxh - RG.per_channel(m1, C) - xh * RG.per_channel(m2, C))
    if add is not None:
        dx = dx + add
    if old is not None:
        dx = dx + old
    Us, Ws = dy.sum(1), (dy * xh).sum(1)
    return dx, (p[:, 0] * Ws).sum(0), (p[:, 0] * Us).sum(0), gamma * Ws + beta * Us, Us


# ------------------------------------------------------------------------------------------------ bounds
def film_apply_bound(x64, mr64, gamma64, beta64, s64, sh64, act, dtype, hilo):
    C = x64.shape[-1]
    mean, rstd = RG.per_channel(mr64[..., 0], C), RG.per_channel(mr64[..., 1], C)
    D = (x64 - mean).abs()
    v = (x64 - mean) * rstd * gamma64 + beta64
    Ev = gamma64.abs() * rstd * (U * mean.abs() + 4.0 * U * D) * (1.0 + 8.0 * U) + U * v.abs()
    p = 1.0 + s64
    z = v * p + sh64
    E = (Ev * p.abs() + 2.0 * U * (v * p).abs()) * (1.0 + 8.0 * U) + U * z.abs()
    y = z
    if act:
        y = RB.silu(z)
        E = 1.1 * E + RB.silu_bound(z.abs() + E, y.abs() + 1.1 * E)
    ut = RG.u_T(dtype)
    return E + (ut * ut if hilo else ut) * (y.abs() + E) + RG.floor_T(dtype) + TINY


def film_bwd_bounds(x64, mr64, groups, gamma64, beta64, s64, sh64, act, dA64, add64, old64, k, dtype=None, hilo=False):
    """Returns dict(dx [B, HW, C], plane (or None), dgamma [C], dbeta [C], dscale [B, C], dshift [B, C]) of per-element bounds."""
    B, HW, C = x64.shape
    cpg = C // groups
    mean, rstd = RG.per_channel(mr64[..., 0], C), RG.per_channel(mr64[..., 1], C)
    xh = (x64 - mean) * rstd
    exh = 2.0 * U * xh.abs()
    p = 1.0 + s64
    G = gamma64 * p                                         # [B, 1, C]
    if act:
        u_ = xh * gamma64 + beta64
        eu = gamma64.abs() * exh + 2.0 * U * ((xh * gamma64).abs() + beta64.abs())
        z = u_ * p + sh64
        ez = p.abs() * eu + 3.0 * U * ((u_ * p).abs() + sh64.abs())
        dy = RB.silu_grad(z, dA64)
        edy = RB.silu_grad_bound(z, dA64) + 0.5 * dA64.abs() * ez
    else:
        dy = dA64
        edy = torch.zeros_like(dA64)
    t2 = dy * xh
    et2 = edy * xh.abs() + (dy.abs() + edy) * exh + U * t2.abs()
    e_u = RG.gam(k) * dy.abs().sum(1) + edy.sum(1)          # [B, C]
    e_w = RG.gam(k + 1) * t2.abs().sum(1) + et2.sum(1)
    n = float(cpg * HW)
    Ga = G.abs()[:, 0]                                      # [B, C]
    e1 = ((e_u * Ga + 5.0 * U * dy.abs().sum(1) * Ga).view(B, groups, cpg).sum(2)) / n
    e2 = ((e_w * Ga + 5.0 * U * t2.abs().sum(1) * Ga).view(B, groups, cpg).sum(2)) / n
    dxh = dy * G
    m1 = RG.per_channel(dxh.view(B, HW, groups, cpg).mean((1, 3)), C)
    m2 = RG.per_channel((dxh * xh).view(B, HW, groups, cpg).mean((1, 3)), C)
    S = dxh.abs() + m1.abs() + (xh * m2).abs()
    e = rstd * (6.0 * U * S + G.abs() * edy + RG.per_channel(e1, C) + m2.abs() * exh + (xh.abs() + exh) * RG.per_channel(e2, C))
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
        ut = RG.u_T(dtype)
        ep = e + (ut * ut if hilo else ut) * (dx.abs() + e) + RG.floor_T(dtype)
    Us, Ws = dy.sum(1), t2.sum(1)
    kb = (B + 15) // 16 + 17
    pa = p.abs()[:, 0]
    e_dg = (pa * (e_w + 2.0 * U * Ws.abs())).sum(0) + RG.gam(kb) * (pa * t2.abs().sum(1)).sum(0) + TINY
    e_db = (pa * (e_u + 2.0 * U * Us.abs())).sum(0) + RG.gam(kb) * (pa * dy.abs().sum(1)).sum(0) + TINY
    e_ds = gamma64.abs() * e_w + beta64.abs() * e_u + 3.0 * U * ((gamma64 * Ws).abs() + (beta64 * Us).abs()) + TINY
    return dict(dx=e, plane=ep, dgamma=e_dg, dbeta=e_db, dscale=e_ds, dshift=e_u + TINY)


# ------------------------------------------------------------------------------------------------ fp32 emulations
def emu_apply16c_film(x, mr32, groups, gamma, beta, film, bstride, off, act, dtype, hilo, defects=()):
    """the FILM body of gn_apply16c_v8_kernel in fp32 (pixel runs and channel runs compute the same values). Returns (hi, lo) int16
    [B, HW, C]. defects: those of film_rows, and 'no_one' (1 + scale taken as scale)"""
    x = RG.flat(x).float()
    B, HW, C = x.shape
    s, sh = film_rows(film.float(), B, C, bstride, off, defects)
    m = RG.per_channel(mr32[..., 0], C)
    r = RG.per_channel(mr32[..., 1], C)
    v = (x - m) * (r * gamma) + beta
    p = s if "no_one" in defects else 1.0 + s
    w = v * p + sh
    if act:
        w = w * torch.sigmoid(w)
    return RG._split(w, dtype, hilo)


def emu_gn_bwd_film(x, mr32, groups, gamma, beta, film, bstride, off, act, dA, add, old, acc, dtype, planes, dgamma0, dbeta0, acc_param,
                    dE0, d_off, defects=()):
    """stedm_gn_bwd_film in fp32 torch. dE0 [B, N]: the matrix before the call (its other columns must survive). Returns
    dict(dx, hi, lo, dgamma, dbeta, dE). defects: those of film_rows, 'no_one', 'dscale_no_beta' (dscale = g W only),
    'dgamma_unweighted' (dgamma = sum_b W)"""
    x = RG.flat(x).float()
    B, HW, C = x.shape
    cpg = C // groups
    s, sh = film_rows(film.float(), B, C, bstride, off, defects)
    p = s if "no_one" in defects else 1.0 + s
    mean, rstd = RG.per_channel(mr32[..., 0], C), RG.per_channel(mr32[..., 1], C)
    xh = (x - mean) * rstd
    dA = RG.flat(dA).float()
    if act:
        z = (xh * gamma + beta) * p + sh
        sg = torch.sigmoid(z)
        dy = dA * (sg * (1.0 + z * (1.0 - sg)))
    else:
        dy = dA
    u = dy.sum(1)
    w = (dy * xh).sum(1)
    G = gamma * p                                             # [B, 1, C]
    n = float(cpg * HW)
    m1 = ((u * G[:, 0]).double().view(B, groups, cpg).sum(2) / n).float()
    m2 = ((w * G[:, 0]).double().view(B, groups, cpg).sum(2) / n).float()
    r = rstd * ((G * dy - RG.per_channel(m1, C)) - xh * RG.per_channel(m2, C))
    if add is not None:
        r = r + RG.flat(add).float()
    if acc:
        r = r + RG.flat(old)
    hi = lo = None
    if planes:
        hi, lo = RG._split(r, dtype, planes == "hilo")
    pw = torch.ones_like(p[:, 0]) if "dgamma_unweighted" in defects else p[:, 0]
    dg = (dgamma0 if acc_param else 0.0) + (pw * w).sum(0)
    db = (dbeta0 if acc_param else 0.0) + (p[:, 0] * u).sum(0)
    dE = dE0.clone()
    dE[:, d_off:d_off + C] = gamma * w + (0.0 if "dscale_no_beta" in defects else beta * u)
    dE[:, d_off + C:d_off + 2 * C] = u
    return dict(dx=r, hi=hi, lo=lo, dgamma=dg, dbeta=db, dE=dE)


# ------------------------------------------------------------------------------------------------ cases shared by the CPU and the GPU tier
# forward: (id, B, H, W, C, groups, hilo, kernel form expected of refs_gn.apply16c_geometry: ('v8', cb > 0?), film layout)
# film layout: (bstride_kind, off): 'row' = each sample its own row of width 2 C + off + 8; 'shared' = bstride 0
FWD = [
    ("cpg1_tiny", 2, 16, 16, 32, 32, False, False, ("row", 0)),           # cpg 1, the TINY net's own width
    ("px_tail", 2, 20, 20, 96, 8, False, False, ("row", 40)),             # pixel runs, tail body only; film_off > 0 inside a wider row
    ("px_full", 3, 32, 32, 512, 32, False, False, ("row", 0)),            # one full iteration, no tail
    ("px_full_tail", 3, 32, 32, 640, 32, False, False, ("shared", 0)),    # full iteration plus tail; film_bstride = 0
    ("hilo", 2, 16, 16, 640, 32, True, False, ("row", 0)),                # hi + lo
    ("chan_runs", 200, 8, 8, 512, 32, False, True, ("row", 0)),           # channel runs, cb = 128
]
FWD_IDS = [c[0] for c in FWD]

# backward: (id, B, H, W, C, groups, expected (cb > 0, ppt) of refs_gn.gn_bwd_fused_cb, act, use_add, acc, acc_param, planes)
BWD = [
    ("ppt2", 2, 8, 8, 64, 32, (True, 2), 1, False, False, False, "hi"),
    ("ppt4", 3, 16, 16, 128, 32, (True, 4), 1, True, True, True, "hilo"),
    ("ppt8", 2, 32, 32, 64, 32, (True, 8), 0, True, False, False, None),
    ("ragged", 2, 10, 10, 96, 8, (True, 4), 1, False, True, True, "hi"),        # 42 pixel lanes over 100 pixels, 3 pixels per thread
    ("chain", 2, 48, 48, 64, 32, (False, 0), 1, True, False, True, "hi"),
]
BWD_IDS = [c[0] for c in BWD]


def film_layout(case_film, B, C):
    """(rows, width, bstride, off) of the flat film tensor of a case"""
    kind, off = case_film
    width = 2 * C + off + 8
    return (1, width, 0, off) if kind == "shared" else (B, width, width, off)


def fwd_film(case, exact, seed=0):
    """the film tensor [rows, width] of a forward case: dyadic for the exact tier, N(0, 0.5) for the bound tier"""
    name, B, H, W, C, groups, hilo, chan, lay = case
    rows, width, bstride, off = film_layout(lay, B, C)
    if exact:
        return film_dyadic(rows, C, width, off)
    return RG.normal((rows, width), seed, f"film.{name}", std=0.5)


def fwd_problem(case, exact, dtype, act=0, eps=1e-5, seed=0):
    """inputs of a forward case and what the kernel must write. Returns dict(x [B, HW, C] fp32, cs (channel partials of x, 256-pixel
    slots), gamma, beta, film [rows, width], bstride, off, eps, act) plus, exact tier: hi (int16 words), mr (fp32 {mean, rstd});
    bound tier: ref / bound (fp64, per element) of the apply tier and mr64 (the fp64 fold of cs, what the kernel's fold rounds)."""
    name, B, H, W, C, groups, hilo, chan, lay = case
    HW = H * W
    rows, width, bstride, off = film_layout(lay, B, C)
    film = fwd_film(case, exact, seed)
    if exact:
        assert act == 0 and eps == 0.0
        x, _, sign, mr = RG.exact_pattern(B, HW, C, 0, 0, groups, "B")
        gamma, beta = RG.dyadic_affine(C)
        s, sh = film_rows(film, B, C, bstride, off)
        y = (sign.float() * gamma + beta) * (1.0 + s) + sh
        assert torch.equal(y.to(dtype).float(), y), "the exact pattern must be representable in the plane format"
        out = dict(hi=y.to(dtype).contiguous().view(torch.int16), mr=mr)
    else:
        x = RG.normal((B, HW, C), seed, f"film.{name}.x", std=1.5, mean=0.3)
        gamma = RG.normal((C,), seed, f"film.{name}.g", std=0.5, mean=1.0)
        beta = RG.normal((C,), seed, f"film.{name}.b", std=0.5)
        out = {}
    cs = RG.chan_partials(x)
    out.update(x=x, cs=cs, gamma=gamma, beta=beta, film=film, bstride=bstride, off=off, eps=eps, act=act)
    if not exact:
        mr64 = RG.fold(cs, None, 0, groups, HW, eps)
        s, sh = film_rows(film.double(), B, C, bstride, off)
        out["mr64"] = mr64
        out["ref"] = film_group_norm(x.double(), groups, gamma.double(), beta.double(), eps, act, s, sh, mean_rstd=mr64)
        out["bound"] = film_apply_bound(x.double(), mr64, gamma.double(), beta.double(), s, sh, act, dtype, hilo)
    return out


def bwd_problem(case, dtype, seed=0):
    """inputs of a backward case, the fp64 closed form on the SAME fp32 {mean, rstd} and its bounds. The film rows sit at offset 8 of rows
    of width 2 C + 24; dE is [B, 2 C + 40] filled with 7.0, the block at columns [16, 16 + 2 C)."""
    name, B, H, W, C, groups, form, act, use_add, acc, acc_param, planes = case
    HW = H * W
    x = RG.normal((B, HW, C), seed, f"filmb.{name}.x", std=1.5, mean=0.3)
    gamma = RG.normal((C,), seed, f"filmb.{name}.g", std=0.5, mean=1.0)
    beta = RG.normal((C,), seed, f"filmb.{name}.b", std=0.5)
    width, off, d_off = 2 * C + 24, 8, 16
    film = RG.normal((B, width), seed, f"filmb.{name}.film", std=0.5)
    dA = RG.normal((B, HW, C), seed, f"filmb.{name}.dA")
    add = RG.normal((B, HW, C), seed, f"filmb.{name}.add") if use_add else None
    old = RG.normal((B, HW, C), seed, f"filmb.{name}.old") if acc else None
    dg0 = RG.normal((C,), seed, f"filmb.{name}.dg0")
    db0 = RG.normal((C,), seed, f"filmb.{name}.db0")
    dE0 = torch.full((B, 2 * C + 40), 7.0)
    mr32 = RG.fold(RG.chan_partials(x), None, 0, groups, HW, 1e-5).float()
    s, sh = film_rows(film.double(), B, C, width, off)
    d = lambda t: None if t is None else t.double()
    dx, dg, db, dsc, dsh = film_group_norm_bwd(x.double(), mr32.double(), groups, gamma.double(), beta.double(), act, s, sh, dA.double(),
                                               d(add), d(old))
    if acc_param:
        dg, db = dg + dg0.double(), db + db0.double()
    k = RG.gn_bwd_k(C, 0, groups, HW)
    bounds = film_bwd_bounds(x.double(), mr32.double(), groups, gamma.double(), beta.double(), s, sh, act, dA.double(), d(add), d(old), k,
                             dtype if planes else None, planes == "hilo")
    if acc_param:       # the accumulate: one more rounded sum
        bounds["dgamma"] = bounds["dgamma"] + U * (dg.abs() + dg0.double().abs())
        bounds["dbeta"] = bounds["dbeta"] + U * (db.abs() + db0.double().abs())
    return dict(x=x, mr32=mr32, gamma=gamma, beta=beta, film=film, bstride=width, off=off, dA=dA, add=add, old=old, dg0=dg0, db0=db0, dE0=dE0,
                d_off=d_off, ref=dict(dx=dx, dgamma=dg, dbeta=db, dscale=dsc, dshift=dsh), bounds=bounds)


def bwd_ratios(case, prob, out, dtype):
    """worst err / bound of every output of a backward case; out: dict(dx, hi, lo, dgamma, dbeta, dE) as emu_gn_bwd_film returns it. The
    columns of dE outside the block must still hold their fill (ratio inf otherwise)."""
    C = case[4]
    planes = case[11]
    ref, bd, d_off = prob["ref"], prob["bounds"], prob["d_off"]
    r = {}
    r["dx"] = ratio(out["dx"].double() - ref["dx"], bd["dx"])
    if planes:
        r["plane"] = ratio(RG.planes_value(out["hi"], out["lo"], dtype) - ref["dx"], bd["plane"])
    r["dgamma"] = ratio(out["dgamma"].double() - ref["dgamma"], bd["dgamma"])
    r["dbeta"] = ratio(out["dbeta"].double() - ref["dbeta"], bd["dbeta"])
    dE = out["dE"].double()
    r["dscale"] = ratio(dE[:, d_off:d_off + C] - ref["dscale"], bd["dscale"])
    r["dshift"] = ratio(dE[:, d_off + C:d_off + 2 * C] - ref["dshift"], bd["dshift"])
    keep = torch.ones(dE.shape[1], dtype=torch.bool)
    keep[d_off:d_off + 2 * C] = False
    r["fill"] = 0.0 if torch.equal(out["dE"][:, keep], prob["dE0"][:, keep]) else float("inf")
    return r


def ratio(err, bound):
    """worst |err| / bound; NaN or inf in err counts as inf"""
    return RG.ratio(err.abs(), bound)
