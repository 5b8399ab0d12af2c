"""The keep-mask stream of the U-Net's ResBlock dropout sites (include/stedm_hip.h, "train-mode dropout": the elementwise stream with the
fourth Philox counter word = the forward counter `step`), restated in numpy on top of oracle.dropmask.philox4x32_10 / thr16, and numpy /
torch references of the drop pass (stedm_gn_apply16c_drop / _film_drop) and of its backward (stedm_gn_bwd_drop / _film_drop). No GPU.
Shared by tests/test_dropout_refs_cpu.py, tests/test_gpu_gn_dropout.py, tests/test_gpu_unet_dropout.py and
tests/golden/make_golden_dropout.py.

  element e = ((b HW + pixel) C + c) of the activation's NHWC linear index keeps iff u16 >= thr16 = lrint(p 65536),
  u16 = field (e & 7) of Philox4x32-10(counter (lo32(e >> 3), hi32(e >> 3), site, step), key (lo32 seed, hi32 seed)), field j = half
  (j & 1) of output word j >> 1; kept values times inv_keep = (float)(1.0 / (1.0 - p)), dropped ones +0; site = 0x55000000 + k.

BOUND of the drop pass (fp32 value -> 16-bit planes). The kernel's value before the mask is the plain pass's w with the plain pass's error
E (refs_gn.apply_bound / refs_gn_film.film_apply_bound without their final rounding term); a kept element is fl(w inv_keep): one more fp32
rounding, then the 16-bit rounding of THAT value. With y the fp64 reference of the kept element (reference activation times the fp32
inv_keep), the plain bound evaluated on the planes of y is  ik E_plain_pre + u |y| + u_T (|y| + ...) + floor; drop_apply_bound states it
as  ik * plain_bound(act value) + 2u |y|, which dominates it (the plain bound already holds u_T (|a| + E) + floor for the activation a,
and ik >= 1 scales the half-step floor up, never down)."""
import numpy as np
import torch

from oracle.dropmask import philox4x32_10, thr16

SITE0 = 0x55000000
MASK32 = np.uint64(0xFFFFFFFF)
U = 2.0 ** -24


def inv_keep(p: float) -> np.float32:
    """(float)(1.0 / (1.0 - p)) with p the C float argument: formed in double, narrowed once"""
    return np.float32(1.0 / (1.0 - float(np.float32(p))))


def keep_mask(n: int, p: float, seed: int, site: int, step: int = 0) -> np.ndarray:
    """bool [n]: the keep mask over the tensor's linear element index"""
    g = np.arange((n + 7) // 8, dtype=np.uint64)
    r = philox4x32_10(g & MASK32, g >> np.uint64(32), np.uint64(site & 0xFFFFFFFF), np.uint64(step & 0xFFFFFFFF), seed & 0xFFFFFFFF,
                      (seed >> 32) & 0xFFFFFFFF)
    u = np.empty((len(g), 8), dtype=np.uint32)
    for j in range(8):
        u[:, j] = (r[j >> 1] >> np.uint32(16 * (j & 1))) & np.uint32(0xFFFF)
    return u.reshape(-1)[:n] >= thr16(p)


def resblock_mask(B: int, HW: int, C: int, p: float, seed: int, k: int, step: int) -> torch.Tensor:
    """bool [B, HW, C] (NHWC order): the mask of the ResBlock with ordinal k at forward counter `step`"""
    assert C % 8 == 0
    return torch.from_numpy(keep_mask(B * HW * C, p, seed, SITE0 + k, step)).view(B, HW, C)


def rank_seed(seed: int, rank: int) -> int:
    """the seed rank `rank` uses under torch.distributed"""
    return (seed ^ ((rank * 0x9E3779B97F4A7C15) % (1 << 64))) % (1 << 64)


# ------------------------------------------------------------------------------------------------ numpy references (fp64)
def _silu(z):
    return z / (1.0 + np.exp(-z))


def _silu_grad(z):
    s = 1.0 / (1.0 + np.exp(-z))
    return s * (1.0 + z * (1.0 - s))


def _stats(x, groups, eps):
    B, HW, C = x.shape
    xg = x.reshape(B, HW, groups, C // groups)
    mean = xg.mean(axis=(1, 3), keepdims=True)
    var = ((xg - mean) ** 2).mean(axis=(1, 3), keepdims=True)
    return xg, mean, 1.0 / np.sqrt(var + eps)


def drop_pass_np(x, gamma, beta, groups, eps, mask, p, scale=None, shift=None):
    """Dropout(SiLU(GroupNorm(x) [(1 + scale) + shift])) in fp64 numpy: x [B, HW, C], mask bool [B, HW, C], scale / shift [B, C] or None"""
    x = np.asarray(x, dtype=np.float64)
    B, HW, C = x.shape
    xg, mean, rstd = _stats(x, groups, eps)
    z = ((xg - mean) * rstd).reshape(B, HW, C) * gamma + beta
    if scale is not None:
        z = z * (1.0 + scale[:, None, :]) + shift[:, None, :]
    return np.where(mask, _silu(z) * float(inv_keep(p)), 0.0)


def drop_pass_bwd_np(x, gamma, beta, groups, eps, mask, p, dA, scale=None, shift=None):
    """the backward of drop_pass_np in closed form (exact statistics): (dx, dgamma [C], dbeta [C], dscale [B, C] or None, dshift or None)"""
    x, dA = np.asarray(x, dtype=np.float64), np.asarray(dA, dtype=np.float64)
    B, HW, C = x.shape
    cpg = C // groups
    xg, mean, rstd = _stats(x, groups, eps)
    xh = ((xg - mean) * rstd).reshape(B, HW, C)
    u = xh * gamma + beta
    pm = np.ones((B, 1, C)) if scale is None else 1.0 + scale[:, None, :]
    z = u * pm + (0.0 if shift is None else shift[:, None, :])
    dy = np.where(mask, dA * float(inv_keep(p)), 0.0) * _silu_grad(z)
    dxh = dy * gamma * pm
    m1 = dxh.reshape(B, HW, groups, cpg).mean(axis=(1, 3), keepdims=True)
    m2 = (dxh * xh).reshape(B, HW, groups, cpg).mean(axis=(1, 3), keepdims=True)
    dx = (rstd * (dxh.reshape(B, HW, groups, cpg) - m1 - xh.reshape(B, HW, groups, cpg) * m2)).reshape(B, HW, C)
    Us, Ws = dy.sum(1), (dy * xh).sum(1)
    dg, db = (pm[:, 0] * Ws).sum(0), (pm[:, 0] * Us).sum(0)
    if scale is None:
        return dx, dg, db, None, None
    return dx, dg, db, gamma * Ws + beta * Us, Us


# ------------------------------------------------------------------------------------------------ kernel-level helpers (torch)
def dA_eff(dA: torch.Tensor, mask: torch.Tensor, p: float) -> torch.Tensor:
    """keep ? dA * inv_keep : +0 as one fp32 multiply (what the DROP backward kernels do with a loaded dA)"""
    ik = torch.tensor(float(inv_keep(p)), dtype=torch.float32, device=dA.device)
    return torch.where(mask.to(dA.device), dA * ik, torch.zeros((), dtype=torch.float32, device=dA.device))


def drop_apply_bound(plain_bound: torch.Tensor, ref_drop: torch.Tensor, p: float) -> torch.Tensor:
    """per-element bound of a kept plane value (module docstring): plain_bound = the plain pass's bound for the same element (fp64)"""
    return float(inv_keep(p)) * plain_bound + 2.0 * U * ref_drop.abs()


def film_bwd_reref(case, prob, dtype, dA32: torch.Tensor):
    """(ref, bounds) of refs_gn_film.bwd_problem recomputed for the gradient dA32 [B, HW, C] in place of the problem's own dA: the fp64
    closed form and the bounds of stedm_gn_bwd_film, unchanged"""
    from tests import refs_gn as RG
    from tests import refs_gn_film as RF
    name, B, H, W, C, groups, form, act, use_add, acc, acc_param, planes = case
    d = lambda t: None if t is None else t.double()
    x64, mr64, g64, b64 = prob["x"].double(), prob["mr32"].double(), prob["gamma"].double(), prob["beta"].double()
    s, sh = RF.film_rows(prob["film"].double(), B, C, prob["bstride"], prob["off"])
    dx, dg, db, dsc, dsh = RF.film_group_norm_bwd(x64, mr64, groups, g64, b64, act, s, sh, dA32.double(), d(prob["add"]), d(prob["old"]))
    if acc_param:
        dg, db = dg + prob["dg0"].double(), db + prob["db0"].double()
    k = RG.gn_bwd_k(C, 0, groups, H * W)
    bounds = RF.film_bwd_bounds(x64, mr64, groups, g64, b64, s, sh, act, dA32.double(), d(prob["add"]), d(prob["old"]), k,
                                dtype if planes else None, planes == "hilo")
    if acc_param:
        bounds["dgamma"] = bounds["dgamma"] + U * (dg.abs() + prob["dg0"].double().abs())
        bounds["dbeta"] = bounds["dbeta"] + U * (db.abs() + prob["db0"].double().abs())
    return dict(dx=dx, dgamma=dg, dbeta=db, dscale=dsc, dshift=dsh), bounds


def doubled_in_range(hi_plain: torch.Tensor, lo_plain, dtype) -> torch.Tensor:
    """bool: the elements whose plane words double exactly (p = 1/2, inv_keep = 2): 2 |v| stays finite and |v| is normal, for the hi word
    and, when given, the lo word. A zero word counts in bf16 only (fp32's exponent range: the fp32 value was zero); an f16 zero may be an
    underflow whose double is not. Normal means ABOVE the smallest normal number: a word equal to it may be a subnormal-range value rounded
    up (spacing 2^-24 in f16), whose double lies in the normal range with half that relative spacing and rounds on its own."""
    def ok(words):
        v = words.view(dtype).float().abs()
        tiny = torch.finfo(dtype).tiny
        zero = (v == 0) if dtype == torch.bfloat16 else torch.zeros_like(v, dtype=torch.bool)
        return (zero | (v > tiny)) & (2.0 * v <= torch.finfo(dtype).max)
    m = ok(hi_plain)
    return m if lo_plain is None else m & ok(lo_plain)
