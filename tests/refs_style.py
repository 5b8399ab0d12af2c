"""Plain torch restatements of the small kernels around the style encoders, the VQ first stage and the prediction epilogue (svit.hip,
swin.hip, vq.hip, post.hip, misc.hip), written from the kernel comments, the docstrings of stedm_amd/ops.py and oracle/{style,swin,vq}.py.
Every function runs in the dtype and on the device of its inputs: fp64 is the reference, fp32 pins a bound. Shared by
tests/test_style_refs_cpu.py (pins these functions against independent statements) and tests/test_gpu_style_kernels.py (pins the
kernels against these functions). Generators, U, TINY, split16 and ln_stats are those of tests/refs_bwd.py.

The derived bounds count operations against the magnitudes of the terms (U = 2^-24 per correctly rounded fp32 operation, the hardware
exp / rcp taken as 2U); none of them is taken from a run of a kernel."""
import math

import torch

from tests.refs_bwd import TINY, U, dyadic, ln_stats, normal, split16  # noqa: F401  (re-exported for the two test files)


# ------------------------------------------------------------------------------------------------ 16-bit planes
# hi = the 16-bit rounding of v (half a 16-bit ulp: 2^-11 |v| for f16's 11 significant bits, 2^-8 |v| for bf16's 8), lo = the 16-bit rounding
# of the fp32 remainder v - hi (|v - hi| <= half an ulp, rounded again): hi + lo misses v by 2^-22 |v| (f16) / 2^-16 |v| (bf16), the relative
# size of what the lo plane cannot hold. Below 2^-14 f16 is subnormal with spacing 2^-24: a plane rounds by up to 2^-25 absolute there
# whatever |v| is (bf16 shares fp32's exponent range: 2^-126 stands in for its floor).
def plane_terms(dtype):
    """(pair relative, hi relative, absolute floor) of a 16-bit hi / lo split"""
    if dtype == torch.float16:
        return 2.0 ** -22, 2.0 ** -11, 2.0 ** -25
    assert dtype == torch.bfloat16
    return 2.0 ** -16, 2.0 ** -8, TINY


def pair_bound(ref64, b, dtype):
    """bound of |hi + lo - ref| for a kernel whose fp32 value is within b of ref"""
    p, _, fl = plane_terms(dtype)
    return b + p * (ref64.abs() + b) + fl


def hi_bound(ref64, b, dtype):
    """bound of |hi - ref|: accepts a single rounding of the exact value as well as the rounding of the rounded fp32 value"""
    _, h, fl = plane_terms(dtype)
    return b + h * (ref64.abs() + b) + fl


# ------------------------------------------------------------------------------------------------ LayerNorm forward
def ln(x, g, b, eps):
    xh, _ = ln_stats(x, eps)
    return xh * g + b


# v = (x - mean) rstd g + b with row sums of depth D (a lane's chain + the butterfly steps), as tests/refs_bwd.py counts them:
#   mean:  em = (D + 1) u mean|x|;  rstd: relative er = (D / 2 + 5.5) u;  xh: exh = em rstd + |xh| (er + 2u)
#   v:     |g| exh + u |xh g| + u |v|   (the product with g, the sum with b; an fma only removes a rounding)
# An input that already carries an absolute error ex (the pooled row of svit_head) moves xh to first order by
#   rstd (ex + mean(ex)) + |xh| rstd mean(|xh| ex)        (d mean <= mean(ex); d rstd / rstd = -rstd mean(xh dx))
def ln_fwd_bound(x64, g64, b64, eps, D, ex=None):
    D = float(D)
    xh, rstd = ln_stats(x64, eps)
    em = (D + 1.0) * U * x64.abs().mean(-1, keepdim=True)
    er = (D / 2.0 + 5.5) * U
    exh = em * rstd + xh.abs() * (er + 2.0 * U)
    if ex is not None:
        exh = exh + rstd * (ex + ex.mean(-1, keepdim=True)) + xh.abs() * rstd * (xh.abs() * ex).mean(-1, keepdim=True)
    return g64.abs() * exh + U * (xh * g64).abs() + U * (xh * g64 + b64).abs() + TINY


def ln_D(dim, lanes=64):
    """a lane adds ceil(dim / lanes) elements in a chain, then log2(lanes) butterfly steps"""
    return (dim + lanes - 1) // lanes + int(math.log2(lanes))


# ------------------------------------------------------------------------------------------------ set-ViT patch path
def spt_gather(img, p):
    """img [B, ns, H, W, 3] -> [B, (H/p)(W/p), p p 3 ns]: feature (p1 p + p2) 3 ns + (c ns + s) of token (hp, wp) is img[b, s, hp p + p1, wp p + p2, c]"""
    B, ns, H, W, _ = img.shape
    x = img.reshape(B, ns, H // p, p, W // p, p, 3).permute(0, 2, 4, 3, 5, 6, 1)          # b hp wp p1 p2 c s
    return x.reshape(B, (H // p) * (W // p), p * p * 3 * ns)


def patch_ln(img, p, g, b, eps):
    return ln(spt_gather(img, p), g, b, eps)


def patch_ln_bound(img64, p, g64, b64, eps):
    x = spt_gather(img64, p)
    return ln_fwd_bound(x, g64, b64, eps, ln_D(x.shape[-1]))


def tok_place(tok, pos, cls):
    """tok [B, ntok, dim], pos [ntok + 2, dim], cls [dim] -> x [B, ntok + 2, dim]: x[:, 0] = cls + pos[0], x[:, 1] = 0 + pos[1], x[:, 2 + t] = tok[:, t] + pos[2 + t]"""
    B, ntok, dim = tok.shape
    x = torch.cat([cls.view(1, 1, dim).expand(B, 1, dim), tok.new_zeros((B, 1, dim)), tok], 1)
    return x + pos.view(1, ntok + 2, dim)


def patch_embed(img, p, g, b, eps, wt, bias, pos, cls):
    """SPT: gather, LayerNorm, Linear (wt K-major [pd, dim]) + bias, placed at token 2.. with the position embedding"""
    tok = patch_ln(img, p, g, b, eps) @ wt + bias
    return tok_place(tok, pos, cls)


# the Linear is one fma chain of pd terms per output (pd u of the summed magnitudes) on LayerNorm values that carry ev, then two rounded
# sums (+ bias, + pos); rows 0 and 1 are one rounded sum each and are compared exactly
def patch_embed_bound(img64, p, g64, b64, eps, wt64, bias64, pos64):
    v = patch_ln(img64, p, g64, b64, eps)
    ev = patch_ln_bound(img64, p, g64, b64, eps)
    pd = v.shape[-1]
    mag = v.abs() @ wt64.abs()
    return ev @ wt64.abs() + pd * U * mag + 2.0 * U * (mag + bias64.abs() + pos64[2:].abs().unsqueeze(0)) + TINY


# ------------------------------------------------------------------------------------------------ pooled head
def head_pool(x, pool, c_old=None):
    """x [B, T, dim]; pool 0 mean / 1 cls (token 0) / 2 sum; + c_old"""
    s = x[:, 0] if pool == 1 else (x.sum(1) / x.shape[1] if pool == 0 else x.sum(1))
    return s if c_old is None else s + c_old


def head(x, pool, c_old, g, b, eps, wt, bias):
    """pool, LayerNorm, Linear (wt K-major [dim, ncls])"""
    return ln(head_pool(x, pool, c_old), g, b, eps) @ wt + bias


# pooling: ANY order of adding T terms is within (T - 1) u of the summed magnitudes (lanes, slabs and the scalar chain alike), the division
# and the sum with c_old round once each; the LayerNorm sees that error as ex, its own row sums run over 256 threads (a chain of
# ceil(dim / 256), 6 butterfly steps, 3 adds across the waves); the Linear is an fma chain of dim terms that starts at the bias
def head_bound(x64, pool, c_old64, g64, b64, eps, wt64, bias64):
    B, T, dim = x64.shape
    if pool == 1:
        pre, ep = x64[:, 0], torch.zeros_like(x64[:, 0])
    else:
        mag = x64.abs().sum(1)
        pre = x64.sum(1)
        ep = (T - 1) * U * mag
        if pool == 0:
            pre, ep = pre / T, ep / T + U * (pre / T).abs()
    if c_old64 is not None:
        ep = ep + U * (pre + c_old64).abs()
        pre = pre + c_old64
    D = (dim + 255) // 256 + 9
    ev = ln_fwd_bound(pre, g64, b64, eps, D, ex=ep)
    v = ln(pre, g64, b64, eps)
    return ev @ wt64.abs() + dim * U * (v.abs() @ wt64.abs() + bias64.abs()) + TINY


# ------------------------------------------------------------------------------------------------ aggregation, rescaler
def agg_max(f, n):
    return f.view(-1, n, f.shape[-1]).max(1)[0]


def agg_mean(f, n):
    return f.view(-1, n, f.shape[-1]).mean(1)


def agg_mean_ordered(f, n):
    """the kernel's order: acc = f[0]; acc += f[j], j = 1..n-1; acc / n, every step rounded in f's dtype"""
    v = f.view(-1, n, f.shape[-1])
    acc = v[:, 0].clone()
    for j in range(1, n):
        acc = acc + v[:, j]
    return acc / n


def box_mean(x, f):
    """x [B, C, H, W] -> [B, C, H/f, W/f]: the mean of every f x f box"""
    B, C, H, W = x.shape
    return x.view(B, C, H // f, f, W // f, f).sum((3, 5)) / (f * f)


def rescale(x, w, n_stages):
    """n_stages halvings (== one 2^n x 2^n box mean for sides divisible by 2^n), then the bias-free 1x1 conv w [cout, cin] (None: identity)"""
    m = box_mean(x, 1 << n_stages)
    return m if w is None else torch.einsum("oc,bchw->bohw", w, m)


# the loop as written: the f^2 values of a box are added row-major in one chain ((f^2 - 1) u of their summed magnitudes), divided once
# (exact: f^2 is a power of two; counted u), then one fma per input channel (cin u of the summed |w m|; without w the weights are 1 and 0)
def rescale_bound(x64, w64, n_stages):
    f = 1 << n_stages
    cin = x64.shape[1]
    m, ma = box_mean(x64, f), box_mean(x64.abs(), f)
    em = (f * f - 1) * U * ma + U * m.abs()
    if w64 is None:
        return em + cin * U * m.abs() + TINY
    wa = w64.abs()
    return torch.einsum("oc,bchw->bohw", wa, em) + cin * U * torch.einsum("oc,bchw->bohw", wa, m.abs()) + TINY


# ------------------------------------------------------------------------------------------------ GEGLU -> planes
def gelu_exact(t):
    """t Phi(t) with Phi from erfc on the negative side (1 + erf cancels there)"""
    return 0.5 * t * torch.special.erfc(-t * (1.0 / math.sqrt(2.0)))


def geglu(g):
    """g [M, 2I] = (value | gate) -> value * gelu(gate), exact erf GELU"""
    I = g.shape[-1] // 2
    return g[..., :I] * gelu_exact(g[..., I:])


# The kernel's GELU is 0.5 t (t >= 0 ? 2 - y : y), y = P(s) exp(-x^2) the Abramowitz-Stegun 7.1.26 form of erfc(x), x = |t| / sqrt 2,
# s = 1 / (1 + 0.3275911 x), P(s) = s (a1 + s (a2 + s (a3 + s (a4 + s a5)))); the published bound of that form is |y - erfc x| <= 1.5e-7, absolute.
#   x: rounded constant, rounded product: 2u |x|;  s: fma u, v_rcp_f32 2u, x's error with weight <= 1: relative 5u
#   P: 4 fma and the product with s round at <= A1(s) = sum |a_i| s^i each: 5u A1;  s's error moves P by 5u A2(s), A2 = sum i |a_i| s^i
#   exp(-x^2): x^2 carries 2 x 2u + u, the product with log2 e two more roundings: exp2's argument moves by 7u x^2 / ln 2, its value by
#   7u x^2 relative; v_exp_f32 2u;  the product P e: u |y|
#   |err y| <= e (5 A1 + 5 A2) u + |y| (7 x^2 + 3) u + 1.5e-7;   2 - y: u (2 - y) <= 2u
#   gelu = (0.5 t) (..): |err| <= 0.5 |t| (err y + 2u) + u |gelu|;   out = value gelu: |value| err gelu + u |out|
AS_A = (0.254829592, 0.284496736, 1.421413741, 1.453152027, 1.061405429)
AS_ERR = 1.5e-7


def geglu_bound(g64):
    I = g64.shape[-1] // 2
    val, t = g64[..., :I], g64[..., I:]
    x = t.abs() * (1.0 / math.sqrt(2.0))
    s = 1.0 / (1.0 + 0.3275911 * x)
    A1 = sum(a * s ** (i + 1) for i, a in enumerate(AS_A))
    A2 = sum((i + 1) * a * s ** (i + 1) for i, a in enumerate(AS_A))
    e = torch.exp(-x * x)
    y = torch.special.erfc(x)
    ey = e * (5.0 * A1 + 5.0 * A2) * U + y * (7.0 * x * x + 3.0) * U + AS_ERR
    eg = 0.5 * t.abs() * (ey + 2.0 * U) + U * gelu_exact(t).abs()
    return val.abs() * eg + U * (val * gelu_exact(t)).abs() + TINY


def geglu_tie_inputs():
    """(value, gate) pairs whose product is 1 + 2^-11 + 2^-24 up to sign and a power of two: gates of 8 and more, where the exact GELU is the
    identity in fp32; the fp32 product rounds to an exact f16 tie, so a single rounding of the exact product (1 + 2^-10) and the rounding of
    the rounded product (1.0) differ, and each is right only with the lo taken against it"""
    a = 1.0 + 2.0 ** -12
    rows = []
    for sv in (1.0, -1.0):
        for kv, kg in ((-3, 3), (-2, 3), (-4, 4), (0, 3), (-3, 4)):
            rows.append((sv * a * 2.0 ** kv, a * 2.0 ** kg))
    v = torch.tensor([r[0] for r in rows], dtype=torch.float32)
    t = torch.tensor([r[1] for r in rows], dtype=torch.float32)
    n = (v.numel() + 3) // 4 * 4
    v = torch.cat([v, v[:n - v.numel()]])
    t = torch.cat([t, t[:n - t.numel()]])
    return torch.cat([v, t]).view(1, 2 * n)


# ------------------------------------------------------------------------------------------------ scaled row softmax -> planes
def softmax_scaled(x, scale):
    """softmax(scale * x) over the last dimension, max subtracted"""
    z = x * scale
    e = torch.exp(z - z.max(-1, keepdim=True)[0])
    return e / e.sum(-1, keepdim=True)


def pad_cols(v, ld):
    out = v.new_zeros(v.shape[:-1] + (ld,))
    out[..., :v.shape[-1]] = v
    return out


# e_k = exp2((x_k scale - m) log2 e), m the largest rounded product. Against the exact a_k = z_k - max z (z = x scale):
#   the product and m round at their own magnitudes, the difference at |a_k| (an fma drops one of the three): u (|z_k| + |m| + |a_k|)
#   the product with log2 e: rounded constant, rounded product: 2u |a_k|;  exp2 turns an absolute argument error into a relative one;
#   v_exp_f32 2u:   E_k = u (|z_k| + |m| + 3 |a_k| + 2), growing with the size of the logits
#   s = sum e: sum E_j e_j + D u s, D = ceil(n / 64) + 6;  1 / s: u;  e_k / s as a product: u
#   relative error of p_k <= E_k + sum_j E_j p_j + (D + 2) u;  2^-126 absolute for what v_exp_f32 flushes
def softmax_bound(x64, scale):
    z = x64 * scale
    m = z.max(-1, keepdim=True)[0]
    a = z - m
    p = softmax_scaled(x64, scale)
    E = U * (z.abs() + m.abs() + 3.0 * a.abs() + 2.0)
    D = float(ln_D(x64.shape[-1]))
    return p * (E + (E * p).sum(-1, keepdim=True) + (D + 2.0) * U) + TINY


# ------------------------------------------------------------------------------------------------ first-stage 1x1 conv, epilogue
def conv1x1(x, w, bias):
    """x [B, cin, H, W], w [cout, cin], bias [cout] or None"""
    out = torch.einsum("oc,bchw->bohw", w, x)
    return out if bias is None else out + bias.view(1, -1, 1, 1)


# acc = bias, then one fma per input channel: cin roundings, each at no more than the summed magnitudes; + 1 so that the bound also holds
# for an evaluation that does not fuse (the products then round too, each at its own magnitude: together u of the sum)
def conv1x1_bound(x64, w64, bias64):
    mag = torch.einsum("oc,bchw->bohw", w64.abs(), x64.abs())
    if bias64 is not None:
        mag = mag + bias64.abs().view(1, -1, 1, 1)
    return (x64.shape[1] + 1) * U * mag + TINY


def seg_merge(seg):
    """seg [B, K, H, W] -> [B, H, W, 2] = {class 0, classes 1..K-1 added in class order}"""
    fg = seg[:, 1].clone()
    for k in range(2, seg.shape[1]):
        fg = fg + seg[:, k]
    return torch.stack([seg[:, 0], fg], -1)


def step_set_t(table, idx, B):
    return table[int(idx)].expand(B).clone()


# ------------------------------------------------------------------------------------------------ Swin-V2 non-GEMM pieces
def swin_patch_rows(img):
    """img [N, 3, H, W] -> [N H/4 W/4, 64]: column c 16 + ky 4 + kx of row (n, ty, tx) is img[n, c, 4 ty + ky, 4 tx + kx]; columns 48..63 zero"""
    N, C, H, W = img.shape
    x = img.reshape(N, 3, H // 4, 4, W // 4, 4).permute(0, 2, 4, 1, 3, 5).reshape(N * (H // 4) * (W // 4), 48)
    return pad_cols(x, 64)


def swin_merge(x):
    """x [N, H, W, C] -> [N ceil(H/2) ceil(W/2), 4C]: [x(0,0) | x(1,0) | x(0,1) | x(1,1)] as (dy, dx), zero beyond an odd side"""
    N, H, W, C = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    xp = x.new_zeros((N, 2 * Ho, 2 * Wo, C))
    xp[:, :H, :W] = x
    v = xp.view(N, Ho, 2, Wo, 2, C).permute(0, 1, 3, 4, 2, 5)                              # n yo xo dx dy c
    return v.reshape(N * Ho * Wo, 4 * C)


def swin_ln(y, g, b, eps, res=None, gate=None, rows_per_gate=1):
    """res + gate[row // rows_per_gate] * LayerNorm(y)"""
    v = ln(y, g, b, eps)
    if gate is not None:
        v = v * gate.repeat_interleave(rows_per_gate).view(-1, 1)
    return v if res is None else v + res


# LayerNorm with dim <= 192 on 32 lanes per row (a chain of 12 register slots, 5 butterfly steps), above on 64 lanes (6 steps); then the
# gate (one rounded product) and the residual (one rounded sum). A gate of 0 leaves res untouched: the bound is then u |res| and the test
# asks for bit equality besides.
def swin_ln_bound(y64, g64, b64, eps, res64=None, gate64=None, rows_per_gate=1):
    dim = y64.shape[-1]
    D = 12 + 5 if dim <= 192 else ln_D(dim, 64)
    bv = ln_fwd_bound(y64, g64, b64, eps, D)
    v = ln(y64, g64, b64, eps)
    if gate64 is not None:
        gt = gate64.repeat_interleave(rows_per_gate).view(-1, 1).abs()
        bv = gt * bv + U * gt * v.abs()
        v = v * gate64.repeat_interleave(rows_per_gate).view(-1, 1)
    if res64 is not None:
        bv = bv + U * (v + res64).abs()
    return bv + TINY


def token_mean(x):
    return x.mean(1)


def token_mean_ordered(x):
    """x [N, T, C]: four partials over tokens w, w + 4, ... (each a chain from 0), ((p0 + p1) + p2) + p3, / T, in x's dtype"""
    N, T, C = x.shape
    parts = []
    for w in range(4):
        s = x.new_zeros((N, C))
        for t in range(w, T, 4):
            s = s + x[:, t]
        parts.append(s)
    return (((parts[0] + parts[1]) + parts[2]) + parts[3]) / T


def swin_rpb(cpb, index, heads):
    """cpb [ntab, heads], index [4096] (clamped to the table) -> [heads, 64, 64] = 16 sigmoid(cpb[index])"""
    e = index.clamp(0, cpb.shape[0] - 1)
    return (16.0 * torch.sigmoid(cpb[e])).t().reshape(heads, 64, 64)


# 16 / (1 + exp2(-c log2 e)): the argument (rounded constant, rounded product) moves exp by 2u |c|, v_exp_f32 2u, both enter 1 + e with weight
# e / (1 + e) < 1; the sum u; the division u:  (6 + 2 |c|) u <= 6 (1 + |c|) u relative, the count of silu in tests/refs_bwd.py
def swin_rpb_bound(cpb64, index, heads):
    e = index.clamp(0, cpb64.shape[0] - 1)
    c = cpb64[e].t().reshape(heads, 64, 64)
    return 6.0 * (1.0 + c.abs()) * U * swin_rpb(cpb64, index, heads).abs() + TINY


# ------------------------------------------------------------------------------------------------ inputs of the f16 pair tests
# (shared: the CPU tier counts, on exactly these inputs, the elements whose f16 rounding differs between the fp32 and the fp64 evaluation
# of the reference; ties cannot be placed by hand behind a LayerNorm or a softmax, a large input has them by itself)
PAIR_EPS = 1e-5
PAIR_MIN_FLIPS = 8


def pair_ln_inputs(rows, dim, seed):
    x = normal((rows, dim), seed, "pair.x", std=1.5, mean=0.3)
    g = normal((dim,), seed, "pair.g", std=0.1, mean=1.0)
    b = normal((dim,), seed, "pair.b", std=0.1)
    return x, g, b


PAIR_LN_APPLY = (512, 256)          # the vector form of ln_apply16 (dim % 256 == 0)
PAIR_LN_APPLY_SCALAR = (656, 200)   # its scalar form
PAIR_SWIN_LN = (683, 192)
PAIR_SWIN_LN_WIDE = (342, 384)
PAIR_PATCH = (11, 8, 8, 64, 8)      # B, ns, H, W, patch: 88 tokens of 1536 features
PAIR_SOFTMAX = (512, 256, 0.125)    # rows, n, scale


def pair_patch_inputs():
    B, ns, H, W, p = PAIR_PATCH
    pd = p * p * 3 * ns
    img = normal((B, ns, H, W, 3), 23, "pair.img", std=0.5, mean=0.1)
    return img, normal((pd,), 23, "pair.pg", std=0.1, mean=1.0), normal((pd,), 23, "pair.pb", std=0.1)


def pair_softmax_inputs():
    rows, n, scale = PAIR_SOFTMAX
    return normal((rows, n), 24, "pair.sm", std=8.0), scale


def f16_flips(v32, v64):
    """elements whose f16 rounding differs between the fp32 and the fp64 evaluation (numpy rounds fp64 to f16 in one step; torch goes through fp32)"""
    import numpy as np
    a = v32.detach().cpu().numpy().astype(np.float16)
    b = v64.detach().cpu().numpy().astype(np.float16)
    return int((a != b).sum())


# ------------------------------------------------------------------------------------------------ inputs of the bounded-kernel tests
# (shared, so that the CPU tier holds each bound against fp32 torch on the inputs the GPU tier uses)
LN_EPS = 1e-5
# (B, ns, H, W, patch): tokens per block tg = 1; pw = 6 -> tg = 2; tg = 8 exactly at the 48 KB budget; just over it -> tg = 4;
# patch_dim 144 (no multiple of 64); patch_dim 48 (below one wave)
PATCH_SHAPES = [(2, 1, 8, 8, 8), (1, 2, 16, 48, 8), (2, 8, 8, 64, 8), (1, 9, 8, 64, 8), (2, 3, 8, 12, 4), (1, 1, 4, 4, 4)]


def patch_inputs(shape):
    B, ns, H, W, p = shape
    pd = p * p * 3 * ns
    img = normal((B, ns, H, W, 3), 31, "patch.img", std=0.5, mean=0.1)
    return img, normal((pd,), 31, "patch.g", std=0.1, mean=1.0), normal((pd,), 31, "patch.b", std=0.1)


def embed_inputs(shape, dim):
    B, ns, H, W, p = shape
    pd, ntok = p * p * 3 * ns, (H // p) * (W // p)
    wt = normal((pd, dim), 32, "embed.wt", std=pd ** -0.5)
    return wt, normal((dim,), 32, "embed.bias", std=0.1), normal((ntok + 2, dim), 32, "embed.pos", std=0.5), normal((dim,), 32, "embed.cls")


HEAD_DIMS = (4, 36, 384, 1024, 1028, 6)     # vector pooling with 256 token lanes, idle threads (28 lanes of 9 quads), 2 lanes, 1 lane; scalar: > 1024, % 4
HEAD_TS = (1, 3, 257)
HEAD_NCLS = (1, 5, 300)


def head_inputs(B, T, dim, ncls, dyadic_x=False):
    x = dyadic((B, T, dim), 33) if dyadic_x else normal((B, T, dim), 33, "head.x", std=1.0, mean=0.2)
    return (x, normal((B, dim), 33, "head.c_old"), normal((dim,), 33, "head.g", std=0.1, mean=1.0), normal((dim,), 33, "head.b", std=0.1),
            normal((dim, ncls), 33, "head.wt", std=dim ** -0.5), normal((ncls,), 33, "head.bias", std=0.1))


def rescale_inputs(n_stages, mult):
    f = 1 << n_stages
    return normal((2, 3, f * mult[0], f * mult[1]), 34, "rescale.x", mean=0.3), normal((5, 3), 34, "rescale.w", std=0.5)


GEGLU_SHAPES = [(M, I) for M in (1, 3) for I in (4, 36)] + [(233100, 36)]      # the last: M I / 4 > 8192 x 256, a second grid-stride trip


def geglu_inputs(M, I):
    g = normal((M, 2 * I), 35, "geglu16.g", std=2.0)
    k = min(M * I, 37)
    flat = g[:, I:].reshape(-1).clone()
    flat[:k] = torch.linspace(-9.0, 9.0, k) if k > 1 else torch.tensor([-9.0])
    g[:, I:] = flat.view(M, I)
    return g


SOFTMAX_ROWS = (1, 5)
SOFTMAX_NS = (1, 63, 64, 65, 200)
SOFTMAX_SCALE = 0.375


def softmax_inputs(rows, n):
    """a column slice [:, 3:3 + n] of a wider tensor; the last row spreads its logits over +-80 / scale"""
    wide = normal((rows, n + 7), 36, "softmax.x", std=4.0)
    x = wide[:, 3:3 + n]
    x[rows - 1] = torch.linspace(-80.0, 80.0, n) / SOFTMAX_SCALE if n > 1 else torch.tensor([80.0 / SOFTMAX_SCALE])
    return wide, x


CONV_CH = (1, 3, 4, 16)
CONV_HW = (1, 255, 257)


def conv_inputs(B, cin, cout, HW, dyadic_in=False):
    if dyadic_in:
        return dyadic((B, cin, 1, HW), 37), dyadic((cout, cin), 38), dyadic((cout,), 39)
    return normal((B, cin, 1, HW), 37, "conv.x"), normal((cout, cin), 37, "conv.w", std=0.5), normal((cout,), 37, "conv.b")


SWIN_LN_DIMS = (96, 100, 192, 193, 384, 768)       # 32 lanes per row up to 192, 64 above; 100 and 193 leave a lane tail
SWIN_LN_ROWS = (1, 7, 9)
SWIN_GATE_P = 0.2


def swin_ln_inputs(rows, dim):
    return (normal((rows, dim), 40, "swin_ln.y", std=1.5, mean=0.3), normal((dim,), 40, "swin_ln.g", std=0.1, mean=1.0),
            normal((dim,), 40, "swin_ln.b", std=0.1), normal((rows, dim), 40, "swin_ln.res"))


def swin_gates(n):
    """0, 1 and 1 / (1 - p) in turn"""
    return torch.tensor([(0.0, 1.0, 1.0 / (1.0 - SWIN_GATE_P))[i % 3] for i in range(n)], dtype=torch.float32)


def rpb_inputs(heads, ntab=225):
    g = torch.Generator().manual_seed(41)
    index = torch.randint(0, ntab, (4096,), generator=g)
    index[5], index[77], index[4095] = -3, ntab, ntab + 1000
    return normal((ntab, heads), 41, "rpb.cpb", std=3.0), index
