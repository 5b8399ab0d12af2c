"""Plain torch restatements of the training step's helper kernels (stedm_amd/csrc/bwd.hip; the SiLU arithmetic is silu_bwd.hpp), written from the formulas in the kernel
comments and the docstrings of stedm_amd/ops.py. Every function runs in the dtype and on the device of its inputs: the tests feed
fp64 for a reference, fp32 to pin a reference's own rounding against its bound. Shared by tests/test_bwd_refs_cpu.py (pins these
functions against torch autograd), tests/test_gpu_bwd_kernels.py (pins the kernels against these functions) and
tests/test_gpu_bwd_conv_exact.py (pins the trainer's dgrad / wgrad dispatch against the convolution-backward references).

Also here: the two input generators and the derived error bounds of the kernels that round (u = 2^-24 is the fp32 unit roundoff:
one correctly rounded operation has relative error <= u, "1 ulp" of the hardware exp / rcp is taken as 2u)."""
import math

import torch

from stedm_amd.utils import prng

U = 2.0 ** -24
TINY = 2.0 ** -126          # smallest normal fp32: the absolute floor for results the hardware flushes


# ------------------------------------------------------------------------------------------------ generators
def dyadic(shape, seed):
    """integers in [-8, 8] scaled by 2^-3, fp32. Any fp32 sum of fewer than 2^17 of them (and of their pairwise differences) is exact in
    every order, so a kernel that sums them must match the fp64 sum bit for bit."""
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(-8, 9, tuple(shape), generator=g).to(torch.float32) / 8.0


def normal(shape, seed, name="x", std=1.0, mean=0.0):
    """fp32 N(mean, std) from the project's numpy-Philox recipe (independent of torch's RNG)"""
    return prng.normal(int(seed), name, tuple(shape), std=std, mean=mean)


def finite_bf16_bits(shape, seed):
    """random int16 bit patterns of finite bf16 values (exponent field 0xff replaced), for kernels that only move 16-bit words"""
    g = torch.Generator().manual_seed(int(seed))
    v = torch.randint(0, 1 << 16, tuple(shape), generator=g, dtype=torch.int32)
    v = torch.where((v & 0x7F80) == 0x7F80, v & ~0x4000, v)
    return torch.where(v >= 1 << 15, v - (1 << 16), v).to(torch.int16)


# ------------------------------------------------------------------------------------------------ data movement
def im2col_t(src_nhwc, ks, mode, Ppad):
    """src [B, Hs, Ws, C] -> [(tap * C + c)][Ppad], column p = (b * Ho + y) * Wo + x over the OUTPUT grid of the convolution; tap = ky * ks + kx
    reads the source at offset (ky - ks // 2, kx - ks // 2), zero outside. mode 0: stride 1; 1: nearest 2x upsample, then stride 1;
    2: stride 2 (Ho = Hs // 2). Columns P..Ppad are zero."""
    if mode == 1:
        src_nhwc = src_nhwc.repeat_interleave(2, 1).repeat_interleave(2, 2)
    B, Hs, Ws, C = src_nhwc.shape
    pad = ks // 2
    st = 2 if mode == 2 else 1
    Ho, Wo = (Hs // 2, Ws // 2) if mode == 2 else (Hs, Ws)
    xp = src_nhwc.new_zeros((B, Hs + 2 * pad, Ws + 2 * pad, C))
    xp[:, pad:pad + Hs, pad:pad + Ws] = src_nhwc
    rows = []
    for ky in range(ks):
        for kx in range(ks):
            patch = xp[:, ky:ky + st * (Ho - 1) + 1:st, kx:kx + st * (Wo - 1) + 1:st]          # [B, Ho, Wo, C]
            rows.append(patch.permute(3, 0, 1, 2).reshape(C, B * Ho * Wo))
    col = torch.cat(rows, 0)
    out = col.new_zeros((ks * ks * C, Ppad))
    out[:, :B * Ho * Wo] = col
    return out


def wgrad_to_oihw(dw, cout, cin):
    """dw [nsplit, taps, cin_ld, cout_ld] (split-K partials of the weight-gradient GEMM) -> OIHW [cout, cin, taps]: slices added in order"""
    s = dw[0].clone()
    for z in range(1, dw.shape[0]):
        s = s + dw[z]
    return s[:, :cin, :cout].permute(2, 1, 0).contiguous()


def sum_planes(part):
    """part [nsplit, n] -> [n], slices added in order"""
    s = part[0].clone()
    for z in range(1, part.shape[0]):
        s = s + part[z]
    return s


def chan_sum_fold(cs):
    """cs [B, nslab, C, 2] (sums in [..., 0]) -> (per_sample [B, C], total [C])"""
    per = cs[..., 0].sum(1)
    return per, per.sum(0)


def sum2x2(x, prior=None):
    """x [B, 2H, 2W, C] -> [B, H, W, C]: ((a0 + a1) + a2) + a3 (+ prior), the kernel's own order, in x's dtype"""
    r = ((x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + x[:, 1::2, 0::2]) + x[:, 1::2, 1::2]
    return r if prior is None else r + prior


def zero_insert(x):
    """x [B, Ho, Wo, C] -> [B, 2Ho, 2Wo, C]: x at even (y, x), zero elsewhere"""
    B, Ho, Wo, C = x.shape
    out = x.new_zeros((B, 2 * Ho, 2 * Wo, C))
    out[:, 0::2, 0::2] = x
    return out


def split16(x32, dtype):
    """fp32 -> (hi, lo) 16-bit planes: hi = round-to-nearest-even cast, lo = cast of the fp32 remainder x - hi"""
    hi = x32.to(dtype)
    return hi, (x32 - hi.to(torch.float32)).to(dtype)


# ------------------------------------------------------------------------------------------------ convolution backward
# What UNetTrainer's dispatch (_dgrad / _wgrad / _up_bwd / _down_bwd) must compute, from the formulas: with y = conv(x, w) + bias and
# dy = dL/dy, dW[co][ci][ky][kx] = sum_p x[p * stride + (ky, kx) - pad][ci] dy[p][co], dx[q][ci] = sum_(k, co) dy[(q - k + pad) / stride][co]
# w[co][ci][k] (terms whose quotient is not a pixel of dy vanish), dbias[co] = sum_p dy[p][co]. Not written with torch.nn.grad.
def wgrad_ref(src_nhwc, dy_nhwc, ks, mode):
    """src [B, Hs, Ws, cin], dy [B, Ho, Wo, cout] (the convolution's output grid) -> dW OIHW [cout, cin, ks, ks]: the transposed im2col of
    the source times the flat gradient. mode as im2col_t: 0 stride 1, 1 nearest 2x then stride 1, 2 stride 2."""
    B, Ho, Wo, cout = dy_nhwc.shape
    cin = src_nhwc.shape[-1]
    P = B * Ho * Wo
    dw = (im2col_t(src_nhwc, ks, mode, P) @ dy_nhwc.reshape(P, cout)).view(1, ks * ks, cin, cout)
    return wgrad_to_oihw(dw, cout, cin).view(cout, cin, ks, ks)


def dgrad_ref(dy_nhwc, w_oihw):
    """dy [B, H, W, cout], w OIHW [cout, cin, ks, ks] -> dx [B, H, W, cin] of the stride-1 convolution with padding ks // 2: the stride-1
    convolution of dy with the flipped, transposed filter, one matmul per tap. Stride 2: dgrad_ref(zero_insert(dy), w); nearest-2x
    upsample in front of the convolution: sum2x2(dgrad_ref(dy, w))."""
    B, H, W, cout = dy_nhwc.shape
    co, cin, ks, _ = w_oihw.shape
    assert co == cout
    pad = ks // 2
    dyp = dy_nhwc.new_zeros((B, H + 2 * pad, W + 2 * pad, cout))
    dyp[:, pad:pad + H, pad:pad + W] = dy_nhwc
    acc = None
    for ky in range(ks):
        for kx in range(ks):
            # dx[q] takes w[k] from dy[q - k + pad]: row q - ky + pad of dy is row q - ky + 2 pad of the padded plane
            patch = dyp[:, 2 * pad - ky:2 * pad - ky + H, 2 * pad - kx:2 * pad - kx + W]
            t = patch.reshape(-1, cout) @ w_oihw[:, :, ky, kx]
            acc = t if acc is None else acc + t
    return acc.view(B, H, W, cin)


def bias_ref(dy_nhwc):
    """the bias gradient: the sum over batch and pixels"""
    return dy_nhwc.sum((0, 1, 2))


def backward_dyadic_ok(K):
    """proof obligation of a bit-exact backward case on `dyadic` data: values are multiples of 1/8 of magnitude <= 1, products multiples of
    1/64 of magnitude <= 1, and every fp32 partial sum of K of them is exact in every order while 64 K <= 2^24. dgrad: K = taps * cout;
    wgrad: K = the total pixel count; + 1 for a prior value of an accumulated output (itself a multiple of 1/8, <= 1)."""
    assert 64 * K <= 2 ** 24, K


# tier-2 data of the dispatch tests, and the shapes of their tier-2 cases (B, H, W of the convolution's INPUT grid, cin -> cout of the forward
# convolution, ks[, mode]); shared so that the CPU tier holds the bound against fp32 torch on the GPU tier's own shapes and inputs
def t2_act(shape, seed):
    """silu(1.3 x + 0.1), x ~ N(0, 1): stands for a normalised + activated activation"""
    return silu(1.3 * normal(shape, seed, "bwd.act") + 0.1)


def t2_grad(shape, seed):
    return normal(shape, seed, "bwd.dy", std=0.1)


def t2_weight(shape_oihw, seed, K):
    return normal(shape_oihw, seed, "bwd.w", std=1.0 / math.sqrt(K))


DGRAD_T2 = {"d_frag_rs": (25, 32, 32, 32, 64, 3), "d_frag_rs_full": (48, 32, 32, 32, 64, 3), "d_frag_lds": (3, 8, 8, 32, 64, 3),
            "d_frag_lds_declined": (129, 8, 8, 32, 64, 3), "d_m16": (97, 16, 16, 64, 288, 3), "d_m16_small": (2, 8, 8, 128, 256, 3),
            "d_m16_full": (769, 8, 8, 32, 256, 3), "d_splitk": (2, 8, 8, 64, 1024, 3)}
DGRAD_T2_PARITY = {"d_parity_frag_lds": (3, 8, 8, 32, 64, 3)}
WGRAD_T2 = {"w_direct_n": (2, 32, 32, 128, 64, 3, 0), "w_gemm_frag": (2, 8, 8, 64, 96, 3, 0), "w_chunks": (5, 128, 128, 32, 32, 3, 0)}
WGRAD_T2_PARITY = {"w_parity_nofrag": (2, 8, 8, 64, 96, 3, 0), "w_parity_nofrag_ragged": (3, 10, 10, 64, 96, 3, 0),
                   "w_parity_mode2": (2, 16, 16, 64, 64, 3, 2)}


def case_seed(name):
    return 100 * sum(ord(ch) for ch in name)


def wgrad_out_hw(H, W, mode):
    return (2 * H, 2 * W) if mode == 1 else ((H // 2, W // 2) if mode == 2 else (H, W))


def dgrad_t2_inputs(name, shape):
    """(dy fp32 [B, H, W, cout], w fp32 OIHW) of a tier-2 dgrad case"""
    B, H, W, cin, cout, ks = shape
    s = case_seed(name)
    return t2_grad((B, H, W, cout), s), t2_weight((cout, cin, ks, ks), s + 1, ks * ks * cout)


def wgrad_t2_inputs(name, shape):
    """(src fp32 [B, H, W, cin], dy fp32 [B, Ho, Wo, cout]) of a tier-2 wgrad case"""
    B, H, W, cin, cout, ks, mode = shape
    s = case_seed(name)
    Ho, Wo = wgrad_out_hw(H, W, mode)
    return t2_act((B, H, W, cin), s), t2_grad((B, Ho, Wo, cout), s + 1)


# ------------------------------------------------------------------------------------------------ SpatialTransformer backward
def ln_stats(x, eps):
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps)
    return xc * rstd, rstd


def ln_bwd(x, dy, gamma, eps, add=None):
    """rows of x / dy [rows, dim]: xh = (x - mean) rstd, dxh = dy gamma, dx = add + rstd (dxh - mean(dxh) - xh mean(dxh xh));
    dgamma = sum_rows dy xh, dbeta = sum_rows dy. Returns (dx, dgamma, dbeta)."""
    xh, rstd = ln_stats(x, eps)
    dxh = dy * gamma
    m1 = dxh.mean(-1, keepdim=True)
    m2 = (dxh * xh).mean(-1, keepdim=True)
    dx = rstd * (dxh - m1 - xh * m2)
    if add is not None:
        dx = dx + add
    return dx, (dy * xh).sum(0), dy.sum(0)


def geglu_bwd(g, dh):
    """g [M, 2I] = (value | gate), out = value * gelu(gate) with the exact erf GELU; dh [M, I] -> dg [M, 2I]"""
    I = g.shape[-1] // 2
    val, gate = g[..., :I], g[..., I:]
    cdf = 0.5 * (1.0 + torch.erf(gate * (1.0 / math.sqrt(2.0))))
    pdf = torch.exp(-0.5 * gate * gate) * (1.0 / math.sqrt(2.0 * math.pi))
    return torch.cat([dh * gate * cdf, dh * val * (cdf + gate * pdf)], -1)


def silu(x):
    return x * torch.sigmoid(x)


def silu_grad(x, dy):
    s = torch.sigmoid(x)
    return dy * (s * (1.0 + x * (1.0 - s)))


# ------------------------------------------------------------------------------------------------ loss
def q_sample(x0, noise, t, sa, s1):
    """sa[t[b]] * x0 + s1[t[b]] * noise: two rounded products, then one rounded sum, in the inputs' dtype"""
    shp = (-1,) + (1,) * (x0.dim() - 1)
    return sa[t].view(shp) * x0 + s1[t].view(shp) * noise


def l1(pred, target, grad_scale):
    """(loss, d_pred) of mean |target - pred|: loss = float32(sum / n) from an exact fp64 sum, d_pred = sign(pred - target) * float32(grad_scale / n)"""
    n = pred.numel()
    d = pred.double() - target.double()
    loss = (d.abs().sum() / n).to(torch.float32)
    gs = torch.tensor(float(grad_scale) / n, dtype=torch.float64).to(torch.float32)
    return loss, torch.sign(d).to(torch.float32) * gs


# ------------------------------------------------------------------------------------------------ derived bounds
# silu_f(x) = x * rcp(1 + exp2(-x * log2 e)). Errors, in units of u, relative to the result:
#   t = -x * log2(e): the rounded constant and the rounded product move t by <= 2u |t|, i.e. exp2(t) by 2u |t| ln 2 = 2 |x| u
#   v_exp_f32 1 ulp = 2u; 1 + e: u (the error of e enters 1 + e with weight e / (1 + e) < 1); v_rcp_f32 1 ulp = 2u; the product: u
#   sum: (6 + 2 |x|) u <= 6 (1 + |x|) u
# Below x = -64 the kernel scales the denominator by 2^-32 (exp2(t - 32), 2^-32 + e, a last exact product with 2^-32) so that v_rcp_f32's
# result stays normal: the plain form returned 0 at x = -88, 45 times the 2^-126 floor away from -5.3e-37. The count is the same: the
# fused t - 32 is rounded once, at the magnitude of t.
SILU_C = 6.0
# silu_grad(y) = s (1 + y (1 - s)), s = rcp(1 + exp(-y)), then dy * that. With sg = sigmoid(y), M = 1 + |y| (1 - sg):
#   |err s| <= sg u [(1 - sg)(2 + 2 |y|) + 3]                      (exp's error enters with weight 1 - sg; add u, rcp 2u)
#   T = 1 + y (1 - s): |err T| <= |y| |err s| + 2u |y| (1 - sg) + u M    (rounded 1 - s, rounded product, rounded sum)
#   s T, then dy * (s T): |err| <= |err s| (M + sg |y|) + sg |err T|' + 2u sg M, which collects to
#   |err| <= sg M u [6.4 (1 + |y|) + 5] <= 12 (1 + |y|) u * sg * M      (sg |y| <= 0.28 for y < 0; (1 - sg)(1 + y) <= 0.55 for y >= 0)
# The bound is relative to |dy| sg M, the sum of the magnitudes of the two terms of silu', NOT to |silu'(y)|: silu' changes sign at
# y = -1.2785 and the rounding of 1 + y (1 - s) does not shrink with it. For y >= 0 the two are the same number.
SILU_GRAD_C = 12.0


def silu_bound(x64, ref64):
    return SILU_C * (1.0 + x64.abs()) * U * ref64.abs() + TINY


def silu_grad_bound(x64, dy64):
    sg = torch.sigmoid(x64)
    return SILU_GRAD_C * (1.0 + x64.abs()) * U * dy64.abs() * sg * (1.0 + x64.abs() * (1.0 - sg)) + TINY


# geglu_bwd: cdf = 0.5 (1 + erff(gate / sqrt 2)), pdf = c exp(-gate^2 / 2); d_value = d gate cdf, d_gate = d value (cdf + gate pdf).
# erff is taken at the 4 ulp = 8u the HIP math tables give it. The error of cdf is ABSOLUTE: for negative gates 1 + erf cancels, so
# neither output has a relative bound against its reference (cdf(-6) = 1e-9 is below one rounding of 1 + erf):
#   z = gate / sqrt 2 (rounded constant, rounded product: 2u |z|) moves erf by 2u |z| erf'(z) <= u;  erf: 8u;  1 + erf: 2u;  x 0.5 exact
#   |err cdf| <= 0.5 (8 + 1) u + u = 5.5 u
#   d_value = (d * gate) * cdf: two rounded products, 2u |ref| <= 2u |d gate|  ->  |err| <= 7.5 u |d gate|  ->  8
#   pdf: gate^2 / 2 rounded (u), exp of it ((2 + 2 |arg|) u with |arg| = gate^2 / 2), rounded constant and product (2u): relative (5 + 1.5 gate^2) u;
#   gate * pdf: |gate| pdf (6 + 1.5 gate^2) u <= 2.2 u  (max of g phi(g) = 0.242, of g^3 phi(g) = 0.46);  the sum: u |cdf + gate pdf| <= 1.13 u
#   bracket: 5.5 + 2.2 + 1.13 = 8.83 u absolute;  (d * value) * bracket: 2u x 1.13  ->  |err| <= 11.1 u |d value|  ->  12
GEGLU_C_VALUE = 8.0
GEGLU_C_GATE = 12.0


def geglu_bwd_bound(g64, dh64):
    I = g64.shape[-1] // 2
    val, gate = g64[..., :I], g64[..., I:]
    return torch.cat([GEGLU_C_VALUE * U * (dh64 * gate).abs(), GEGLU_C_GATE * U * (dh64 * val).abs()], -1) + TINY


# ln_bwd, one wave per row of n = dim elements: a lane adds its L = ceil(n / 64) elements in a chain, then 6 butterfly steps, so a row sum
# carries <= D u sum|terms| with D = L + 6. With mean|.| the row mean of magnitudes:
#   mean:  em = (D + 1) u mean|x|                                   (sum, divide)
#   rstd:  relative er = (D / 2 + 5.5) u                            (squares 3u, sum D u, / n, + eps, sqrt 1 ulp, 1 / . -> (D + 5) u / 2 + 3u)
#   xh:    |err| <= exh = em rstd + |xh| (er + 2u)
#   m1:    e1 = (D + 2) u mean|dxh|                                 (dxh = dy gamma rounded, sum, divide)
#   m2:    e2 = em rstd mean|dxh| + (er + (D + 5) u) mean|dxh xh|
#   dx = rstd (dxh - m1 - xh m2): with S = |dxh| + |m1| + |xh m2|
#          |err| <= rstd [ S (4u + er) + e1 + |m2| exh + |xh| e2 ]  (+ u (|dx| + |add|) for the rounded sum with add)
# S (4u + er) is the issue's "multiple of 2^-24 rstd (|dxh| + |m1| + |xh m2|)" with the multiple D / 2 + 9.5; e1, |m2| exh and |xh| e2 are
# the summation terms of the three row means.
def _ln_D(dim):
    return (dim + 63) // 64 + 6


def ln_bwd_dx_bound(x64, dy64, gamma64, eps, add64=None):
    D = float(_ln_D(x64.shape[-1]))
    xh, rstd = ln_stats(x64, eps)
    dxh = dy64 * gamma64
    m1 = dxh.mean(-1, keepdim=True)
    m2 = (dxh * xh).mean(-1, keepdim=True)
    em = (D + 1.0) * U * x64.abs().mean(-1, keepdim=True)
    er = (D / 2.0 + 5.5) * U
    exh = em * rstd + xh.abs() * (er + 2.0 * U)
    e1 = (D + 2.0) * U * dxh.abs().mean(-1, keepdim=True)
    e2 = em * rstd * dxh.abs().mean(-1, keepdim=True) + (er + (D + 5.0) * U) * (dxh * xh).abs().mean(-1, keepdim=True)
    S = dxh.abs() + m1.abs() + (xh * m2).abs()
    b = rstd * (S * (4.0 * U + er) + e1 + m2.abs() * exh + xh.abs() * e2)
    if add64 is not None:
        b = b + U * (add64.abs() + rstd * S)
    return b + TINY


def ln_bwd_dgamma_term_bound(x64, dy64, eps):
    """per-element bound of ONE row's term dy xh of dgamma: |dy| exh + u |dy xh| (the rounded product)"""
    D = float(_ln_D(x64.shape[-1]))
    xh, rstd = ln_stats(x64, eps)
    em = (D + 1.0) * U * x64.abs().mean(-1, keepdim=True)
    er = (D / 2.0 + 5.5) * U
    exh = em * rstd + xh.abs() * (er + 2.0 * U)
    return dy64.abs() * exh + U * (dy64 * xh).abs() + TINY


def ln_bwd_param_bounds(x64, dy64, eps, rows_per_block, nblocks, prior_g=None, prior_b=None):
    """worst-case bounds of the column sums (dgamma, dbeta): every row's term bound, plus the summation chain of a column: a wave adds
    ceil(rows_per_block / 4) rows, 3 adds join the waves, nblocks adds join the blocks (+ 1 for the accumulate)"""
    depth = float((rows_per_block + 3) // 4 + 3 + nblocks + 1)
    xh, _ = ln_stats(x64, eps)
    bg = ln_bwd_dgamma_term_bound(x64, dy64, eps).sum(0) + depth * U * (dy64 * xh).abs().sum(0)
    bb = depth * U * dy64.abs().sum(0) + TINY
    if prior_g is not None:
        bg = bg + depth * U * prior_g.abs()
        bb = bb + depth * U * prior_b.abs()
    return bg, bb


# ------------------------------------------------------------------------------------------------ inputs of the rounded-kernel tests
# (shared, so that the CPU tier can hold each bound against fp32 torch on exactly the inputs the GPU tier uses)
SILU_POINTS = [0.0, 1e-8, -1e-8, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0]


def silu_inputs():
    x = torch.cat([normal((1 << 16,), 11, "silu.x", std=4.0), torch.tensor(SILU_POINTS, dtype=torch.float32)])
    dy = normal(x.shape, 11, "silu.dy")
    return x, dy


GEGLU_SHAPES = [(M, I) for M in (1, 3, 4096 * 5 + 1) for I in (1, 320, 1280)]


def geglu_inputs(M, I):
    g = normal((M, 2 * I), 12, "geglu.g", std=3.0)
    k = min(M * I, 193)
    pts = torch.linspace(-12.0, 12.0, k) if k > 1 else torch.tensor([-12.0])
    flat = g[:, I:].reshape(-1).clone()
    flat[:k] = pts                                                   # gate values out to +-12
    g[:, I:] = flat.view(M, I)
    return g, normal((M, I), 12, "geglu.dh")


LN_DIMS = (1, 64, 100, 320, 1280, 2048)
LN_ROWS = (1, 3, 63, 64, 65, 4098)
LN_SHAPES = [(r, d) for d in LN_DIMS for r in LN_ROWS] + [(131072 + 5, 64)]
LN_EPS = 1e-5


def ln_inputs(rows, dim):
    x = normal((rows, dim), 13, "ln.x", std=1.5, mean=0.3)
    dy = normal((rows, dim), 13, "ln.dy")
    gamma = normal((dim,), 13, "ln.gamma", std=0.1, mean=1.0)
    add = normal((rows, dim), 13, "ln.add")
    return x, dy, gamma, add


def ln_block_rows(rows):
    """(rows per block, blocks) of ln_bwd's launch: at most 2048 blocks of at least 64 rows"""
    nblk = min((rows + 63) // 64, 2048)
    rpb = (rows + nblk - 1) // nblk
    return rpb, (rows + rpb - 1) // rpb


L1_NS = (1, 255, 4096, 4097, 1024 * 4096 + 3)


def l1_inputs(n):
    return dyadic((n,), 14), dyadic((n,), 15)
