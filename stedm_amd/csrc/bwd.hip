// Backward-pass kernels of the training step (p_losses ddpm.py:1015-1048 under autograd, i.e. the reverse
// of UNetModel.forward openaimodel.py:761-806). The two heavy contractions of every convolution's backward run on the forward's
// own MFMA convolution kernels: dgrad = the same convolution with the flipped / transposed filter; wgrad = one GEMM
// dW[(tap, ci)][co] = sum_p col[(tap, ci)][p] * dY^T[co][p] over "transposed im2col" planes written here. This unit holds those planes and
// the HBM-bound fp32 helpers around the contractions: the weight-gradient and bias folds, the resampling backward, the small GEMM's
// split-K reduce, SiLU, axpby, q_sample, the two losses, the SpatialRescaler weight gradient and the SpatialTransformer pieces (LayerNorm,
// GEGLU). GroupNorm backward is gn_bwd.hip, attention backward attn_bwd.hip, the gradient norm and AdamW / EMA opt.hip.
// No atomics: every reduction has a fixed order, gradients are bitwise reproducible.
#include "common.hpp"
#include "sgemm.hpp"
#include "silu_bwd.hpp"

using namespace stedm;

namespace {

// ------------------------------------------------------------------------------------------------ transposed im2col (16-bit)
// src [B][Hs][Ws][C] 16-bit NHWC -> dst [(tap*C + c)][Ppad], p = (b*Ho + y)*Wo + x over the OUTPUT grid of the convolution;
// mode 0: stride 1 (Ho = Hs); 1: nearest-2x upsample then conv (Ho = 2Hs); 2: stride 2 (Ho = Hs/2). ks 1 or 3 (pad ks/2).
// grid (Ppad/64, ceil(C/64), taps), 256 threads: a 64-pixel x 64-channel tile goes through LDS.
__global__ void __launch_bounds__(256) im2col_t16_kernel(const uint16_t* __restrict__ src, uint16_t* __restrict__ dst, int B, int Hs, int Ws, int C, int Ho,
                                                         int Wo, int ks, int mode, long P, long Ppad) {
  __shared__ uint16_t tile[64][72];
  const int tap = blockIdx.z, ky = tap / ks - ks / 2, kx = tap % ks - ks / 2;
  const long p0 = (long)blockIdx.x * 64;
  const int c0 = blockIdx.y * 64;
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int e = threadIdx.x + it * 256, pl = e >> 3, cq = (e & 7) * 8;
    const long p = p0 + pl;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (p < P && c0 + cq < C) {
      const int x = (int)(p % Wo), y = (int)((p / Wo) % Ho), b = (int)(p / ((long)Wo * Ho));
      int sy, sx; bool ok;
      if (mode == 1) { const int uy = y + ky, ux = x + kx; ok = uy >= 0 && uy < Ho && ux >= 0 && ux < Wo; sy = uy >> 1; sx = ux >> 1; }
      else if (mode == 2) { sy = 2 * y + ky; sx = 2 * x + kx; ok = sy >= 0 && sy < Hs && sx >= 0 && sx < Ws; }
      else { sy = y + ky; sx = x + kx; ok = sy >= 0 && sy < Hs && sx >= 0 && sx < Ws; }
      if (ok) v = *reinterpret_cast<const uint4*>(src + (((long)b * Hs + sy) * Ws + sx) * C + c0 + cq);
    }
    *reinterpret_cast<uint4*>(&tile[pl][cq]) = v;
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int e = threadIdx.x + it * 256, cl = e >> 3, pq = (e & 7) * 8;
    if (c0 + cl >= C) continue;
    uint16_t r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = tile[pq + j][cl];
    uint4 v;
    v.x = r[0] | ((uint32_t)r[1] << 16); v.y = r[2] | ((uint32_t)r[3] << 16);
    v.z = r[4] | ((uint32_t)r[5] << 16); v.w = r[6] | ((uint32_t)r[7] << 16);
    *reinterpret_cast<uint4*>(dst + ((long)tap * C + c0 + cl) * Ppad + p0 + pq) = v;
  }
}

// dw [taps][cin_ld][cout_ld] fp32 (GEMM result) -> grad OIHW [cout][cin][taps] (+= when accumulate).
// grid (ceil(cout/32), ceil(cin/CIT)): a [taps][CIT ci][32 co] block goes through LDS: 128-B runs in, (CIT ci x taps)-float runs out.
// CIT = 16; 4 for small filters with many split-K partials (128 -> 128: a 4 x 8 grid of blocks walked 32 partials serially in 20 us).
template <int CIT>
__global__ void __launch_bounds__(256) wgrad_to_oihw_kernel(const float* __restrict__ dw, float* __restrict__ grad, int cout, int cin, int taps, int cin_ld,
                                                            int cout_ld, int accumulate, int nsplit) {
  __shared__ float tile[9 * CIT][33];
  constexpr int SH = CIT == 16 ? 4 : 2;
  const int co0 = blockIdx.x * 32, ci0 = blockIdx.y * CIT;
  if ((cout_ld & 3) == 0 && co0 + 32 <= cout && (reinterpret_cast<uintptr_t>(dw) & 15) == 0) {
    // 16-B loads along co (8 lanes cover a 128-B run): a quarter of the load instructions, four times the bytes in flight per lane
    for (int e = threadIdx.x; e < taps * CIT * 8; e += 256) {
      const int c4 = e & 7, r = e >> 3;               // r = tap * CIT + ci_local
      const int tap = r >> SH, cil = r & (CIT - 1);
      const int ci = ci0 + cil;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ci < cin)
#pragma unroll 8
        for (int z = 0; z < nsplit; ++z) {            // split-K partials, fixed order
          const float4 w = *reinterpret_cast<const float4*>(dw + (((long)z * taps + tap) * cin_ld + ci) * cout_ld + co0 + c4 * 4);
          v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w;
        }
      tile[r][c4 * 4] = v.x; tile[r][c4 * 4 + 1] = v.y; tile[r][c4 * 4 + 2] = v.z; tile[r][c4 * 4 + 3] = v.w;
    }
  } else
  for (int e = threadIdx.x; e < taps * CIT * 32; e += 256) {
    const int col = e & 31, r = e >> 5;               // r = tap * CIT + ci_local
    const int tap = r >> SH, cil = r & (CIT - 1);
    const int co = co0 + col, ci = ci0 + cil;
    float v = 0.f;
    if (co < cout && ci < cin)
#pragma unroll 4
      for (int z = 0; z < nsplit; ++z) v += dw[(((long)z * taps + tap) * cin_ld + ci) * cout_ld + co];    // split-K partials, fixed order
    tile[r][col] = v;
  }
  __syncthreads();
  const int run = CIT * taps;                         // contiguous floats of one output row: [ci0 .. ci0+CIT-1][taps]
  for (int e = threadIdx.x; e < 32 * run; e += 256) {
    const int col = e / run, k = e - col * run;       // k = ci_local * taps + tap
    const int cil = k / taps, tap = k - cil * taps;
    const int co = co0 + col, ci = ci0 + cil;
    if (co < cout && ci < cin) {
      const long o = ((long)co * cin + ci) * taps + tap;
      grad[o] = (accumulate ? grad[o] : 0.f) + tile[tap * CIT + cil][col];
    }
  }
}

// cs [B][nslab][C][2] (sums in [..][0]) -> per_sample[b*ld + c] (optional) and total[c] (+= when accumulate; optional)
// grid ceil(C/16); 256 threads = 16 channels x 16 sample lanes (pure load latency: few samples per lane, their loads in flight together;
// fixed-order fold of the 16 lanes through LDS)
__global__ void __launch_bounds__(256) chan_sum_fold_kernel(const float* __restrict__ cs, int B, int nslab, int C, float* __restrict__ per_sample, long ld,
                                                            float* __restrict__ total, int accumulate, float* __restrict__ total2) {
  __shared__ float red[16][16];
  const int cl = threadIdx.x & 15, bl = threadIdx.x >> 4, c = blockIdx.x * 16 + cl;
  float tot = 0.f;
  if (c < C) {
    int b = bl;
    for (; b + 48 < B; b += 64) {
      float u[4] = {0.f, 0.f, 0.f, 0.f};
      for (int k = 0; k < nslab; ++k) {
#pragma unroll
        for (int i = 0; i < 4; ++i) u[i] += cs[(((long)(b + 16 * i) * nslab + k) * C + c) * 2];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (per_sample) per_sample[(long)(b + 16 * i) * ld + c] = u[i];
        tot += u[i];
      }
    }
    for (; b < B; b += 16) {
      float u = 0.f;
      for (int k = 0; k < nslab; ++k) u += cs[(((long)b * nslab + k) * C + c) * 2];
      if (per_sample) per_sample[(long)b * ld + c] = u;
      tot += u;
    }
  }
  red[bl][cl] = tot;
  __syncthreads();
  if (bl == 0 && c < C && total) {
    float t = 0.f;
#pragma unroll
    for (int l = 0; l < 16; ++l) t += red[l][cl];   // fixed order
    const float v = (accumulate ? total[c] : 0.f) + t;
    total[c] = v;
    if (total2) total2[c] = v;      // a second parameter with the same gradient (two biases added onto one tensor)
  }
}

// ------------------------------------------------------------------------------------------------ resampling
// out[b][y][x][c] (+)= sum of the 2x2 block of in [B][2H][2W][C]  (backward of the nearest-neighbour 2x upsample)
__global__ void sum2x2_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int Q, int accumulate, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int q = (int)(i % Q), x = (int)((i / Q) % W), y = (int)((i / ((long)Q * W)) % H), b = (int)(i / ((long)Q * W * H));
  const float4* p = reinterpret_cast<const float4*>(in) + (((long)b * 2 * H + 2 * y) * 2 * W + 2 * x) * Q + q;
  const float4 a0 = p[0], a1 = p[Q], a2 = p[(long)2 * W * Q], a3 = p[(long)2 * W * Q + Q];
  float4 r = make_float4(a0.x + a1.x + a2.x + a3.x, a0.y + a1.y + a2.y + a3.y, a0.z + a1.z + a2.z + a3.z, a0.w + a1.w + a2.w + a3.w);
  float4* o = reinterpret_cast<float4*>(out) + i;
  if (accumulate) { const float4 v = *o; r.x += v.x; r.y += v.y; r.z += v.z; r.w += v.w; }
  *o = r;
}

// 16-bit planes [B][2Ho][2Wo][C]: value of in[b][y/2][x/2][c] at even (y, x), zero elsewhere (dgrad of a stride-2 convolution
// is the stride-1 convolution of this zero-inserted gradient with the flipped filter)
template <typename T>
__global__ void zero_insert16_kernel(const float* __restrict__ in, T* __restrict__ hi, T* __restrict__ lo, int Ho, int Wo, int Q, long total) {
  typedef T V4 __attribute__((ext_vector_type(4)));
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;   // over the [B][2Ho][2Wo][Q] output
  if (i >= total) return;
  const int q = (int)(i % Q), x = (int)((i / Q) % (2 * Wo)), y = (int)((i / ((long)Q * 2 * Wo)) % (2 * Ho)), b = (int)(i / ((long)Q * 4 * Wo * Ho));
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!(x & 1) && !(y & 1)) v = reinterpret_cast<const float4*>(in)[(((long)b * Ho + (y >> 1)) * Wo + (x >> 1)) * Q + q];
  V4 h; h[0] = (T)v.x; h[1] = (T)v.y; h[2] = (T)v.z; h[3] = (T)v.w;
  reinterpret_cast<V4*>(hi)[i] = h;
  if (lo) {
    V4 l; l[0] = (T)(v.x - (float)h[0]); l[1] = (T)(v.y - (float)h[1]); l[2] = (T)(v.z - (float)h[2]); l[3] = (T)(v.w - (float)h[3]);
    reinterpret_cast<V4*>(lo)[i] = l;
  }
}

// ------------------------------------------------------------------------------------------------ small fp32 GEMM
// C[M][N] = alpha * op(A) op(B) + beta * C; op(A)[m][k] = ta ? A[k*lda + m] : A[m*lda + k]; op(B)[k][n] = tb ? B[n*ldb + k] : B[k*ldb + n]
// (the tiled kernel is sgemm.hpp's; this unit holds the fixed-order reduce of its split-K slices)
__global__ void gemm_f32_reduce_kernel(const float* __restrict__ part, int ks, float* __restrict__ Cm, long ldc, int M, int N, float alpha, float beta) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)M * N) return;
  float s = 0.f;
  for (int z = 0; z < ks; ++z) s += part[(long)z * M * N + i];   // fixed order
  const long o = (i / N) * ldc + (i % N);
  Cm[o] = alpha * s + (beta != 0.f ? beta * Cm[o] : 0.f);
}

// mode 0: out = silu(x); mode 1: out = dy * silu'(x)
__global__ void silu_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ out, long n, int mode) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = mode == 0 ? silu_tail_f(x[i]) : dy[i] * silu_grad(x[i]);
}

// y = alpha * x + beta * y (gradient accumulation over micro-batches: accumulate_grad_batches of the reference's Trainer)
__global__ void axpby_kernel(const float* __restrict__ x, float* __restrict__ y, long n4, float alpha, float beta) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const float4 a = reinterpret_cast<const float4*>(x)[i];
  float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
  if (beta != 0.f) b = reinterpret_cast<float4*>(y)[i];      // beta = 0 starts an accumulation window: y may hold anything (NaN included), as in BLAS
  b.x = alpha * a.x + beta * b.x; b.y = alpha * a.y + beta * b.y; b.z = alpha * a.z + beta * b.z; b.w = alpha * a.w + beta * b.w;
  reinterpret_cast<float4*>(y)[i] = b;
}

// q_sample (ddpm.py:277-280 + extract_into_tensor util.py:96-99): out = sqrt_ac[t[b]] * x0 + sqrt_1mac[t[b]] * noise; n = elements per sample
__global__ void q_sample_kernel(const float* __restrict__ x0, const float* __restrict__ noise, const int64_t* __restrict__ t, const float* __restrict__ sa,
                                const float* __restrict__ s1, float* __restrict__ out, long n, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int64_t tb = t[i / n];
  out[i] = __fadd_rn(__fmul_rn(sa[tb], x0[i]), __fmul_rn(s1[tb], noise[i]));     // two products then a sum, like the reference (no FMA contraction)
}

// ------------------------------------------------------------------------------------------------ loss
// L1 (ddpm.py:282-295, 1030-1040): loss = mean |target - pred|; dpred = sign(pred - target) * scale / n
__global__ void __launch_bounds__(256) l1_partial_kernel(const float* __restrict__ pred, const float* __restrict__ target, float* __restrict__ dpred, long n,
                                                         float gscale, double* __restrict__ part) {
  __shared__ double red[256];
  double s = 0.0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float d = pred[i] - target[i];
    s += (double)fabsf(d);
    if (dpred) dpred[i] = d > 0.f ? gscale : (d < 0.f ? -gscale : 0.f);
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}
__global__ void l1_final_kernel(const double* __restrict__ part, int nb, double inv_n, float* __restrict__ loss) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < nb; ++i) s += part[i];
    *loss = (float)(s * inv_n);
  }
}

// The reference's full objective (ddpm.py:1015-1048) on the eps prediction, pred / target [B][n]:
//   ls_b = mean_i f(target - pred), f = |.| (kind 0) or (.)^2 (kind 1);  lv_b = logvar[t_b]
//   loss = lsw * mean_b(ls_b exp(-lv_b) + lv_b) + ew * mean_b(lvlb[t_b] ls_b)
// One pass: d_pred[b][i] = c_b f'(pred - target) with c_b = (lsw exp(-lv_b) + ew lvlb[t_b]) gscale / (B n) formed in fp64 and narrowed once (it does
// not depend on the sums); f' = sign (0 at 0) or 2 d. blockIdx.y = sample, blockIdx.x strides over its n elements; fp64 partial per (sample, block).
constexpr int DL_THREADS = 256;
constexpr int DL_ELEMS = 1024;        // elements per block before the stride loop goes round again
constexpr int DL_MAX_BLOCKS = 64;     // blocks per sample
static int dl_blocks(long n) {
  const long b = (n + DL_ELEMS - 1) / DL_ELEMS;
  return (int)(b > DL_MAX_BLOCKS ? DL_MAX_BLOCKS : b);
}
__global__ void __launch_bounds__(DL_THREADS) diffusion_loss_partial_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                            const int64_t* __restrict__ t, const float* __restrict__ logvar,
                                                                            const float* __restrict__ lvlb, float* __restrict__ dpred, long n, int kind,
                                                                            double lsw, double ew, double gscale, double* __restrict__ part) {
  __shared__ double red[DL_THREADS];
  const int b = blockIdx.y;
  const long base = (long)b * n;
  float cb = 0.f;
  if (dpred) {
    const int64_t tb = t[b];
    cb = (float)((lsw * exp(-(double)logvar[tb]) + ew * (double)lvlb[tb]) * gscale / ((double)gridDim.y * (double)n));
  }
  double s = 0.0;
  for (long i = (long)blockIdx.x * DL_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * DL_THREADS) {
    const double dd = (double)pred[base + i] - (double)target[base + i];       // exact; (float)dd is the fp32 difference
    const float d = (float)dd;
    s += kind == 0 ? fabs(dd) : dd * dd;
    if (dpred) dpred[base + i] = kind == 0 ? (d > 0.f ? cb : (d < 0.f ? -cb : 0.f)) : (2.f * d) * cb;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = DL_THREADS / 2; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) part[(long)b * gridDim.x + blockIdx.x] = red[0];
}
// Finishing launch (one block): ls_b from the partials in block order, the four scalars in fp64 (narrowed once each), and
//   d_logvar[k] = lsw gscale / B * sum_{b: t_b = k} (1 - ls_b exp(-logvar[k])), b in index order (no atomics: duplicates in t are the normal case);
// every one of the T entries is written, those no t_b names with 0.
__global__ void __launch_bounds__(DL_THREADS) diffusion_loss_final_kernel(const double* __restrict__ part, int nbs, const int64_t* __restrict__ t,
                                                                          const float* __restrict__ logvar, const float* __restrict__ lvlb, int B, int T,
                                                                          long n, double lsw, double ew, double gscale, double* __restrict__ ls,
                                                                          float* __restrict__ d_logvar, float* __restrict__ out) {
  for (int b = threadIdx.x; b < B; b += DL_THREADS) {
    double s = 0.0;
    for (int j = 0; j < nbs; ++j) s += part[(long)b * nbs + j];
    ls[b] = s / (double)n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, g = 0.0, v = 0.0;
    for (int b = 0; b < B; ++b) {
      const int64_t tb = t[b];
      const double lv = (double)logvar[tb];
      a += ls[b];
      g += ls[b] * exp(-lv) + lv;
      v += (double)lvlb[tb] * ls[b];
    }
    a /= (double)B; g /= (double)B; v /= (double)B;
    out[0] = (float)(lsw * g + ew * v);
    out[1] = (float)a;
    out[2] = (float)g;
    out[3] = (float)v;
  }
  if (!d_logvar) return;
  for (int k = threadIdx.x; k < T; k += DL_THREADS) {
    double acc = 0.0, e = 0.0;
    bool hit = false;
    for (int b = 0; b < B; ++b) {
      if (t[b] != (int64_t)k) continue;
      if (!hit) { e = exp(-(double)logvar[k]); hit = true; }
      acc += 1.0 - ls[b] * e;
    }
    d_logvar[k] = hit ? (float)(lsw * gscale / (double)B * acc) : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------ SpatialRescaler
// SpatialRescaler (encoders/modules.py:123-130) weight gradient: dW[co][ci] = sum_{b,p} d_out[b][co][p] * boxmean_f(x)[b][ci][p].
// grid B (one block per sample, per-sample partials), then a fixed-order sum over the batch.
__global__ void __launch_bounds__(256) rescale_wgrad_partial_kernel(const float* __restrict__ x, const float* __restrict__ d_out, float* __restrict__ part, int cin,
                                                                    int cout, int H, int W, int f) {
  __shared__ float red[256];
  const int b = blockIdx.x, Ho = H / f, Wo = W / f, np = Ho * Wo;
  for (int e = 0; e < cin * cout; ++e) {
    const int co = e / cin, ci = e % cin;
    float s = 0.f;
    for (int p = threadIdx.x; p < np; p += 256) {
      const int yo = p / Wo, xo = p % Wo;
      const float* px = x + (((long)b * cin + ci) * H + (long)yo * f) * W + (long)xo * f;
      float m = 0.f;
      for (int dy = 0; dy < f; ++dy)
        for (int dx = 0; dx < f; ++dx) m += px[(long)dy * W + dx];
      s += d_out[((long)b * cout + co) * np + p] * (m / (float)(f * f));
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) part[(long)b * cin * cout + e] = red[0];
    __syncthreads();
  }
}
__global__ void rescale_wgrad_final_kernel(const float* __restrict__ part, int B, int n, float* __restrict__ dw, int accumulate) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += part[(long)b * n + e];
  dw[e] = (accumulate ? dw[e] : 0.f) + s;
}

}  // namespace

// ================================================================================================ C ABI
extern "C" int stedm_spatial_rescale_wgrad(const float* x, const float* d_out, float* ws, float* dw, int B, int cin, int cout, int H, int W, int n_stages,
                                           int accumulate, void* stream) {
  STEDM_CHECK_ARG(x && d_out && ws && dw && n_stages >= 0 && n_stages < 8 && cin * cout <= 1024, "spatial_rescale_wgrad: bad args");
  const int f = 1 << n_stages;
  STEDM_CHECK_ARG(H % f == 0 && W % f == 0, "spatial_rescale_wgrad: H, W must be divisible by 2^n_stages");
  rescale_wgrad_partial_kernel<<<B, 256, 0, as_stream(stream)>>>(x, d_out, ws, cin, cout, H, W, f);
  rescale_wgrad_final_kernel<<<(cin * cout + 63) / 64, 64, 0, as_stream(stream)>>>(ws, B, cin * cout, dw, accumulate);
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int stedm_im2col_t16(const void* src16, void* dst16, int B, int Hs, int Ws, int C, int ks, int mode, long Ppad, void* stream) {
  STEDM_CHECK_ARG(src16 && dst16 && C % 8 == 0 && (ks == 1 || ks == 3) && mode >= 0 && mode <= 2 && Ppad % 64 == 0, "im2col_t16: bad args");
  const int Ho = mode == 1 ? 2 * Hs : (mode == 2 ? Hs / 2 : Hs), Wo = mode == 1 ? 2 * Ws : (mode == 2 ? Ws / 2 : Ws);
  const long P = (long)B * Ho * Wo;
  STEDM_CHECK_ARG(Ppad >= P, "im2col_t16: Ppad < P");
  dim3 grid((unsigned)(Ppad / 64), (C + 63) / 64, ks * ks);
  im2col_t16_kernel<<<grid, 256, 0, as_stream(stream)>>>((const uint16_t*)src16, (uint16_t*)dst16, B, Hs, Ws, C, Ho, Wo, ks, mode, P, Ppad);
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int stedm_wgrad_to_oihw(const float* dw, float* grad, int cout, int cin, int taps, int cin_ld, int cout_ld, int accumulate, int nsplit,
                                   void* stream) {
  STEDM_CHECK_ARG(dw && grad && cin_ld >= cin && cout_ld >= cout && nsplit >= 1, "wgrad_to_oihw: bad args");
  STEDM_CHECK_ARG(taps >= 1 && taps <= 9, "wgrad_to_oihw: taps must be 1..9");
  if (((cout + 31) / 32) * ((cin + 15) / 16) < 128 && nsplit >= 4)     // few blocks, long serial walks: quarter tiles
    wgrad_to_oihw_kernel<4><<<dim3((cout + 31) / 32, (cin + 3) / 4), 256, 0, as_stream(stream)>>>(dw, grad, cout, cin, taps, cin_ld, cout_ld, accumulate, nsplit);
  else
    wgrad_to_oihw_kernel<16><<<dim3((cout + 31) / 32, (cin + 15) / 16), 256, 0, as_stream(stream)>>>(dw, grad, cout, cin, taps, cin_ld, cout_ld, accumulate, nsplit);
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int stedm_chan_sum_fold2(const float* cs, int B, int nslab, int C, float* per_sample, long ld, float* total, int accumulate, float* total2,
                                    void* stream) {
  STEDM_CHECK_ARG(cs && (per_sample || total) && (total || !total2), "chan_sum_fold: bad args");
  chan_sum_fold_kernel<<<(C + 15) / 16, 256, 0, as_stream(stream)>>>(cs, B, nslab, C, per_sample, ld, total, accumulate, total2);
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int stedm_chan_sum_fold(const float* cs, int B, int nslab, int C, float* per_sample, long ld, float* total, int accumulate, void* stream) {
  return stedm_chan_sum_fold2(cs, B, nslab, C, per_sample, ld, total, accumulate, nullptr, stream);
}

extern "C" int stedm_sum2x2(const float* in, float* out, int B, int H, int W, int C, int accumulate, void* stream) {
  STEDM_CHECK_ARG(in && out && C % 4 == 0, "sum2x2: bad args");
  const long total = (long)B * H * W * (C / 4);
  sum2x2_kernel<<<(unsigned)((total + 255) / 256), 256, 0, as_stream(stream)>>>(in, out, H, W, C / 4, accumulate, total);
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int stedm_zero_insert16(const float* in, void* hi, void* lo, int B, int Ho, int Wo, int C, int mm_dtype, void* stream) {
  STEDM_CHECK_ARG(in && hi && C % 4 == 0 && (mm_dtype == STEDM_F16 || mm_dtype == STEDM_BF16), "zero_insert16: bad args");
  const long total = (long)B * 4 * Ho * Wo * (C / 4);
  const unsigned grid = (unsigned)((total + 255) / 256);
  if (mm_dtype == STEDM_F16) zero_insert16_kernel<_Float16><<<grid, 256, 0, as_stream(stream)>>>(in, (_Float16*)hi, (_Float16*)lo, Ho, Wo, C / 4, total);
  else zero_insert16_kernel<__bf16><<<grid, 256, 0, as_stream(stream)>>>(in, (__bf16*)hi, (__bf16*)lo, Ho, Wo, C / 4, total);
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int stedm_gemm_f32(const float* A, long lda, int trans_a, const float* Bm, long ldb, int trans_b, float* Cm, long ldc, int M, int N, int K, float alpha,
                              float beta, float* ws, long ws_floats, void* stream) {
  STEDM_CHECK_ARG(A && Bm && Cm && M > 0 && N > 0 && K > 0, "gemm_f32: bad args");
  const int tiles = ((N + 63) / 64) * ((M + 63) / 64);
  int ks = 1;
  if (ws && tiles < 128 && K >= 1024) {          // few output tiles, long K: slices of K on separate blocks, fixed-order reduce
    ks = K / 256 < 64 ? K / 256 : 64;
    while (ks > 1 && (long)ks * M * N > ws_floats) --ks;
  }
  const int kchunk = ks > 1 ? ((K + ks - 1) / ks + 31) / 32 * 32 : K;
  if (ks > 1) ks = (K + kchunk - 1) / kchunk;
  stedm::SgemmArgs g{A, lda, trans_a, Bm, ldb, trans_b, Cm, ldc, M, N, K, alpha, beta, kchunk, ws, nullptr, 0, 0};
  stedm::sgemm_launch(g, ks, as_stream(stream));
  if (ks > 1) gemm_f32_reduce_kernel<<<(unsigned)(((long)M * N + 255) / 256), 256, 0, as_stream(stream)>>>(ws, ks, Cm, ldc, M, N, alpha, beta);
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int stedm_silu(const float* x, const float* dy, float* out, long n, int mode, void* stream) {
  STEDM_CHECK_ARG(x && out && (mode == 0 || dy), "silu: bad args");
  silu_kernel<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(x, dy, out, n, mode);
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int stedm_axpby_f32(const float* x, float* y, long n, float alpha, float beta, void* stream) {
  STEDM_CHECK_ARG(x && y && n > 0 && n % 4 == 0 && ((uintptr_t)x % 16 == 0) && ((uintptr_t)y % 16 == 0), "axpby_f32: n %% 4 and 16-B alignment required");
  axpby_kernel<<<(unsigned)((n / 4 + 255) / 256), 256, 0, as_stream(stream)>>>(x, y, n / 4, alpha, beta);
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int stedm_q_sample(const float* x0, const float* noise, const int64_t* t, const float* sqrt_ac, const float* sqrt_1mac, float* out, int B, long n,
                              void* stream) {
  STEDM_CHECK_ARG(x0 && noise && t && sqrt_ac && sqrt_1mac && out && B > 0 && n > 0, "q_sample: bad args");
  const long total = (long)B * n;
  q_sample_kernel<<<(unsigned)((total + 255) / 256), 256, 0, as_stream(stream)>>>(x0, noise, t, sqrt_ac, sqrt_1mac, out, n, total);
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int stedm_l1_loss(const float* pred, const float* target, long n, float grad_scale, float* d_pred, double* ws, float* loss, void* stream) {
  STEDM_CHECK_ARG(pred && target && ws && loss && n > 0, "l1_loss: bad args");
  const int nb = (int)((n + 256 * 16 - 1) / (256 * 16) < 1024 ? (n + 256 * 16 - 1) / (256 * 16) : 1024);
  l1_partial_kernel<<<nb, 256, 0, as_stream(stream)>>>(pred, target, d_pred, n, grad_scale / (float)n, ws);
  l1_final_kernel<<<1, 64, 0, as_stream(stream)>>>(ws, nb, 1.0 / (double)n, loss);
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int stedm_diffusion_loss_blocks(long n) { return n > 0 ? dl_blocks(n) : 0; }

extern "C" int stedm_diffusion_loss(const float* pred, const float* target, const int64_t* t, const float* logvar, const float* lvlb, int B, long n, int T,
                                    int kind, double l_simple_weight, double elbo_weight, double grad_scale, float* d_pred, float* d_logvar, double* ws,
                                    long ws_doubles, float* out, void* stream) {
  STEDM_CHECK_ARG(pred && target && t && logvar && lvlb && ws && out && B > 0 && B <= 65535 && n > 0 && T > 0 && (kind == 0 || kind == 1),
                  "diffusion_loss: bad args");
  const int nbs = dl_blocks(n);
  STEDM_CHECK_ARG(ws_doubles >= (long)B * (nbs + 1), "diffusion_loss: ws needs B * (stedm_diffusion_loss_blocks(n) + 1) doubles");
  diffusion_loss_partial_kernel<<<dim3(nbs, B), DL_THREADS, 0, as_stream(stream)>>>(pred, target, t, logvar, lvlb, d_pred, n, kind, l_simple_weight,
                                                                                     elbo_weight, grad_scale, ws);
  diffusion_loss_final_kernel<<<1, DL_THREADS, 0, as_stream(stream)>>>(ws, nbs, t, logvar, lvlb, B, T, n, l_simple_weight, elbo_weight, grad_scale,
                                                                        ws + (long)B * nbs, d_logvar, out);
  STEDM_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------ SpatialTransformer backward pieces
// LayerNorm backward over rows of `dim` (BasicTransformerBlock.norm1/2/3, attention.py:205-215): xh = (x - mean) rstd, dxh = dy gamma,
//   dx = add + rstd (dxh - mean(dxh) - xh mean(dxh xh));   dgamma = sum_rows dy xh, dbeta = sum_rows dy.
// One wave per row (a lane holds dim / 64 <= 32 elements); a block of 4 waves walks its rows and leaves ONE partial row of (dgamma | dbeta)
// in part[block][2][dim]; ln_bwd_fold adds the blocks in a fixed order.
namespace {
__global__ void __launch_bounds__(256) ln_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ gamma, float eps,
                                                     const float* add, float* dx, float* __restrict__ part, long rows, int dim, int rows_per_block) {
  constexpr int NV = 32;
  __shared__ float sp[4][2][2048];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float dg[NV], db[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) { dg[j] = 0.f; db[j] = 0.f; }
  const long r0 = (long)blockIdx.x * rows_per_block;
  const long r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
  for (long row = r0 + wave; row < r1; row += 4) {
    const float* px = x + row * dim;
    const float* pd = dy + row * dim;
    float xv[NV], dv[NV];
    float s1 = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int k = lane + 64 * j;
      xv[j] = k < dim ? px[k] : 0.f;
      dv[j] = k < dim ? pd[k] : 0.f;
      s1 += xv[j];
    }
    const float mean = wave_sum(s1) / dim;
    float s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) { const float d = lane + 64 * j < dim ? xv[j] - mean : 0.f; s2 += d * d; }
    const float rstd = 1.0f / sqrtf(wave_sum(s2) / dim + eps);
    float a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int k = lane + 64 * j;
      if (k < dim) {
        const float xh = (xv[j] - mean) * rstd;
        const float dxh = dv[j] * gamma[k];
        a1 += dxh; a2 += dxh * xh;
        dg[j] += dv[j] * xh; db[j] += dv[j];
        xv[j] = xh; dv[j] = dxh;
      }
    }
    const float m1 = wave_sum(a1) / dim, m2 = wave_sum(a2) / dim;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int k = lane + 64 * j;
      if (k < dim) {
        float v = rstd * (dv[j] - m1 - xv[j] * m2);
        if (add) v += add[row * dim + k];
        dx[row * dim + k] = v;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int k = lane + 64 * j;
    if (k < dim) { sp[wave][0][k] = dg[j]; sp[wave][1][k] = db[j]; }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * dim; i += 256) {
    const int w = i / dim, k = i - w * dim;
    part[((long)blockIdx.x * 2 + w) * dim + k] = sp[0][w][k] + sp[1][w][k] + sp[2][w][k] + sp[3][w][k];     // fixed order
  }
}

__global__ void __launch_bounds__(256) ln_bwd_fold_kernel(const float* __restrict__ part, int nblk, int dim, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                          int accumulate) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * dim) return;
  const int w = i / dim, k = i - w * dim;
  float s = 0.f;
  for (int b = 0; b < nblk; ++b) s += part[((long)b * 2 + w) * dim + k];     // fixed order
  float* d = w == 0 ? dgamma : dbeta;
  d[k] = accumulate ? d[k] + s : s;
}

// GEGLU backward (attention.py:37-44: out = value * gelu(gate), exact erf GELU): g [M][2 I] = (value | gate), dh [M][I] -> dg [M][2 I]
__global__ void __launch_bounds__(256) geglu_bwd_kernel(const float* __restrict__ g, const float* __restrict__ dh, float* __restrict__ dg, long M, int I) {
  const long total = M * I;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long row = i / I;
    const int c = (int)(i - row * I);
    const float val = g[row * 2 * I + c], gate = g[row * 2 * I + I + c], d = dh[i];
    const float cdf = 0.5f * (1.0f + erff(gate * 0.70710678118654752f));
    const float pdf = 0.3989422804014327f * __expf(-0.5f * gate * gate);
    dg[row * 2 * I + c] = d * gate * cdf;
    dg[row * 2 * I + I + c] = d * val * (cdf + gate * pdf);
  }
}
}  // namespace

extern "C" int stedm_ln_bwd_blocks(long rows) { return (int)((rows + 63) / 64 < 2048 ? (rows + 63) / 64 : 2048); }

extern "C" int stedm_ln_bwd(const float* x, const float* dy, const float* gamma, float eps, const float* add, float* dx, float* dgamma, float* dbeta,
                            float* ws, long rows, int dim, int accumulate, void* stream) {
  STEDM_CHECK_ARG(x && dy && gamma && dx && dgamma && dbeta && ws && rows > 0, "ln_bwd: bad args");
  STEDM_CHECK_ARG(dim > 0 && dim <= 2048, "ln_bwd: rows of up to 2048 channels (dim=%d)", dim);
  const int nblk = stedm_ln_bwd_blocks(rows);
  const int rpb = (int)((rows + nblk - 1) / nblk);
  const int nb = (int)((rows + rpb - 1) / rpb);
  ln_bwd_kernel<<<nb, 256, 0, as_stream(stream)>>>(x, dy, gamma, eps, add, dx, ws, rows, dim, rpb);
  STEDM_LAUNCH_CHECK();
  ln_bwd_fold_kernel<<<(2 * dim + 255) / 256, 256, 0, as_stream(stream)>>>(ws, nb, dim, dgamma, dbeta, accumulate);
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int stedm_geglu_bwd(const float* g, const float* dh, float* dg, long M, int I, void* stream) {
  STEDM_CHECK_ARG(g && dh && dg && M > 0 && I > 0, "geglu_bwd: bad args");
  const long total = M * I;
  const int grid = (int)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
  geglu_bwd_kernel<<<grid, 256, 0, as_stream(stream)>>>(g, dh, dg, M, I);
  STEDM_LAUNCH_CHECK();
  return 0;
}
