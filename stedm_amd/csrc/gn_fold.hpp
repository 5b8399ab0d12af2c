// GroupNorm statistics from channel partials, stated once: the {sum, sumsq} -> {mean, rstd} formula, the block fold of the partials
// of a virtual concat [x1 | x2] with its summation order, the per-channel table of the 8-wide apply kernels with the fp16 guard's
// switch for the normalised planes, the FiLM modulation of scale-shift-norm blocks (gn_film) and the 16-bit hi / lo split. gn.hip (the apply kernels), gn_bwd.hip (gn_fold_kernel) and the
// convolution epilogues that normalise their own output (conv_io.hip, conv_rs.inc) must agree bit for bit; they do so by calling this.
#pragma once
#include "common.hpp"

namespace stedm {

// mean = su / n and rstd = 1 / sqrt(var + eps), var = sq / n - mean^2 clamped at 0 (fp32 partials can leave it negative), in double
// with the reciprocal inv_n = 1 / n as a factor; both results are rounded to fp32 once.
__device__ __forceinline__ void gn_mean_rstd(double su, double sq, double inv_n, float eps, float& mean, float& rstd) {
  const double m = su * inv_n;
  double var = sq * inv_n - m * m;
  var = var > 0.0 ? var : 0.0;
  mean = (float)m;
  rstd = (float)(1.0 / sqrt(var + (double)eps));
}

// A value beyond the fp16 range (65 504) in a run of pixels makes that run's sum of squares exceed 65 504^2 = 4.29e9: a block whose channel
// partials all stay below the threshold cannot overflow and skips the per-element test of its stream (NaN / inf partials fail the `<` too).
#define STEDM_F16_SQ_SAFE 4.0e9f

// The channel partials {sum, sumsq} of one virtual concat: channels [0, c1) in cs1[B][nslab1][c1][2], the rest in cs2[B2][nslab2][c2][2]
// (the tensors may be partitioned into different slot counts); C = c1 + c2 channels in `groups` groups over HW pixels.
struct GnPartials {
  const float* cs1; int nslab1, c1;
  const float* cs2; int nslab2, c2;
  int groups, HW;
  float eps;
  float* mr;     // optional [B][groups][2] = {mean, rstd}
};

// The fold, for a 256-thread block and the groups [g_lo, g_lo + ng) of sample b (cs2 rows of sample b2), ng <= 64. THE ORDER every
// site that folds the same statistics reproduces: entry e = slab * cpg + channel of the group; lane l of the group's L = 256 / ng lanes
// adds the entries e = l, l + L, ... in double (slots a tensor does not have add nothing); the lanes' doubles are then added in lane
// order and go through gn_mean_rstd. Leaves {mean, rstd} of group g in lmean[g] / lrstd[g] (LDS; a caller that only wants the side
// output passes NULL) and, under write_mr, in p.mr[b][g]. dsu / dsq: 256 doubles of LDS each. The values are visible to the block after
// its next barrier. Returns the block-uniform flag "some partial of these groups admits |x| > 65504" (STEDM_F16_SQ_SAFE); a caller with no
// use for it (FLAG = false) gets a plain barrier in place of the block-wide OR.
template <bool FLAG = true>
__device__ __forceinline__ bool gn_fold_block(const GnPartials& p, int b, int b2, int g_lo, int ng, bool write_mr, double* dsu, double* dsq,
                                              float* lmean, float* lrstd) {
  const int cpg = (p.c1 + p.c2) / p.groups;
  const int L = 256 / ng;
  const int gl = threadIdx.x / L, l = threadIdx.x % L, g = g_lo + gl;
  double su = 0.0, sq = 0.0;
  int big = 0;
  if (gl < ng) {
    const int nmax = p.nslab1 > p.nslab2 ? p.nslab1 : p.nslab2;
    const int n = cpg * nmax;
    for (int e = l; e < n; e += L) {
      const int k = e / cpg, c = g * cpg + (e - k * cpg);
      if (c < p.c1) {
        if (k < p.nslab1) { const float* q = p.cs1 + (((long)b * p.nslab1 + k) * p.c1 + c) * 2; su += (double)q[0]; sq += (double)q[1]; big |= !(q[1] < STEDM_F16_SQ_SAFE); }
      } else if (k < p.nslab2) {
        const float* q = p.cs2 + (((long)b2 * p.nslab2 + k) * p.c2 + (c - p.c1)) * 2; su += (double)q[0]; sq += (double)q[1]; big |= !(q[1] < STEDM_F16_SQ_SAFE);
      }
    }
  }
  dsu[threadIdx.x] = su; dsq[threadIdx.x] = sq;
  bool over = false;
  if constexpr (FLAG) over = __syncthreads_or(big) != 0;
  else __syncthreads();
  if (gl < ng && l == 0) {
    double s = 0.0, q = 0.0;
    for (int i = 0; i < L; ++i) { s += dsu[threadIdx.x + i]; q += dsq[threadIdx.x + i]; }
    float mean, rstd;
    gn_mean_rstd(s, q, 1.0 / ((double)cpg * p.HW), p.eps, mean, rstd);
    if (lmean) { lmean[g] = mean; lrstd[g] = rstd; }
    if (p.mr && write_mr) { p.mr[((long)b * p.groups + g) * 2] = mean; p.mr[((long)b * p.groups + g) * 2 + 1] = rstd; }
  }
  return over;
}

// The normalised planes have their own guard switch: |x^| <= sqrt(n) whatever the raw values are, so a plane value can only leave the fp16
// range through gamma / beta (sqrt(n) |gamma| + |beta| > 65504) - small raw values do not rule that out. rn = sqrt(n), n = cpg * HW.
__device__ __forceinline__ int gn_norm_admits_over(float rn, float gamma, float beta) { return !(rn * fabsf(gamma) + fabsf(beta) < 65504.f); }

// Block-uniform: some channel of [0, C) admits a normalised value beyond the fp16 range (always false without `guard`). Its barrier also
// publishes the fold's lmean / lrstd.
__device__ __forceinline__ bool gn_norm_over(const float* gamma, const float* beta, int C, int cpg, int HW, bool guard) {
  int nb = 0;
  if (guard) {
    const float rn = sqrtf((float)cpg * (float)HW);
    for (int c = threadIdx.x; c < C; c += 256) nb |= gn_norm_admits_over(rn, gamma[c], beta[c]);
  }
  return __syncthreads_or(nb) != 0;
}

// The same switch for the channels [c_lo, c_lo + c_n) while building their rows of the LDS table tab[3][C] of the 8-wide kernels:
// tab[c] = mean, tab[C + c] = rstd * gamma, tab[2 C + c] = beta. Waits for the fold's lmean / lrstd first; the table is complete on return.
// gscale: a factor on the plane values after the activation (the 1 / (1 - p) of a dropout pass; |act(z)| <= |z|): the switch is taken on the scaled affine.
__device__ __forceinline__ bool gn_build_table(float* tab, const float* lmean, const float* lrstd, const float* gamma, const float* beta, int C,
                                               int cpg, int HW, int c_lo, int c_n, bool guard, float gscale = 1.0f) {
  __syncthreads();
  int nb = 0;
  const float rn = sqrtf((float)cpg * (float)HW);
  for (int c = c_lo + threadIdx.x; c < c_lo + c_n; c += 256) {
    const int gc = c / cpg;
    const float gmc = gamma[c], btc = beta[c];
    tab[c] = lmean[gc];
    tab[C + c] = lrstd[gc] * gmc;
    tab[2 * C + c] = btc;
    if (guard) nb |= gn_norm_admits_over(rn, gmc * gscale, btc * gscale);
  }
  return __syncthreads_or(nb) != 0;
}

// FiLM (scale-shift norm, openaimodel.py:280-284): the GroupNorm output is modulated per (sample, channel) by the embedding row
// film[b][film_off + c] = scale, film[b][film_off + C + c] = shift (th.chunk(emb_out, 2, dim=1): scale half first). THE ORDER, in fp32:
//   u = (x - mean) * (rstd * gamma) + beta        (the table rows and the order of the plain 8-wide kernels)
//   z = u * (1 + scale) + shift                   (1 + scale rounded to fp32 once, when the table is built)
// No folded affine: u keeps the bits the plain kernel would give, and the backward recomputes z from the same two steps.
__device__ __forceinline__ float gn_film(float x, float mean, float rg, float beta, float one_scale, float shift) {
  const float u = (x - mean) * rg + beta;
  return u * one_scale + shift;
}

// gn_build_table for a FiLM block of sample b: tab[5][C], rows 0 .. 2 as above, tab[3 C + c] = 1 + scale, tab[4 C + c] = shift. The guard's
// switch is evaluated on the sample's effective affine gamma (1 + scale), beta (1 + scale) + shift: a plane value can leave the fp16
// range through scale / shift alone. film_row: the sample's row, already offset (film + b * film_bstride + film_off).
__device__ __forceinline__ bool gn_build_table_film(float* tab, const float* lmean, const float* lrstd, const float* gamma, const float* beta,
                                                    const float* film_row, int C, int cpg, int HW, int c_lo, int c_n, bool guard, float gscale = 1.0f) {
  __syncthreads();
  int nb = 0;
  const float rn = sqrtf((float)cpg * (float)HW);
  for (int c = c_lo + threadIdx.x; c < c_lo + c_n; c += 256) {
    const int gc = c / cpg;
    const float gmc = gamma[c], btc = beta[c];
    const float op = 1.0f + film_row[c], sh = film_row[C + c];
    tab[c] = lmean[gc];
    tab[C + c] = lrstd[gc] * gmc;
    tab[2 * C + c] = btc;
    tab[3 * C + c] = op;
    tab[4 * C + c] = sh;
    if (guard) nb |= gn_norm_admits_over(rn, gmc * op * gscale, (btc * op + sh) * gscale);
  }
  return __syncthreads_or(nb) != 0;
}

// Four fp32 values as 16-bit ones: returns hi = (T)v and, with want_lo, leaves lo = (T)(v - (float)hi), the residual of the first rounding,
// in `lo` (untouched otherwise). want_lo is a flag of its own, not a nullable pointer to the caller's variable: the address of a private
// variable is a per-lane value, and a test of it would be a divergent branch in the middle of a stream.
template <typename T>
using vec4_of = T __attribute__((ext_vector_type(4)));

template <typename T>
__device__ __forceinline__ vec4_of<T> split16(const float4& v, bool want_lo, vec4_of<T>& lo) {
  vec4_of<T> hi;
  hi[0] = (T)v.x; hi[1] = (T)v.y; hi[2] = (T)v.z; hi[3] = (T)v.w;
  if (want_lo) { lo[0] = (T)(v.x - (float)hi[0]); lo[1] = (T)(v.y - (float)hi[1]); lo[2] = (T)(v.z - (float)hi[2]); lo[3] = (T)(v.w - (float)hi[3]); }
  return hi;
}

}  // namespace stedm
