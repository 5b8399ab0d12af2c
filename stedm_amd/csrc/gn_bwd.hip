// GroupNorm backward of the training step: d act(GroupNorm([x1 | x2])) with the SiLU derivative, the FiLM form of scale-shift-norm blocks and
// the dropout mask of the forward regenerated on load (templates on <T, FILM, DROP>), plus the statistics fold of the forward's channel
// partials (stedm_gn_fold, arithmetic in gn_fold.hpp). HBM-bound fp32 work. Two kernel forms: one pass with the slice in registers, or
// statistics, fold and apply; one host function (gn_bwd_launch) chooses between them for all four entries. The forward is gn.hip.
// No atomics: every reduction has a fixed order, gradients are bitwise reproducible.
#include "common.hpp"
#include "gn_fold.hpp"
#include "dropmask.hpp"
#include "silu_bwd.hpp"

using namespace stedm;

namespace {

// ------------------------------------------------------------------------------------------------ GroupNorm statistics
// chan partials of the (virtual concat) input -> mr[B][groups][2] = {mean, rstd}
// (one block per sample folds all its groups, as a pixel-run block of the forward's apply kernels does: the same bits, gn_fold.hpp)
__global__ void __launch_bounds__(256) gn_fold_kernel(GnPartials p) {
  __shared__ double dsu[256], dsq[256];
  gn_fold_block<false>(p, blockIdx.x, blockIdx.x, 0, p.groups, true, dsu, dsq, nullptr, nullptr);
}

struct GnBwdArgs {
  const float* x1; const float* x2; int c1, c2;
  const float* mr; const float* gamma; const float* beta; const float* dA;   // dA: [B][HW][C] gradient w.r.t. act(GN(x))
  int groups, HW, act;
  float* part;        // [B][nslab][C][2] {sum dy, sum dy*xhat}
  const float* gm;    // [B][groups][2]   {mean_g(gamma*dy), mean_g(gamma*dy*xhat)}
  const float* add;   // optional [B][HW][C] added to dx (the residual / skip branch of the block)
  float* dx1; float* dx2; int acc1, acc2;
  void* o_hi; void* o_lo;   // optional 16-bit planes of dx (operand of the producer convolution's dgrad / wgrad)
  const float* film; long film_bs; int film_off;   // FILM kernels (stedm_gn_bwd_film): sample b's row film + b * film_bs + film_off = {scale[C], shift[C]}
  DropArgs dr;        // DROP kernels (stedm_gn_bwd_drop / _film_drop): the keep mask of the forward's dropout pass, regenerated from the counters
};

// DROP: the activation went through train-mode dropout before the convolution that produced dA (openaimodel.py:241). The first thing a
// thread does with a loaded dA quad is dA_eff = keep ? dA * inv_keep : +0 (drop_quad, dropmask.hpp: one fp32 multiply, the forward's mask
// of element ((b HW + pixel) C + c)); everything after it is the arithmetic of the plain kernels on dA_eff, so the results equal the plain
// entry's on a pre-masked dA bit for bit. The DROP = false instantiations compile to what they were. Needs C % 8 == 0.
template <bool DROP>
__device__ __forceinline__ void gn_bwd_drop4(float (&ds)[4], const GnBwdArgs& a, int b, int pix, int C, int c, uint32_t dstep) {
  if constexpr (DROP) drop_quad(ds[0], ds[1], ds[2], ds[3], (uint64_t)((long)b * a.HW + pix) * (uint64_t)C + (uint64_t)c, a.dr, dstep);
}

// FiLM form (use_scale_shift_norm, openaimodel.py:280-284): z = u (1 + s) + sh with u = xh gamma + beta, the two steps of the forward's
// gn_film; dy = dA silu'(z); dx is the GroupNorm backward with the per-sample weight gamma (1 + s_b) in place of gamma. The FILM = false
// instantiations compile to what they were.
template <bool FILM>
__device__ __forceinline__ float gn_bwd_arg(float xh, float ga, float be, float op, float sh) {
  if constexpr (FILM) return (xh * ga + be) * op + sh;
  else return xh * ga + be;
}

// grid (B, kGnBwdSlab-pixel slabs, blocks of 64 channel quads). 64-pixel slabs: with 256 the grid of a 16x16 x 512-channel tensor at batch 64
// was 128 blocks (half the chip idle, 64 dependent pixel steps per thread)
constexpr int kGnBwdSlab = 64;
template <bool FILM = false, bool DROP = false>
__global__ void __launch_bounds__(256) gn_bwd_stats_kernel(GnBwdArgs a) {
  __shared__ float cpart[256 * 8];
  const int b = blockIdx.x, slab = blockIdx.y, nslab = gridDim.y;
  const int C = a.c1 + a.c2, Q = C >> 2, t = threadIdx.x, cpg = C / a.groups;
  const int qb0 = blockIdx.z * 64, QB = min(64, Q - qb0);
  const int npl = 256 / QB, tq = t % QB, tp = t / QB;
  const int c = (qb0 + tq) * 4;
  const int px0 = min(a.HW, slab * kGnBwdSlab), px1 = min(a.HW, px0 + kGnBwdSlab);
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  if (tp < npl) {
    float mean[4], rstd[4], ga[4], be[4], op[4] = {1.f, 1.f, 1.f, 1.f}, sh[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int g = (c + j) / cpg;
      mean[j] = a.mr[((long)b * a.groups + g) * 2]; rstd[j] = a.mr[((long)b * a.groups + g) * 2 + 1];
      ga[j] = a.gamma[c + j]; be[j] = a.beta[c + j];
      if constexpr (FILM) { const float* fr = a.film + (long)b * a.film_bs + a.film_off; op[j] = 1.0f + fr[c + j]; sh[j] = fr[C + c + j]; }
    }
    const float* px = c < a.c1 ? a.x1 + (long)b * a.HW * a.c1 + c : a.x2 + (long)b * a.HW * a.c2 + (c - a.c1);
    const int ldx = c < a.c1 ? a.c1 : a.c2;
    const float* pd = a.dA + (long)b * a.HW * C + c;
    uint32_t dstep = 0u;
    if constexpr (DROP) dstep = drop_step_of(a.dr);
    for (int pix = px0 + tp; pix < px1; pix += npl) {
      const float4 xv = *reinterpret_cast<const float4*>(px + (long)pix * ldx);
      const float4 dv = *reinterpret_cast<const float4*>(pd + (long)pix * C);
      const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
      float ds[4] = {dv.x, dv.y, dv.z, dv.w};
      gn_bwd_drop4<DROP>(ds, a, b, pix, C, c, dstep);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float xh = (xs[j] - mean[j]) * rstd[j];
        const float dy = a.act ? ds[j] * silu_grad(gn_bwd_arg<FILM>(xh, ga[j], be[j], op[j], sh[j])) : ds[j];
        s1[j] += dy; s2[j] += dy * xh;
      }
    }
    float* d = cpart + (tp * QB + tq) * 8;
#pragma unroll
    for (int j = 0; j < 4; ++j) { d[j] = s1[j]; d[4 + j] = s2[j]; }
  }
  __syncthreads();
  if (t < QB) {
    float u[4] = {0.f, 0.f, 0.f, 0.f}, w[4] = {0.f, 0.f, 0.f, 0.f};
    for (int l = 0; l < npl; ++l) {
      const float* d = cpart + (l * QB + t) * 8;
#pragma unroll
      for (int j = 0; j < 4; ++j) { u[j] += d[j]; w[j] += d[4 + j]; }
    }
    float* dst = a.part + (((long)b * nslab + slab) * C + (qb0 + t) * 4) * 2;
#pragma unroll
    for (int j = 0; j < 4; ++j) { dst[j * 2] = u[j]; dst[j * 2 + 1] = w[j]; }
  }
}

// grid B: slab partials -> bc[B][C][2] (per-sample channel sums) and gm[B][groups][2]
// film_row != NULL: the sums are weighted by the sample's gamma (1 + scale) (row of sample b at film_row + b * film_bs)
__global__ void __launch_bounds__(256) gn_bwd_fold_kernel(const float* __restrict__ part, int nslab, int C, int groups, int HW,
                                                          const float* __restrict__ gamma, float* __restrict__ bc, float* __restrict__ gm,
                                                          const float* __restrict__ film_row = nullptr, long film_bs = 0) {
  extern __shared__ float sm[];   // [C][2] gamma-weighted sums
  const int b = blockIdx.x, cpg = C / groups;
  for (int c = threadIdx.x; c < C; c += 256) {
    float u = 0.f, w = 0.f;
    for (int k = 0; k < nslab; ++k) { const float* p = part + (((long)b * nslab + k) * C + c) * 2; u += p[0]; w += p[1]; }
    bc[((long)b * C + c) * 2] = u; bc[((long)b * C + c) * 2 + 1] = w;
    const float gmc = film_row ? gamma[c] * (1.0f + film_row[(long)b * film_bs + c]) : gamma[c];
    sm[c * 2] = u * gmc; sm[c * 2 + 1] = w * gmc;
  }
  __syncthreads();
  if (threadIdx.x < groups) {
    double u = 0.0, w = 0.0;
    for (int c = threadIdx.x * cpg; c < (threadIdx.x + 1) * cpg; ++c) { u += (double)sm[c * 2]; w += (double)sm[c * 2 + 1]; }
    const double n = (double)cpg * HW;
    gm[((long)b * groups + threadIdx.x) * 2] = (float)(u / n);
    gm[((long)b * groups + threadIdx.x) * 2 + 1] = (float)(w / n);
  }
}

// dgamma[c] (+)= sum_b bc[b][c][1]; dbeta[c] (+)= sum_b bc[b][c][0]; grid ceil(C/16), 256 threads = 16 channels x 16 sample lanes: the kernel
// is pure load latency, so a lane walks few samples (4 at batch 64, their loads in flight together) and the grid is 4x the 64-channel form's
__global__ void __launch_bounds__(256) gn_bwd_param_kernel(const float* __restrict__ bc, int B, int C, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                           int accumulate) {
  __shared__ float red[16][16][2];
  const int cl = threadIdx.x & 15, bl = threadIdx.x >> 4, c = blockIdx.x * 16 + cl;
  float u = 0.f, w = 0.f;
  if (c < C) {
    int b = bl;
    for (; b + 48 < B; b += 64) {
      float2 v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = *reinterpret_cast<const float2*>(bc + ((long)(b + 16 * i) * C + c) * 2);
#pragma unroll
      for (int i = 0; i < 4; ++i) { u += v[i].x; w += v[i].y; }
    }
    for (; b < B; b += 16) { const float2 v = *reinterpret_cast<const float2*>(bc + ((long)b * C + c) * 2); u += v.x; w += v.y; }
  }
  red[bl][cl][0] = u; red[bl][cl][1] = w;
  __syncthreads();
  if (bl == 0 && c < C) {
    float su = 0.f, sw = 0.f;
#pragma unroll
    for (int l = 0; l < 16; ++l) { su += red[l][cl][0]; sw += red[l][cl][1]; }   // fixed order
    dbeta[c] = (accumulate ? dbeta[c] : 0.f) + su;
    dgamma[c] = (accumulate ? dgamma[c] : 0.f) + sw;
  }
}

// The FiLM form of the parameter pass, from the same bc[b][c] = {U = sum dy, W = sum dy xhat} (z = (xhat gamma + beta)(1 + s) + sh):
//   dshift[b][c] = U;  dscale[b][c] = gamma_c W + beta_c U;  dgamma[c] (+)= sum_b (1 + s_bc) W;  dbeta[c] (+)= sum_b (1 + s_bc) U
// dscale / dshift go to row b of the embedding-gradient matrix dE (row stride de_ld): dE[b][de_off + c] and dE[b][de_off + C + c], the
// order of th.chunk. Same grid and lane walk as gn_bwd_param_kernel: a lane takes samples bl, bl + 16, ... in order, the 16 lanes join
// in lane order - no atomics, a fixed order.
__global__ void __launch_bounds__(256) gn_bwd_film_param_kernel(const float* __restrict__ bc, int B, int C, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, const float* __restrict__ film, long film_bs,
                                                                int film_off, float* __restrict__ dE, long de_ld, int de_off,
                                                                float* __restrict__ dgamma, float* __restrict__ dbeta, int accumulate) {
  __shared__ float red[16][16][2];
  const int cl = threadIdx.x & 15, bl = threadIdx.x >> 4, c = blockIdx.x * 16 + cl;
  float u = 0.f, w = 0.f;
  if (c < C) {
    const float gmc = gamma[c], btc = beta[c];
    for (int b = bl; b < B; b += 16) {
      const float2 v = *reinterpret_cast<const float2*>(bc + ((long)b * C + c) * 2);
      const float op = 1.0f + film[(long)b * film_bs + film_off + c];
      dE[(long)b * de_ld + de_off + c] = gmc * v.y + btc * v.x;
      dE[(long)b * de_ld + de_off + C + c] = v.x;
      u += op * v.x; w += op * v.y;
    }
  }
  red[bl][cl][0] = u; red[bl][cl][1] = w;
  __syncthreads();
  if (bl == 0 && c < C) {
    float su = 0.f, sw = 0.f;
#pragma unroll
    for (int l = 0; l < 16; ++l) { su += red[l][cl][0]; sw += red[l][cl][1]; }   // fixed order
    dbeta[c] = (accumulate ? dbeta[c] : 0.f) + su;
    dgamma[c] = (accumulate ? dgamma[c] : 0.f) + sw;
  }
}

// dx = rstd * (gamma*dy - m1 - xhat*m2) (+ add); grid (B, ceil(HW*Q / 1024)), one float4 per thread x 4
template <typename T, bool FILM = false, bool DROP = false>
__global__ void __launch_bounds__(256) gn_bwd_apply_kernel(GnBwdArgs a) {
  typedef T V4 __attribute__((ext_vector_type(4)));
  const int b = blockIdx.x, C = a.c1 + a.c2, Q = C >> 2, cpg = C / a.groups;
  const long total = (long)a.HW * Q;
  uint32_t dstep = 0u;
  if constexpr (DROP) dstep = drop_step_of(a.dr);
  for (int k = 0; k < 4; ++k) {
    const long e = ((long)blockIdx.y * 4 + k) * 256 + threadIdx.x;
    if (e >= total) return;
    const int pix = (int)(e / Q), c = (int)(e % Q) * 4;
    const bool first = c < a.c1;
    const float4 xv = first ? *reinterpret_cast<const float4*>(a.x1 + ((long)b * a.HW + pix) * a.c1 + c)
                            : *reinterpret_cast<const float4*>(a.x2 + ((long)b * a.HW + pix) * a.c2 + (c - a.c1));
    const long o = ((long)b * a.HW + pix) * C + c;
    const float4 dv = *reinterpret_cast<const float4*>(a.dA + o);
    const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
    float ds[4] = {dv.x, dv.y, dv.z, dv.w};
    gn_bwd_drop4<DROP>(ds, a, b, pix, C, c, dstep);
    // per-channel constants: 16-B loads of gamma / beta; the group's {mean, rstd} and {m1, m2} once per quad when a quad never straddles
    // two groups (channels per group % 4 == 0: every shape of the U-Net) — 4 loads instead of 24 scalar ones per quad
    const float4 ga4 = *reinterpret_cast<const float4*>(a.gamma + c), be4 = *reinterpret_cast<const float4*>(a.beta + c);
    const float gas[4] = {ga4.x, ga4.y, ga4.z, ga4.w}, bes[4] = {be4.x, be4.y, be4.z, be4.w};
    float mean[4], rstd[4], m1[4], m2[4];
    if ((cpg & 3) == 0) {
      const long gi = ((long)b * a.groups + c / cpg) * 2;
      const float2 mr = *reinterpret_cast<const float2*>(a.mr + gi), gm = *reinterpret_cast<const float2*>(a.gm + gi);
#pragma unroll
      for (int j = 0; j < 4; ++j) { mean[j] = mr.x; rstd[j] = mr.y; m1[j] = gm.x; m2[j] = gm.y; }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long gi = ((long)b * a.groups + (c + j) / cpg) * 2;
        mean[j] = a.mr[gi]; rstd[j] = a.mr[gi + 1]; m1[j] = a.gm[gi]; m2[j] = a.gm[gi + 1];
      }
    }
    float r[4];
    float ops[4] = {1.f, 1.f, 1.f, 1.f}, shs[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (FILM) {
      const float* fr = a.film + (long)b * a.film_bs + a.film_off;
      const float4 s4 = *reinterpret_cast<const float4*>(fr + c), h4 = *reinterpret_cast<const float4*>(fr + C + c);
      ops[0] = 1.0f + s4.x; ops[1] = 1.0f + s4.y; ops[2] = 1.0f + s4.z; ops[3] = 1.0f + s4.w;
      shs[0] = h4.x; shs[1] = h4.y; shs[2] = h4.z; shs[3] = h4.w;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float xh = (xs[j] - mean[j]) * rstd[j];
      const float dy = a.act ? ds[j] * silu_grad(gn_bwd_arg<FILM>(xh, gas[j], bes[j], ops[j], shs[j])) : ds[j];
      if constexpr (FILM) r[j] = rstd[j] * ((gas[j] * ops[j]) * dy - m1[j] - xh * m2[j]);
      else r[j] = rstd[j] * (gas[j] * dy - m1[j] - xh * m2[j]);
    }
    if (a.add) {
      const float4 av = *reinterpret_cast<const float4*>(a.add + o);
      r[0] += av.x; r[1] += av.y; r[2] += av.z; r[3] += av.w;
    }
    float* dst = first ? a.dx1 + ((long)b * a.HW + pix) * a.c1 + c : a.dx2 + ((long)b * a.HW + pix) * a.c2 + (c - a.c1);
    if (first ? a.acc1 : a.acc2) {
      const float4 old = *reinterpret_cast<const float4*>(dst);
      r[0] += old.x; r[1] += old.y; r[2] += old.z; r[3] += old.w;
    }
    *reinterpret_cast<float4*>(dst) = make_float4(r[0], r[1], r[2], r[3]);
    if (a.o_hi) {
      V4 hi;
#pragma unroll
      for (int j = 0; j < 4; ++j) hi[j] = (T)r[j];
      reinterpret_cast<V4*>(a.o_hi)[o >> 2] = hi;
      if (a.o_lo) {
        V4 lo;
#pragma unroll
        for (int j = 0; j < 4; ++j) lo[j] = (T)(r[j] - (float)hi[j]);
        reinterpret_cast<V4*>(a.o_lo)[o >> 2] = lo;
      }
    }
  }
}

// One-pass form: a block owns (sample b, a run of `cb` channels made of whole groups) and keeps xhat and dy of its HW x cb slice in REGISTERS
// (512 threads = qb channel quads x 512 / qb pixel lanes, PPT pixels per thread), so x and dA are read ONCE, with every load of the slice
// in flight at once, and the group means never leave the block: statistics, fold and apply in one launch (the three-kernel chain above
// cost ~50 us of launches and tails per GroupNorm on tensors that stream in ~25 us). Writes bc[b][c][2] for gn_bwd_param_kernel.
struct GnBwdFusedArgs {
  GnBwdArgs g;
  float* bc;
  int cb;
};

template <typename T, int PPT, bool FILM = false, bool DROP = false>
__global__ void __launch_bounds__(512) gn_bwd_fused_kernel(GnBwdFusedArgs fa) {
  typedef T V4 __attribute__((ext_vector_type(4)));
  __shared__ float red[512 * 8 + 2 * 288 + 2 * 72];  // [npl][qb][8] lane partials | [cb][2] gamma-weighted sums | [groups of the block][2]
  const GnBwdArgs& a = fa.g;
  const int b = blockIdx.x, cb = fa.cb, c0 = blockIdx.y * cb;
  const int C = a.c1 + a.c2, cpg = C / a.groups, qb = cb >> 2, t = threadIdx.x;
  const int npl = 512 / qb, tq = t % qb, tp = t / qb;
  const bool on = tp < npl;
  const int c = c0 + tq * 4;
  const bool first = c0 < a.c1;                      // the host keeps a block on one side of the concat seam
  const float* px = first ? a.x1 + (long)b * a.HW * a.c1 + c : a.x2 + (long)b * a.HW * a.c2 + (c - a.c1);
  const int ldx = first ? a.c1 : a.c2;
  const float* pd = a.dA + (long)b * a.HW * C + c;
  float mean[4], rstd[4], ga[4], be[4], op[4] = {1.f, 1.f, 1.f, 1.f}, sh[4] = {0.f, 0.f, 0.f, 0.f};
  float xh[PPT][4], dy[PPT][4];
  float4 av[PPT];
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  if (on) {
    float4 xv[PPT], dv[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      const int pix = tp + k * npl;
      xv[k] = dv[k] = av[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (pix < a.HW) {
        xv[k] = *reinterpret_cast<const float4*>(px + (long)pix * ldx);
        dv[k] = *reinterpret_cast<const float4*>(pd + (long)pix * C);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int g = (c + j) / cpg;
      mean[j] = a.mr[((long)b * a.groups + g) * 2]; rstd[j] = a.mr[((long)b * a.groups + g) * 2 + 1];
      ga[j] = a.gamma[c + j]; be[j] = a.beta[c + j];
      if constexpr (FILM) { const float* fr = a.film + (long)b * a.film_bs + a.film_off; op[j] = 1.0f + fr[c + j]; sh[j] = fr[C + c + j]; }
    }
    if (a.add) {     // the residual branch's gradient is needed after the fold: in flight across it
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        const int pix = tp + k * npl;
        if (pix < a.HW) av[k] = *reinterpret_cast<const float4*>(a.add + ((long)b * a.HW + pix) * C + c);
      }
    }
    uint32_t dstep = 0u;
    if constexpr (DROP) dstep = drop_step_of(a.dr);
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
      const bool live = tp + k * npl < a.HW;
      const float xi[4] = {xv[k].x, xv[k].y, xv[k].z, xv[k].w};
      float di[4] = {dv[k].x, dv[k].y, dv[k].z, dv[k].w};
      gn_bwd_drop4<DROP>(di, a, b, tp + k * npl, C, c, dstep);      // (a dead pixel's quad is zeros: the mask leaves them +0)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        xh[k][j] = (xi[j] - mean[j]) * rstd[j];
        dy[k][j] = a.act ? di[j] * silu_grad(gn_bwd_arg<FILM>(xh[k][j], ga[j], be[j], op[j], sh[j])) : di[j];
        if (live) { s1[j] += dy[k][j]; s2[j] += dy[k][j] * xh[k][j]; }
      }
    }
    float* d = red + (tp * qb + tq) * 8;
#pragma unroll
    for (int j = 0; j < 4; ++j) { d[j] = s1[j]; d[4 + j] = s2[j]; }
  }
  __syncthreads();
  float* gsum = red + 512 * 8;                       // [cb][2]
  float* gmv = gsum + 2 * 288;                       // [cb / cpg][2]  (cb <= 288)
  if (t < qb) {
    float u[4] = {0.f, 0.f, 0.f, 0.f}, w[4] = {0.f, 0.f, 0.f, 0.f};
    for (int l = 0; l < npl; ++l) {                  // fixed order
      const float* d = red + (l * qb + t) * 8;
#pragma unroll
      for (int j = 0; j < 4; ++j) { u[j] += d[j]; w[j] += d[4 + j]; }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int cc = c0 + t * 4 + j;
      fa.bc[((long)b * C + cc) * 2] = u[j]; fa.bc[((long)b * C + cc) * 2 + 1] = w[j];
      float gmm = a.gamma[cc];
      if constexpr (FILM) gmm *= 1.0f + a.film[(long)b * a.film_bs + a.film_off + cc];
      gsum[(t * 4 + j) * 2] = u[j] * gmm; gsum[(t * 4 + j) * 2 + 1] = w[j] * gmm;
    }
  }
  __syncthreads();
  if (t < cb / cpg) {
    double u = 0.0, w = 0.0;
    for (int k = t * cpg; k < (t + 1) * cpg; ++k) { u += (double)gsum[k * 2]; w += (double)gsum[k * 2 + 1]; }
    const double n = (double)cpg * a.HW;
    gmv[t * 2] = (float)(u / n); gmv[t * 2 + 1] = (float)(w / n);
  }
  __syncthreads();
  if (!on) return;
  float m1[4], m2[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { const int gl = (tq * 4 + j) / cpg; m1[j] = gmv[gl * 2]; m2[j] = gmv[gl * 2 + 1]; }
  float* pdx = first ? a.dx1 + (long)b * a.HW * a.c1 + c : a.dx2 + (long)b * a.HW * a.c2 + (c - a.c1);
  const bool acc = first ? a.acc1 : a.acc2;
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int pix = tp + k * npl;
    if (pix >= a.HW) break;
    float r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if constexpr (FILM) r[j] = rstd[j] * ((ga[j] * op[j]) * dy[k][j] - m1[j] - xh[k][j] * m2[j]);
      else r[j] = rstd[j] * (ga[j] * dy[k][j] - m1[j] - xh[k][j] * m2[j]);
    }
    r[0] += av[k].x; r[1] += av[k].y; r[2] += av[k].z; r[3] += av[k].w;
    const long o = ((long)b * a.HW + pix) * C + c;
    float* dst = pdx + (long)pix * ldx;
    if (acc) {
      const float4 old = *reinterpret_cast<const float4*>(dst);
      r[0] += old.x; r[1] += old.y; r[2] += old.z; r[3] += old.w;
    }
    *reinterpret_cast<float4*>(dst) = make_float4(r[0], r[1], r[2], r[3]);
    if (a.o_hi) {
      V4 hi;
#pragma unroll
      for (int j = 0; j < 4; ++j) hi[j] = (T)r[j];
      reinterpret_cast<V4*>(a.o_hi)[o >> 2] = hi;
      if (a.o_lo) {
        V4 lo;
#pragma unroll
        for (int j = 0; j < 4; ++j) lo[j] = (T)(r[j] - (float)hi[j]);
        reinterpret_cast<V4*>(a.o_lo)[o >> 2] = lo;
      }
    }
  }
}

template <typename T, bool FILM = false, bool DROP = false>
static void launch_gn_bwd_fused(const GnBwdFusedArgs& fa, int ppt, dim3 grid, hipStream_t st) {
  if (ppt <= 2) gn_bwd_fused_kernel<T, 2, FILM, DROP><<<grid, 512, 0, st>>>(fa);
  else if (ppt <= 4) gn_bwd_fused_kernel<T, 4, FILM, DROP><<<grid, 512, 0, st>>>(fa);
  else gn_bwd_fused_kernel<T, 8, FILM, DROP><<<grid, 512, 0, st>>>(fa);
}

// channel run of the one-pass kernel for this shape (0: use the three-kernel chain): whole groups, one side of the concat seam, rows of
// at least 64 B (128 B preferred), at most 8 pixels per thread; *ppt_out = pixels per thread
static int gn_bwd_fused_cb(int c1, int c2, int groups, int HW, int* ppt_out) {
  const int C = c1 + c2, cpg = C / groups;
  int unit = cpg;
  while (unit % 4 != 0) unit *= 2;                   // whole groups and whole quads
  auto ppt_of = [&](int cb) { const int npl = 512 / (cb / 4); return npl > 0 ? (HW + npl - 1) / npl : 1 << 20; };
  // the widest run at <= 4 pixels per thread (88 registers: two blocks per CU) with rows of >= 128 B; else the widest at <= 8 (164 registers)
  int best = 0;
  for (int pass = 0; pass < 2 && best == 0; ++pass)
    for (int cb = unit; cb <= 288; cb += unit) {
      if (c1 % cb != 0 || (c2 != 0 && c2 % cb != 0) || cb < (pass == 0 ? 32 : 16) || ppt_of(cb) > (pass == 0 ? 4 : 8)) continue;
      best = cb;
    }
  if (best == 0) return 0;
  *ppt_out = ppt_of(best);
  return best;
}

// where the parameter gradients go: dgamma / dbeta [C] (+= when acc_param) and, for the FiLM entries, row b of d_film (gn_bwd_film_param_kernel)
struct GnBwdParamOut { float* dgamma; float* dbeta; int acc_param; float* d_film; long d_film_bs; int d_film_off; };

// The one launch of GroupNorm backward, behind all four entries. Workspace: part [B][nslab][C][2] | bc [B][C][2] | gm [B][groups][2] (a.part and
// a.gm are set here). The one-pass kernel where gn_bwd_fused_cb finds a channel run (x and dA read once, no slab partials), else statistics,
// fold and apply; tests/refs_gn.py (gn_bwd_fused_cb) restates the rule. The parameter kernel runs last in every form: it reads only bc, which
// nothing after the fold writes.
template <bool FILM, bool DROP>
static int gn_bwd_launch(GnBwdArgs a, int B, int mm_dtype, float* ws, const GnBwdParamOut& po, void* stream) {
  const int C = a.c1 + a.c2, nslab = (a.HW + kGnBwdSlab - 1) / kGnBwdSlab, Q = C / 4;
  a.part = ws;
  float* bc = a.part + (long)B * nslab * C * 2;
  float* gm = bc + (long)B * C * 2;
  a.gm = gm;
  hipStream_t st = as_stream(stream);
  int ppt = 0;
  const int cb = gn_bwd_fused_cb(a.c1, a.c2, a.groups, a.HW, &ppt);
  if (cb > 0) {
    const GnBwdFusedArgs fa{a, bc, cb};
    if (mm_dtype == STEDM_F16) launch_gn_bwd_fused<_Float16, FILM, DROP>(fa, ppt, dim3(B, C / cb), st);
    else launch_gn_bwd_fused<__bf16, FILM, DROP>(fa, ppt, dim3(B, C / cb), st);
  } else {
    gn_bwd_stats_kernel<FILM, DROP><<<dim3(B, nslab, (Q + 63) / 64), 256, 0, st>>>(a);
    gn_bwd_fold_kernel<<<B, 256, (size_t)C * 8, st>>>(a.part, nslab, C, a.groups, a.HW, a.gamma, bc, gm, FILM ? a.film + a.film_off : nullptr, a.film_bs);
    const dim3 grid(B, (unsigned)(((long)a.HW * Q + 1023) / 1024));
    if (mm_dtype == STEDM_F16) gn_bwd_apply_kernel<_Float16, FILM, DROP><<<grid, 256, 0, st>>>(a);
    else gn_bwd_apply_kernel<__bf16, FILM, DROP><<<grid, 256, 0, st>>>(a);
  }
  if constexpr (FILM)
    gn_bwd_film_param_kernel<<<(C + 15) / 16, 256, 0, st>>>(bc, B, C, a.gamma, a.beta, a.film, a.film_bs, a.film_off, po.d_film, po.d_film_bs, po.d_film_off,
                                                            po.dgamma, po.dbeta, po.acc_param);
  else
    gn_bwd_param_kernel<<<(C + 15) / 16, 256, 0, st>>>(bc, B, C, po.dgamma, po.dbeta, po.acc_param);
  STEDM_LAUNCH_CHECK();
  return 0;
}

// The argument checks the four entries share, under the entry's own name; film: the film row and d_film row rules of the FiLM entries on top.
static int gn_bwd_check(const char* who, const GnBwdArgs& a, int B, int mm_dtype, const float* ws, const GnBwdParamOut& po, bool film) {
  const int C = a.c1 + a.c2;
  STEDM_CHECK_ARG(a.x1 && a.mr && a.gamma && a.beta && a.dA && ws && a.dx1 && po.dgamma && po.dbeta && (!film || (a.film && po.d_film)), "%s: null pointer", who);
  STEDM_CHECK_ARG(C % 4 == 0 && a.c1 % 4 == 0 && a.groups > 0 && a.groups <= 64 && C % a.groups == 0 && C * 8 <= 65536, "%s: channel constraints", who);
  STEDM_CHECK_ARG(mm_dtype == STEDM_F16 || mm_dtype == STEDM_BF16, "%s: bad mm_dtype", who);
  if (!film) return 0;
  STEDM_CHECK_ARG(B > 0 && a.HW > 0 && C > 0 && a.film_off >= 0 && a.film_off % 4 == 0 && a.film_bs % 4 == 0 &&
                      (a.film_bs == 0 || a.film_bs >= (long)a.film_off + 2 * C),
                  "%s: a film row holds 2 C values from film_off, 16-byte aligned (film_bstride=%ld film_off=%d C=%d)", who, a.film_bs, a.film_off, C);
  STEDM_CHECK_ARG(((uintptr_t)a.film & 15) == 0, "%s: film must be 16-byte aligned", who);
  STEDM_CHECK_ARG(po.d_film_off >= 0 && po.d_film_bs >= (long)po.d_film_off + 2 * C, "%s: a d_film row receives 2 C values from d_film_off", who);
  return 0;
}

// the dropout arguments of the drop entries -> DropArgs. One source tensor, C % 8 == 0.
static int gn_bwd_drop_args(float p, unsigned long long seed, unsigned site, unsigned step, const int32_t* step_ptr, int C, DropArgs* d) {
  STEDM_CHECK_ARG(p >= 0.f && p < 1.f, "gn_bwd_drop: p must be in [0, 1) (p=%g)", (double)p);
  STEDM_CHECK_ARG(C > 0 && C % 8 == 0, "gn_bwd_drop: need C %% 8 == 0 (C=%d)", C);
  *d = DropArgs{(uint64_t)seed, site, step, step_ptr, (uint32_t)lrint((double)p * 65536.0), (float)(1.0 / (1.0 - (double)p))};
  return 0;
}

}  // namespace

extern "C" int stedm_gn_fold(const float* cs1, int nslab1, int c1, const float* cs2, int nslab2, int c2, int groups, int B, int HW, float eps, float* mean_rstd,
                             void* stream) {
  STEDM_CHECK_ARG(cs1 && mean_rstd && groups > 0 && groups <= 64 && (c1 + c2) % groups == 0 && (cs2 != nullptr) == (c2 > 0), "gn_fold: bad args");
  gn_fold_kernel<<<B, 256, 0, as_stream(stream)>>>(GnPartials{cs1, nslab1, c1, cs2, nslab2, c2, groups, HW, eps, mean_rstd});
  STEDM_LAUNCH_CHECK();
  return 0;
}

// The four backward entries: each checks its arguments (gn_bwd_check under its own name), fills GnBwdArgs and calls gn_bwd_launch.
extern "C" int stedm_gn_bwd(const float* x1, int c1, const float* x2, int c2, const float* mean_rstd, const float* gamma, const float* beta, int groups, int act,
                            const float* dA, const float* add, int B, int HW, float* ws, float* dx1, int acc1, float* dx2, int acc2, void* dx16_hi,
                            void* dx16_lo, int mm_dtype, float* dgamma, float* dbeta, int acc_param, void* stream) {
  STEDM_CHECK_ARG((x2 != nullptr) == (c2 > 0) && (c2 == 0 || dx2), "gn_bwd: x2/c2/dx2 mismatch");
  const GnBwdArgs a{x1, x2, c1, c2, mean_rstd, gamma, beta, dA, groups, HW, act, nullptr, nullptr, add, dx1, dx2, acc1, acc2, dx16_hi, dx16_lo};
  const GnBwdParamOut po{dgamma, dbeta, acc_param, nullptr, 0, 0};
  if (const int rc = gn_bwd_check("gn_bwd", a, B, mm_dtype, ws, po, false)) return rc;
  return gn_bwd_launch<false, false>(a, B, mm_dtype, ws, po, stream);
}

// stedm_gn_bwd with the per-sample affine of a use_scale_shift_norm block (one source tensor): the FILM instantiations, and
// gn_bwd_film_param_kernel in place of gn_bwd_param_kernel.
extern "C" int stedm_gn_bwd_film(const float* x1, int c1, const float* mean_rstd, const float* gamma, const float* beta, int groups, int act,
                                 const float* film, long film_bstride, int film_off, const float* dA, const float* add, int B, int HW, float* ws,
                                 float* dx1, int acc1, void* dx16_hi, void* dx16_lo, int mm_dtype, float* dgamma, float* dbeta, int acc_param,
                                 float* d_film, long d_film_bstride, int d_film_off, void* stream) {
  const GnBwdArgs a{x1, nullptr, c1, 0, mean_rstd, gamma, beta, dA, groups, HW, act, nullptr, nullptr, add, dx1, nullptr, acc1, 0, dx16_hi, dx16_lo,
                    film, film_bstride, film_off};
  const GnBwdParamOut po{dgamma, dbeta, acc_param, d_film, d_film_bstride, d_film_off};
  if (const int rc = gn_bwd_check("gn_bwd_film", a, B, mm_dtype, ws, po, true)) return rc;
  return gn_bwd_launch<true, false>(a, B, mm_dtype, ws, po, stream);
}

// stedm_gn_bwd / stedm_gn_bwd_film for a GroupNorm whose activation went through the dropout pass (stedm_gn_apply16c_drop / _film_drop with the
// same p, seed, site and effective step): the DROP instantiations. One source tensor, C % 8 == 0. p == 0 is the plain entry.
extern "C" int stedm_gn_bwd_drop(const float* x1, int c1, const float* x2, int c2, const float* mean_rstd, const float* gamma, const float* beta, int groups,
                                 int act, const float* dA, const float* add, int B, int HW, float* ws, float* dx1, int acc1, float* dx2, int acc2,
                                 void* dx16_hi, void* dx16_lo, int mm_dtype, float* dgamma, float* dbeta, int acc_param, float p, unsigned long long seed,
                                 unsigned site, unsigned step, const int32_t* step_ptr, void* stream) {
  DropArgs d;
  if (const int rc = gn_bwd_drop_args(p, seed, site, step, step_ptr, c1, &d)) return rc;
  STEDM_CHECK_ARG(x2 == nullptr && c2 == 0 && dx2 == nullptr, "gn_bwd_drop: one source tensor only (x2, dx2 must be NULL)");
  (void)acc2;
  if (p == 0.f) return stedm_gn_bwd(x1, c1, nullptr, 0, mean_rstd, gamma, beta, groups, act, dA, add, B, HW, ws, dx1, acc1, nullptr, 0, dx16_hi, dx16_lo, mm_dtype,
                                    dgamma, dbeta, acc_param, stream);
  STEDM_CHECK_ARG(B > 0 && HW > 0, "gn_bwd_drop: channel constraints (B and HW must be positive)");
  const GnBwdArgs a{x1, nullptr, c1, 0, mean_rstd, gamma, beta, dA, groups, HW, act, nullptr, nullptr, add, dx1, nullptr, acc1, 0, dx16_hi, dx16_lo,
                    nullptr, 0, 0, d};
  const GnBwdParamOut po{dgamma, dbeta, acc_param, nullptr, 0, 0};
  if (const int rc = gn_bwd_check("gn_bwd_drop", a, B, mm_dtype, ws, po, false)) return rc;
  return gn_bwd_launch<false, true>(a, B, mm_dtype, ws, po, stream);
}

extern "C" int stedm_gn_bwd_film_drop(const float* x1, int c1, const float* mean_rstd, const float* gamma, const float* beta, int groups, int act,
                                      const float* film, long film_bstride, int film_off, const float* dA, const float* add, int B, int HW, float* ws,
                                      float* dx1, int acc1, void* dx16_hi, void* dx16_lo, int mm_dtype, float* dgamma, float* dbeta, int acc_param,
                                      float* d_film, long d_film_bstride, int d_film_off, float p, unsigned long long seed, unsigned site, unsigned step,
                                      const int32_t* step_ptr, void* stream) {
  DropArgs d;
  if (const int rc = gn_bwd_drop_args(p, seed, site, step, step_ptr, c1, &d)) return rc;
  if (p == 0.f) return stedm_gn_bwd_film(x1, c1, mean_rstd, gamma, beta, groups, act, film, film_bstride, film_off, dA, add, B, HW, ws, dx1, acc1, dx16_hi, dx16_lo,
                                         mm_dtype, dgamma, dbeta, acc_param, d_film, d_film_bstride, d_film_off, stream);
  const GnBwdArgs a{x1, nullptr, c1, 0, mean_rstd, gamma, beta, dA, groups, HW, act, nullptr, nullptr, add, dx1, nullptr, acc1, 0, dx16_hi, dx16_lo,
                    film, film_bstride, film_off, d};
  const GnBwdParamOut po{dgamma, dbeta, acc_param, d_film, d_film_bstride, d_film_off};
  if (const int rc = gn_bwd_check("gn_bwd_film_drop", a, B, mm_dtype, ws, po, true)) return rc;
  return gn_bwd_launch<true, true>(a, B, mm_dtype, ws, po, stream);
}

extern "C" long stedm_gn_bwd_ws_floats(int B, int HW, int C, int groups) {
  return (long)B * ((HW + kGnBwdSlab - 1) / kGnBwdSlab) * C * 2 + (long)B * C * 2 + (long)B * groups * 2;
}
