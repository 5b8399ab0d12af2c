// General DPM-Solver (dpm_solver.py: orders 1-3, multistep / singlestep, noise and data prediction, both solver types,
// denoise_to_zero, dynamic thresholding), driven by the host plan of stedm_amd/dpm_solver.py (dpm_plan): one table row per model
// evaluation (NFE), selected on the device by *step_idx so that one captured NFE serves every row.
#include <stdint.h>

#include "common.hpp"
using namespace stedm;

namespace {

// row layout (dpm_solver.R_*)
enum { R_ALPHA = 0, R_SIGMA, R_TO_X0, R_THRESH, R_W, R_KIND, R_COMMIT, R_P, R_U0, R_V0, R_U1, R_V1, R_A, R_B, R_C, R_D, R_K0, R_K1, R_E,
       R_F, R_Q };
enum { K_FIRST = 0, K_DIFF, K_MS3, K_SS3T, K_COPY };

struct DpmuRow {
  float alpha, sigma, a, b, c, d, k0, k1, e, f, q;
  int to_x0, w, kind, commit, P, U0, V0, U1, V1;
  unsigned need;      // bit j: the update reads slot j
};

__device__ __forceinline__ int slot_of(float v) { return min(max((int)v, 0), 2); }

__device__ __forceinline__ DpmuRow load_row(const float* __restrict__ rows, const int32_t* __restrict__ step_idx) {
  const float* r = rows + (long)(step_idx ? *step_idx : 0) * STEDM_DPMU_NCOEF;
  DpmuRow o;
  o.alpha = r[R_ALPHA]; o.sigma = r[R_SIGMA]; o.a = r[R_A]; o.b = r[R_B]; o.c = r[R_C]; o.d = r[R_D];
  o.k0 = r[R_K0]; o.k1 = r[R_K1]; o.e = r[R_E]; o.f = r[R_F]; o.q = r[R_Q];
  o.to_x0 = r[R_TO_X0] != 0.0f; o.commit = r[R_COMMIT] != 0.0f;
  o.kind = min(max((int)r[R_KIND], 0), (int)K_COPY);
  o.w = slot_of(r[R_W]); o.P = slot_of(r[R_P]);
  o.U0 = slot_of(r[R_U0]); o.V0 = slot_of(r[R_V0]); o.U1 = slot_of(r[R_U1]); o.V1 = slot_of(r[R_V1]);
  o.need = 1u << o.P;
  if (o.kind == K_DIFF) o.need |= (1u << o.U0) | (1u << o.V0);
  if (o.kind == K_MS3 || o.kind == K_SS3T) o.need |= (1u << o.U0) | (1u << o.V0) | (1u << o.U1) | (1u << o.V1);
  return o;
}

__device__ __forceinline__ float pick(float m0, float m1, float m2, int j) { return j == 0 ? m0 : (j == 1 ? m1 : m2); }

// the model output of the row: the CFG combine, then data_prediction_fn's x0 when the row asks for it
__device__ __forceinline__ float dpmu_model(float xin, float ec, float eu, bool cfg, float s, const DpmuRow& r) {
#pragma clang fp contract(off)       // every product and sum rounded on its own, as torch's CPU ops round them
  const float eps = cfg ? eu + s * (ec - eu) : ec;
  return r.to_x0 ? (xin - r.sigma * eps) / r.alpha : eps;      // IEEE division
}

// the update into the next U-Net input from the base xb and the slots m0..m2 (the kinds of dpm_solver.K_*)
__device__ __forceinline__ float dpmu_combine(float xb, float m0, float m1, float m2, const DpmuRow& r) {
#pragma clang fp contract(off)
  if (r.kind == K_COPY) return pick(m0, m1, m2, r.P);
  float o = r.a * xb - r.b * pick(m0, m1, m2, r.P);
  if (r.kind == K_DIFF) {
    o = o + r.c * (r.k0 * (pick(m0, m1, m2, r.U0) - pick(m0, m1, m2, r.V0)));
  } else if (r.kind != K_FIRST) {
    const float d10 = r.k0 * (pick(m0, m1, m2, r.U0) - pick(m0, m1, m2, r.V0));
    const float d11 = r.k1 * (pick(m0, m1, m2, r.U1) - pick(m0, m1, m2, r.V1));
    float D1, D2;
    if (r.kind == K_MS3) {
      D1 = d10 + r.e * (d10 - d11);
      D2 = r.f * (d10 - d11);
    } else {
      D1 = (r.e * d10 - r.f * d11) / r.q;
      D2 = (2.0f * (d11 - d10)) / r.q;
    }
    o = (o + r.c * D1) + r.d * D2;
  }
  return o;
}

// One element: mode ALL computes the model output into slot w and the update; MODEL only the former; COMBINE only the latter (slot w is
// then read back, after stedm_dpm_threshold has rewritten it).
struct DpmuIO {
  float xin, xb, ec, eu, m0, m1, m2;
};

__device__ __forceinline__ void dpmu_elem(DpmuIO& v, const DpmuRow& r, bool cfg, float s, int mode, float& mw, float& out, float& px0) {
#pragma clang fp contract(off)
  if (mode != STEDM_DPMU_COMBINE) {
    mw = dpmu_model(v.xin, v.ec, v.eu, cfg, s, r);
    v.m0 = r.w == 0 ? mw : v.m0;       // selects, not an indexed private array (that would live in scratch)
    v.m1 = r.w == 1 ? mw : v.m1;
    v.m2 = r.w == 2 ? mw : v.m2;
  }
  if (mode != STEDM_DPMU_MODEL) {
    out = dpmu_combine(v.xb, v.m0, v.m1, v.m2, r);
    const float mv = pick(v.m0, v.m1, v.m2, r.w);
    px0 = r.to_x0 ? mv : (v.xin - r.sigma * mv) / r.alpha;
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) dpm_update_kernel(float* x, float* base, const float* __restrict__ e_c, const float* __restrict__ e_u,
                                                         float* slots, long slot_stride, float* pred_x0, const float* __restrict__ rows,
                                                         const int32_t* __restrict__ step_idx, float s, int mode, long n) {
  const long e0 = 4 * ((long)blockIdx.x * 256 + threadIdx.x);
  if (e0 >= n) return;
  const DpmuRow r = load_row(rows, step_idx);
  const bool cfg = e_u != nullptr;
  const bool calc = mode != STEDM_DPMU_COMBINE, comb = mode != STEDM_DPMU_MODEL;
  // slots the update reads from memory: slot w comes from registers unless this launch only combines
  const unsigned rd = comb ? (calc ? (r.need & ~(1u << r.w)) : (r.need | (1u << r.w))) : 0u;
  if (VEC && e0 + 4 <= n) {
    float4 xin = make_float4(0.f, 0.f, 0.f, 0.f), xb = xin, ec = xin, eu = xin, m[3] = {xin, xin, xin};
    if (calc || !r.to_x0) xin = *reinterpret_cast<const float4*>(x + e0);
    if (comb) xb = *reinterpret_cast<const float4*>(base + e0);
    if (calc) {
      ec = *reinterpret_cast<const float4*>(e_c + e0);
      eu = cfg ? *reinterpret_cast<const float4*>(e_u + e0) : ec;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
      if (rd & (1u << j)) m[j] = *reinterpret_cast<const float4*>(slots + j * slot_stride + e0);
    float4 mw, out, px;
#define STEDM_DPMU_LANE(C)                                                                  \
    {                                                                                       \
      DpmuIO v{xin.C, xb.C, ec.C, eu.C, m[0].C, m[1].C, m[2].C};                            \
      dpmu_elem(v, r, cfg, s, mode, mw.C, out.C, px.C);                                     \
    }
    STEDM_DPMU_LANE(x) STEDM_DPMU_LANE(y) STEDM_DPMU_LANE(z) STEDM_DPMU_LANE(w)
#undef STEDM_DPMU_LANE
    if (calc) *reinterpret_cast<float4*>(slots + r.w * slot_stride + e0) = mw;
    if (comb) {
      *reinterpret_cast<float4*>(x + e0) = out;
      if (r.commit) *reinterpret_cast<float4*>(base + e0) = out;
      if (pred_x0) *reinterpret_cast<float4*>(pred_x0 + e0) = px;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long e = e0 + j;
      if (e < n) {
        DpmuIO v{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (calc || !r.to_x0) v.xin = x[e];
        if (comb) v.xb = base[e];
        if (calc) {
          v.ec = e_c[e];
          v.eu = cfg ? e_u[e] : v.ec;
        }
        if (rd & 1u) v.m0 = slots[e];
        if (rd & 2u) v.m1 = slots[slot_stride + e];
        if (rd & 4u) v.m2 = slots[2 * slot_stride + e];
        float mw = 0.f, out = 0.f, px = 0.f;
        dpmu_elem(v, r, cfg, s, mode, mw, out, px);
        if (calc) slots[r.w * slot_stride + e] = mw;
        if (comb) {
          x[e] = out;
          if (r.commit) base[e] = out;
          if (pred_x0) pred_x0[e] = px;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Dynamic thresholding (data_prediction_fn, dpm_solver.py:361-374), one workgroup per sample of n elements:
//   q = torch.quantile(|x0|, 0.995) exactly: rank = 0.995f * (n - 1) in fp32, the order statistics at floor(rank) and ceil(rank), and
//       torch's CPU lerp (fma(w, hi - lo, lo) for w < 0.5, fma(w - 1, hi - lo, hi) otherwise);
//   s = max(q, max_val);  x0 = clamp(x0, -s, s) / s.
// The floor(rank)-th order statistic comes from a radix select on the bit pattern of |x| (non-negative floats order like their bits):
// four 8-bit digit passes, each a 256-bin histogram of the elements that share the digits found so far, kept per wave in LDS (integer
// LDS atomics: the counts, and so the result, do not depend on their order). The ceil(rank)-th is the same value while the equal run
// reaches it, otherwise the smallest bit pattern above it (one min pass). No global atomics, nothing allocated, nothing to reset.
// ------------------------------------------------------------------------------------------------
constexpr int TH_THREADS = 1024;
constexpr int TH_WAVES = TH_THREADS / 64;

__global__ void __launch_bounds__(TH_THREADS) dpm_threshold_kernel(float* slots, long slot_stride, const float* __restrict__ rows,
                                                                   const int32_t* __restrict__ step_idx, float max_val, long n,
                                                                   float* __restrict__ q_out) {
  int w = 0;
  if (rows) {
    const float* r = rows + (long)(step_idx ? *step_idx : 0) * STEDM_DPMU_NCOEF;
    if (r[R_THRESH] == 0.0f) return;     // uniform over the grid: every workgroup leaves
    w = slot_of(r[R_W]);
  }
  float* xs = slots + w * slot_stride + (long)blockIdx.x * n;
  const int tid = threadIdx.x, wave = tid >> 6;
  __shared__ uint32_t hist[TH_WAVES][256];
  __shared__ uint32_t tot[256];
  __shared__ uint32_t s_digit, s_k, s_cnt, s_min;

  const float rank = 0.995f * (float)(n - 1);
  const long lo = (long)floorf(rank), hi = (long)ceilf(rank);
  const float wt = rank - (float)lo;
  uint32_t prefix = 0, mask = 0, k = (uint32_t)lo, count_eq = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = tid; i < TH_WAVES * 256; i += TH_THREADS) (&hist[0][0])[i] = 0u;
    __syncthreads();
    for (long i = tid; i < n; i += TH_THREADS) {
      const uint32_t b = __float_as_uint(xs[i]) & 0x7FFFFFFFu;
      if ((b & mask) == prefix) atomicAdd(&hist[wave][(b >> shift) & 255u], 1u);
    }
    __syncthreads();
    uint32_t c = 0;
    if (tid < 256) {
      for (int v = 0; v < TH_WAVES; ++v) c += hist[v][tid];
      tot[tid] = c;
    }
    __syncthreads();
    // inclusive scan of tot over the 256 bins (Hillis-Steele in place)
    for (int off = 1; off < 256; off <<= 1) {
      uint32_t add = 0;
      if (tid < 256 && tid >= off) add = tot[tid - off];
      __syncthreads();
      if (tid < 256) tot[tid] += add;
      __syncthreads();
    }
    if (tid < 256) {
      const uint32_t incl = tot[tid], excl = incl - c;
      if (excl <= k && k < incl) {
        s_digit = (uint32_t)tid;
        s_k = k - excl;
        s_cnt = c;      // the count of the chosen bin
      }
    }
    __syncthreads();
    prefix |= s_digit << shift;
    mask |= 255u << shift;
    k = s_k;
    count_eq = s_cnt;
    __syncthreads();
  }
  // prefix: the bits of the floor(rank)-th smallest |x|; k: its position inside the run of count_eq equal values
  uint32_t above = prefix;
  if (hi != lo && k + 1 >= count_eq) {
    if (tid == 0) s_min = 0xFFFFFFFFu;
    __syncthreads();
    uint32_t m = 0xFFFFFFFFu;
    for (long i = tid; i < n; i += TH_THREADS) {
      const uint32_t b = __float_as_uint(xs[i]) & 0x7FFFFFFFu;
      if (b > prefix) m = min(m, b);
    }
    atomicMin(&s_min, m);
    __syncthreads();
    above = s_min;
  }
  const float vb = __uint_as_float(prefix), va = __uint_as_float(above);
  const float d = va - vb;
  const float q = fabsf(wt) < 0.5f ? fmaf(wt, d, vb) : fmaf(wt - 1.0f, d, va);
  if (q_out && tid == 0) q_out[blockIdx.x] = q;
  const float sc = fmaxf(q, max_val);
  for (long i = tid; i < n; i += TH_THREADS) xs[i] = fminf(fmaxf(xs[i], -sc), sc) / sc;
}

}  // namespace

extern "C" int stedm_dpm_update(float* x, float* base, const float* e_c, const float* e_u, float* slots, long slot_stride, float* pred_x0,
                                const float* rows, const int32_t* step_idx, float cfg_scale, int mode, long n, void* stream) {
  STEDM_CHECK_ARG(x && base && slots && rows, "dpm_update: null pointer");
  STEDM_CHECK_ARG(mode == STEDM_DPMU_ALL || mode == STEDM_DPMU_MODEL || mode == STEDM_DPMU_COMBINE, "dpm_update: bad mode %d", mode);
  STEDM_CHECK_ARG(mode == STEDM_DPMU_COMBINE || e_c, "dpm_update: e_c is required unless mode is COMBINE");
  STEDM_CHECK_ARG(n > 0 && n <= (1L << 40) && slot_stride >= n, "dpm_update: bad element count %ld / slot stride %ld", n, slot_stride);
  const bool aligned = ((uintptr_t)x | (uintptr_t)base | (uintptr_t)e_c | (uintptr_t)e_u | (uintptr_t)slots | (uintptr_t)pred_x0) % 16 == 0 &&
                       slot_stride % 4 == 0;
  const long groups = (n + 3) / 4;
  const long blocks = (groups + 255) / 256;
  STEDM_CHECK_ARG(blocks <= 0x7FFFFFFFL, "dpm_update: %ld elements exceed one launch", n);
  if (aligned)
    dpm_update_kernel<true><<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(x, base, e_c, e_u, slots, slot_stride, pred_x0, rows, step_idx,
                                                                            cfg_scale, mode, n);
  else
    dpm_update_kernel<false><<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(x, base, e_c, e_u, slots, slot_stride, pred_x0, rows,
                                                                             step_idx, cfg_scale, mode, n);
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int stedm_dpm_threshold(float* slots, long slot_stride, const float* rows, const int32_t* step_idx, float max_val, int B, long n,
                                   float* q_out, void* stream) {
  STEDM_CHECK_ARG(slots, "dpm_threshold: null pointer");
  STEDM_CHECK_ARG(B > 0 && n > 0 && n <= (1L << 31) && slot_stride >= (long)B * n, "dpm_threshold: bad sizes B %d n %ld stride %ld", B, n,
                  slot_stride);
  dpm_threshold_kernel<<<(unsigned)B, TH_THREADS, 0, as_stream(stream)>>>(slots, slot_stride, rows, step_idx, max_val, n, q_out);
  STEDM_LAUNCH_CHECK();
  return 0;
}
