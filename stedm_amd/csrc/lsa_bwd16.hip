// LSA backward on the 16-bit matrix pipe (v_mfma_f32_32x32x16_{f16,bf16}): the opt-in second form of stedm_lsa_bwd (svit_bwd.hip) for the
// single-product modes. The fp32 form stays the default; this one reads the forward's hi planes only.
//
// Numerics contract (tests/refs_lsa_bwd16.py is the same function in fp64). R = round to nearest even into the mode's 16-bit format.
// Exactly three values are rounded:
//   dOr = R(s dO)             s = one exact power of two per call, from the biased exponent e of amax|dO| (a max over the bit patterns of
//                             |dO|, order-independent): s = 2^(clamp(264 - e, 1, 253) - 127), so that s amax lies in [2^10, 2^11);
//                             amax == 0: s = 1. The same rule in f16 and bf16. No host synchronisation. s is divided out of every output
//                             by an exact multiplication with 1 / s.
//   Pd  = R(P keep / (1 - p)) the operand of dV += Pd^T dOr
//   dS  = R(dS)               the operand of dQ += dS K and dK += dS^T Q
// Everything else is fp32 or better: S = q k^T and dP = dOr V^T are 16-bit MFMA products of 16-bit values with fp32 accumulation; the
// row maximum, 1 / row sum and D = sum_j Pd dP come from the unrounded fp32 P and dP; P = exp2(s - max) / sum (not exp2(s - LSE));
// dS = P o (keep / (1 - p) dP - D) is exactly 0 on the masked diagonal and beyond T; d temperature = sum dS o s from the unrounded dS in
// fp64, one partial per block, folded in block order. Output scales as in the fp32 form: dQ exp(temperature), dK ln 2.
// No float atomics: bitwise reproducible. Pad rows (>= T) of q / k and pad columns of vt are replaced by zero before they are staged.
//
// Geometry. A prep pass writes five zero-padded 16-bit planes into the workspace: dOr [BH][Tp][64] and its transpose [BH][64][Tp], the
// transposes of q and k [BH][64][Tp] and V = vt^T [BH][Tp][64] - every contraction then finds its operand with the contracted index
// contiguous, and the main kernels stage tiles with plain 16-byte copies.
//   q kernel  grid (BH, ceil(T / 128)), four waves of 32 queries. Per 64-key tile a wave forms S^T and dP^T (A = K / V rows from LDS, B =
//             its q / dOr rows in registers): lane (r, h) holds query r and keys 32 sub + (e & 3) + 8 (e >> 2) + 4 h - the forward's layout
//             (lsa_flash_kernel), so the lane follows stream h of its query and its 32-bit keep word is the tile's. Two passes: statistics
//             (online, per lane; the two halves of a row meet once at the end), then dS, which goes from the accumulator registers
//             straight into the B operand of dQ^T += K^T dS^T. The passes are two launches of one template (each within 256 registers);
//             pass 1 takes the row statistics from the workspace. The keep words are written to the workspace as a 1-bit mask
//             [BH][Tp / 64][2][Tp] (B H Tp Tp / 8 bytes) in pass 0 and read back in pass 1.
//   kv kernel grid (BH, ceil(T / 128)), four waves of 32 keys, K / V rows in registers; per 64-query tile S and dP (A = q / dOr rows from
//             LDS), keep words from the mask (no stream is advanced), Pd and dS from the accumulators into the B operands of
//             dV^T += dOr^T Pd and dK^T += Q^T dS.
// LDS: 27 KiB (q) and 37 KiB (kv) per workgroup.
#include <float.h>

#include "conv_common.hpp"
#include "dropmask.hpp"
using namespace stedm;

namespace {

constexpr int PT = 72;                  // row pitch (16-bit elements) of the 64 x 64 LDS tiles: 144 B, 16-B aligned rows
constexpr int TILE = 64 * PT;
constexpr float kLn2 = 0.6931471805599453f;

struct Lsa16Args {
  const void *q, *k, *vt;               // the forward's hi planes: q, k [BH][Tp][64], vt [BH][64][Tp]
  const float* dO;                      // [B*T][H*64]
  float* dqkv;                          // [B*T][3*H*64]
  unsigned* amax;                       // bit pattern of max |dO|
  float *rmax, *rinv, *dlt;             // [BH][Tp]
  double* tpart;                        // [BH * gridDim.y]
  void *g, *gt, *qt, *kt, *vr;          // prep planes
  unsigned* mask;                       // [BH][Tp / 64][2][Tp] keep words (p > 0)
  int T, Tp, H;
  float qscale;
  unsigned thr16, site;
  unsigned long long seed;
  float inv_keep;
};

// s and 1 / s from the bit pattern of amax |dO|
__device__ __forceinline__ void do_scale(unsigned bits, float& s, float& inv) {
  if (bits == 0u) { s = 1.f; inv = 1.f; return; }
  int se = 264 - (int)((bits >> 23) & 0xFFu);
  se = se < 1 ? 1 : (se > 253 ? 253 : se);
  s = __uint_as_float((unsigned)se << 23);
  inv = __uint_as_float((unsigned)(254 - se) << 23);
}

__global__ void __launch_bounds__(256) lsa16_amax_kernel(const float* __restrict__ x, long n4, unsigned* __restrict__ amax) {
  unsigned m = 0u;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const uint4 v = reinterpret_cast<const uint4*>(x)[i];
    m = max(max(m, v.x & 0x7FFFFFFFu), max(v.y & 0x7FFFFFFFu, max(v.z & 0x7FFFFFFFu, v.w & 0x7FFFFFFFu)));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
  if ((threadIdx.x & 63) == 0 && m != 0u) atomicMax(amax, m);      // a max of bit patterns of non-negative floats: order-independent
}

// t [64][66] -> dst[d * pitch + i], d, i < 64: the transpose of the tile, 16 bytes per store
template <typename T>
__device__ __forceinline__ void store_transposed(const T* t, T* dst, long pitch) {
  typedef T V8 __attribute__((ext_vector_type(8)));
  for (int c = threadIdx.x; c < 512; c += 256) {
    const int d = c >> 3, i8 = (c & 7) * 8;
    V8 v;
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = t[(i8 + u) * 66 + d];
    *reinterpret_cast<V8*>(dst + d * pitch + i8) = v;
  }
}

// grid (BH, Tp / 64): dOr rows i0 .. i0 + 63 of the sample-head -> g [BH][Tp][64], gt [BH][64][Tp]; rows >= T are zero
template <typename T>
__global__ void __launch_bounds__(256) lsa16_prep_do_kernel(Lsa16Args a) {
  typedef T V4 __attribute__((ext_vector_type(4)));
  __shared__ T t[64 * 66];
  const int bh = blockIdx.x, b = bh / a.H, hd = bh % a.H, i0 = blockIdx.y * 64, HD = a.H * 64;
  float s, inv;
  do_scale(*a.amax, s, inv);
  T* g = reinterpret_cast<T*>(a.g);
  for (int c = threadIdx.x; c < 1024; c += 256) {
    const int row = c >> 4, c4 = (c & 15) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i0 + row < a.T) v = *reinterpret_cast<const float4*>(a.dO + ((long)b * a.T + i0 + row) * HD + hd * 64 + c4);
    V4 o;
    o[0] = (T)(v.x * s); o[1] = (T)(v.y * s); o[2] = (T)(v.z * s); o[3] = (T)(v.w * s);
    *reinterpret_cast<V4*>(g + ((long)bh * a.Tp + i0 + row) * 64 + c4) = o;
#pragma unroll
    for (int u = 0; u < 4; ++u) t[row * 66 + c4 + u] = o[u];
  }
  __syncthreads();
  store_transposed<T>(t, reinterpret_cast<T*>(a.gt) + (long)bh * 64 * a.Tp + i0, a.Tp);
}

// grid (BH, Tp / 64, 3): z = 0: q rows -> qt, 1: k rows -> kt (rows >= T zero), 2: vt columns -> vr (columns >= T zero)
template <typename T>
__global__ void __launch_bounds__(256) lsa16_prep_planes_kernel(Lsa16Args a) {
  typedef T V8 __attribute__((ext_vector_type(8)));
  __shared__ T t[64 * 66];
  const int bh = blockIdx.x, i0 = blockIdx.y * 64, z = blockIdx.z;
  const T* src;
  long spitch;
  if (z < 2) { src = reinterpret_cast<const T*>(z == 0 ? a.q : a.k) + ((long)bh * a.Tp + i0) * 64; spitch = 64; }
  else { src = reinterpret_cast<const T*>(a.vt) + (long)bh * 64 * a.Tp + i0; spitch = a.Tp; }
  for (int c = threadIdx.x; c < 512; c += 256) {
    const int row = c >> 3, c8 = (c & 7) * 8;
    const V8 v = *reinterpret_cast<const V8*>(src + row * spitch + c8);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const bool ok = z < 2 ? i0 + row < a.T : i0 + c8 + u < a.T;
      t[row * 66 + c8 + u] = ok ? v[u] : (T)0.f;
    }
  }
  __syncthreads();
  if (z < 2) store_transposed<T>(t, reinterpret_cast<T*>(z == 0 ? a.qt : a.kt) + (long)bh * 64 * a.Tp + i0, a.Tp);
  else store_transposed<T>(t, reinterpret_cast<T*>(a.vr) + ((long)bh * a.Tp + i0) * 64, 64);
}

// 64 rows x 64 elements from src (row pitch `pitch`) -> dst [64][PT]; rows >= nvalid are zero and not read
template <typename T>
__device__ __forceinline__ void stage64(const T* src, long pitch, int nvalid, T* dst) {
  typedef T V8 __attribute__((ext_vector_type(8)));
  for (int c = threadIdx.x; c < 512; c += 256) {
    const int row = c >> 3, c8 = (c & 7) * 8;
    V8 v;
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = (T)0.f;
    if (row < nvalid) v = *reinterpret_cast<const V8*>(src + row * pitch + c8);
    *reinterpret_cast<V8*>(dst + row * PT + c8) = v;
  }
}

// A operand whose contraction index follows the accumulator's row order: elements j + (t & 3) + 8 (t >> 2), t = 0 .. 7
template <typename T>
__device__ __forceinline__ typename MM<T>::V8 frag_acc_order(const T* p) {
  typedef typename MM<T>::V4 V4;
  const V4 lo = *reinterpret_cast<const V4*>(p), hi = *reinterpret_cast<const V4*>(p + 8);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// ------------------------------------------------------------------------------------------------ query side
// PASS 0: statistics and mask; PASS 1: dS, dQ and the partial of d temperature (one launch each: both stay within 256 registers)
template <typename T, bool DROP, int PASS>
__global__ void __launch_bounds__(256, 2) lsa16_q_kernel(Lsa16Args a) {
  typedef typename MM<T>::V8 V8;
  __shared__ __attribute__((aligned(16))) T sm[3 * TILE];
  __shared__ double red[256];
  T *sK = sm, *sV = sm + TILE, *sKt = sm + 2 * TILE;
  const int bh = blockIdx.x, b = bh / a.H, hd = bh % a.H;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, r = l & 31, h = l >> 5;
  const int gi = blockIdx.y * 128 + 32 * w + r;
  const bool rowok = gi < a.T;
  const int HD = a.H * 64, nkt = (a.T + 63) / 64, nktp = a.Tp / 64;
  const T* kg = reinterpret_cast<const T*>(a.k) + (long)bh * a.Tp * 64;
  const T* vg = reinterpret_cast<const T*>(a.vr) + (long)bh * a.Tp * 64;
  const T* ktg = reinterpret_cast<const T*>(a.kt) + (long)bh * 64 * a.Tp;
  V8 qf[4], gf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
    for (int u = 0; u < 8; ++u) qf[ks][u] = (T)0.f;
    if (rowok) qf[ks] = *reinterpret_cast<const V8*>(reinterpret_cast<const T*>(a.q) + ((long)bh * a.Tp + gi) * 64 + 16 * ks + 8 * h);
    gf[ks] = *reinterpret_cast<const V8*>(reinterpret_cast<const T*>(a.g) + ((long)bh * a.Tp + gi) * 64 + 16 * ks + 8 * h);
  }
  float sc_s, sc_inv;
  do_scale(*a.amax, sc_s, sc_inv);
  float m_run = -INFINITY, l_run = 0.f, d_run = 0.f, linv = 0.f, dv = 0.f;
  double tsum = 0.0;
  f32x16 dq[2];
#pragma unroll
  for (int e = 0; e < 16; ++e) { dq[0][e] = 0.f; dq[1][e] = 0.f; }

  constexpr int pass = PASS;
  if (pass == 1) {
    const long o = (long)bh * a.Tp + gi;
    m_run = rowok ? a.rmax[o] : 0.f;
    linv = rowok ? a.rinv[o] : 0.f;
    dv = rowok ? a.dlt[o] : 0.f;
  }
  {
    U4 st{};
    if (DROP && pass == 0 && rowok) st = attn_stream_init((unsigned)gi, (unsigned)bh, a.site, (unsigned)h, a.seed);
    for (int kt = 0; kt < nkt; ++kt) {
      const int j0 = kt * 64;
      __syncthreads();
      stage64<T>(kg + (long)j0 * 64, 64, a.T - j0, sK);
      stage64<T>(vg + (long)j0 * 64, 64, 64, sV);
      if (pass == 1) stage64<T>(ktg + j0, a.Tp, 64, sKt);
      __syncthreads();
      unsigned kw = ~0u;
      if (DROP) {
        unsigned* mw = a.mask + ((long)(bh * nktp + kt) * 2 + h) * a.Tp + gi;
        if (pass == 0) {
          if (rowok) kw = attn_keep_bits(st, a.thr16);
          *mw = kw;
        } else kw = *mw;
      }
      f32x16 s[2], dp[2];
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
        for (int e = 0; e < 16; ++e) { s[sub][e] = 0.f; dp[sub][e] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const int off = (32 * sub + r) * PT + 16 * ks + 8 * h;
          s[sub] = MM<T>::mfma(*reinterpret_cast<const V8*>(sK + off), qf[ks], s[sub]);
          dp[sub] = MM<T>::mfma(*reinterpret_cast<const V8*>(sV + off), gf[ks], dp[sub]);
        }
      }
      if (pass == 0) {
        float mx = -INFINITY;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int col = j0 + 32 * sub + (e & 3) + 8 * (e >> 2) + 4 * h;
            const float x = col >= a.T ? -INFINITY : (col == gi ? -FLT_MAX : s[sub][e]);
            s[sub][e] = x;
            mx = fmaxf(mx, x);
          }
        const float m_new = fmaxf(m_run, mx);
        const float m_safe = m_new == -INFINITY ? 0.f : m_new;       // a lane's half of a tile may hold no key below T
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_safe);
        float rs = 0.f, ds = 0.f;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const float ex = __builtin_amdgcn_exp2f(s[sub][e] - m_safe);
            rs += ex;
            if (!DROP || ((kw >> (16 * sub + e)) & 1u)) ds += ex * dp[sub][e];
          }
        l_run = l_run * alpha + rs;
        d_run = d_run * alpha + ds;
        m_run = m_new;
      } else {
        V8 bf[2][2];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int col = j0 + 32 * sub + (e & 3) + 8 * (e >> 2) + 4 * h;
            const bool valid = rowok && col < a.T && col != gi;
            const float x = s[sub][e];
            const float p = valid ? __builtin_amdgcn_exp2f(x - m_run) * linv : 0.f;
            const float g = (!DROP || ((kw >> (16 * sub + e)) & 1u)) ? dp[sub][e] * a.inv_keep : 0.f;
            const float dsv = valid ? p * (g - dv) : 0.f;
            if (valid) tsum += (double)dsv * (double)x;
            bf[sub][e >> 3][e & 7] = (T)dsv;
          }
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
          for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
              dq[db] = MM<T>::mfma(frag_acc_order<T>(sKt + (32 * db + r) * PT + 32 * sub + 16 * s2 + 4 * h), bf[sub][s2], dq[db]);
      }
    }
    if (pass == 0) {
      // the two halves of the row (lane h = 0 / 1) meet; both lanes compute the same bits (the sums are symmetric)
      const float m_o = __shfl_xor(m_run, 32, 64), l_o = __shfl_xor(l_run, 32, 64), d_o = __shfl_xor(d_run, 32, 64);
      const float m = fmaxf(m_run, m_o);
      const float fa = __builtin_amdgcn_exp2f(m_run - m), fb = __builtin_amdgcn_exp2f(m_o - m);
      const float lt = l_run * fa + l_o * fb, dt = d_run * fa + d_o * fb;
      m_run = m;
      linv = 1.0f / lt;
      dv = dt * linv * a.inv_keep;
      if (h == 0 && rowok) { a.rmax[(long)bh * a.Tp + gi] = m; a.rinv[(long)bh * a.Tp + gi] = linv; a.dlt[(long)bh * a.Tp + gi] = dv; }
      return;
    }
  }
  const float sc = a.qscale * kLn2;
  if (rowok) {
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int d = 32 * db + 8 * g4 + 4 * h;
        *reinterpret_cast<float4*>(a.dqkv + ((long)b * a.T + gi) * (3 * HD) + hd * 64 + d) =
            make_float4(dq[db][4 * g4] * sc * sc_inv, dq[db][4 * g4 + 1] * sc * sc_inv, dq[db][4 * g4 + 2] * sc * sc_inv, dq[db][4 * g4 + 3] * sc * sc_inv);
      }
  }
  red[tid] = tsum;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int i = 0; i < 256; ++i) t += red[i];                 // fixed order
    a.tpart[(long)bh * gridDim.y + blockIdx.y] = t * 0.6931471805599453;
  }
}

// ------------------------------------------------------------------------------------------------ key side
template <typename T, bool DROP>
__global__ void __launch_bounds__(256, 2) lsa16_kv_kernel(Lsa16Args a) {
  typedef typename MM<T>::V8 V8;
  __shared__ __attribute__((aligned(16))) T sm[4 * TILE];
  __shared__ __attribute__((aligned(16))) float sst[3 * 64];
  T *sQ = sm, *sG = sm + TILE, *sQt = sm + 2 * TILE, *sGt = sm + 3 * TILE;
  const int bh = blockIdx.x, b = bh / a.H, hd = bh % a.H;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, r = l & 31, h = l >> 5;
  const int kj = blockIdx.y * 128 + 32 * w + r;
  const bool colok = kj < a.T;
  const int HD = a.H * 64, nqt = (a.T + 63) / 64, nktp = a.Tp / 64;
  const T* qg = reinterpret_cast<const T*>(a.q) + (long)bh * a.Tp * 64;
  const T* gg = reinterpret_cast<const T*>(a.g) + (long)bh * a.Tp * 64;
  const T* qtg = reinterpret_cast<const T*>(a.qt) + (long)bh * 64 * a.Tp;
  const T* gtg = reinterpret_cast<const T*>(a.gt) + (long)bh * 64 * a.Tp;
  V8 kf[4], vf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
    for (int u = 0; u < 8; ++u) kf[ks][u] = (T)0.f;
    if (colok) kf[ks] = *reinterpret_cast<const V8*>(reinterpret_cast<const T*>(a.k) + ((long)bh * a.Tp + kj) * 64 + 16 * ks + 8 * h);
    vf[ks] = *reinterpret_cast<const V8*>(reinterpret_cast<const T*>(a.vr) + ((long)bh * a.Tp + kj) * 64 + 16 * ks + 8 * h);
  }
  // the key's place in its 64-key tile: keep bit `kbit` of the word of stream `khs` (the forward's layout)
  const int kc = kj & 31, khs = (kc >> 2) & 1, kbit = 16 * ((kj >> 5) & 1) + (kc & 3) + 4 * (kc >> 3);
  const unsigned* mrow = DROP ? a.mask + ((long)(bh * nktp + (kj >> 6)) * 2 + khs) * a.Tp : nullptr;
  float sc_s, sc_inv;
  do_scale(*a.amax, sc_s, sc_inv);
  f32x16 dk[2], dvv[2];
#pragma unroll
  for (int e = 0; e < 16; ++e) { dk[0][e] = 0.f; dk[1][e] = 0.f; dvv[0][e] = 0.f; dvv[1][e] = 0.f; }

  for (int qt = 0; qt < nqt; ++qt) {
    const int i0 = qt * 64;
    __syncthreads();
    stage64<T>(qg + (long)i0 * 64, 64, a.T - i0, sQ);
    stage64<T>(gg + (long)i0 * 64, 64, 64, sG);
    stage64<T>(qtg + i0, a.Tp, 64, sQt);
    stage64<T>(gtg + i0, a.Tp, 64, sGt);
    if (tid < 64) {
      const bool ok = i0 + tid < a.T;
      const long o = (long)bh * a.Tp + i0 + tid;
      sst[tid] = ok ? a.rmax[o] : 0.f;
      sst[64 + tid] = ok ? a.rinv[o] : 0.f;
      sst[128 + tid] = ok ? a.dlt[o] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int ib = 0; ib < 2; ++ib) {
      f32x16 s, dp;
#pragma unroll
      for (int e = 0; e < 16; ++e) { s[e] = 0.f; dp[e] = 0.f; }
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int off = (32 * ib + r) * PT + 16 * ks + 8 * h;
        s = MM<T>::mfma(*reinterpret_cast<const V8*>(sQ + off), kf[ks], s);
        dp = MM<T>::mfma(*reinterpret_cast<const V8*>(sG + off), vf[ks], dp);
      }
      V8 pb[2], sb[2];
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int il = 32 * ib + 8 * g4 + 4 * h;      // accumulator elements 4 g4 .. 4 g4 + 3: queries i0 + il ..
        uint4 kw = make_uint4(~0u, ~0u, ~0u, ~0u);
        if (DROP && colok) kw = *reinterpret_cast<const uint4*>(mrow + i0 + il);
        const float4 m4 = *reinterpret_cast<const float4*>(sst + il), l4 = *reinterpret_cast<const float4*>(sst + 64 + il),
                     d4 = *reinterpret_cast<const float4*>(sst + 128 + il);
        const float mm[4] = {m4.x, m4.y, m4.z, m4.w}, ll[4] = {l4.x, l4.y, l4.z, l4.w}, dd[4] = {d4.x, d4.y, d4.z, d4.w};
        const unsigned kk[4] = {kw.x, kw.y, kw.z, kw.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int e = 4 * g4 + u, gi = i0 + il + u;
          const bool valid = colok && gi < a.T && gi != kj;
          const bool keep = !DROP || ((kk[u] >> kbit) & 1u);
          const float p = valid ? __builtin_amdgcn_exp2f(s[e] - mm[u]) * ll[u] : 0.f;
          const float pd = keep ? p * a.inv_keep : 0.f;
          const float dsv = valid ? p * ((keep ? dp[e] * a.inv_keep : 0.f) - dd[u]) : 0.f;
          pb[e >> 3][e & 7] = (T)pd;
          sb[e >> 3][e & 7] = (T)dsv;
        }
      }
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const int off = (32 * db + r) * PT + 32 * ib + 16 * s2 + 4 * h;
          dvv[db] = MM<T>::mfma(frag_acc_order<T>(sGt + off), pb[s2], dvv[db]);      // dV^T += dOr^T Pd
          dk[db] = MM<T>::mfma(frag_acc_order<T>(sQt + off), sb[s2], dk[db]);        // dK^T += Q^T dS
        }
    }
  }
  if (colok) {
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        float* o = a.dqkv + ((long)b * a.T + kj) * (3 * HD) + hd * 64 + 32 * db + 8 * g4 + 4 * h;
        *reinterpret_cast<float4*>(o + HD) = make_float4(dk[db][4 * g4] * kLn2 * sc_inv, dk[db][4 * g4 + 1] * kLn2 * sc_inv,
                                                         dk[db][4 * g4 + 2] * kLn2 * sc_inv, dk[db][4 * g4 + 3] * kLn2 * sc_inv);
        *reinterpret_cast<float4*>(o + 2 * HD) = make_float4(dvv[db][4 * g4] * sc_inv, dvv[db][4 * g4 + 1] * sc_inv, dvv[db][4 * g4 + 2] * sc_inv,
                                                             dvv[db][4 * g4 + 3] * sc_inv);
      }
  }
}

__global__ void lsa16_temp_fold_kernel(const double* __restrict__ part, int n, const unsigned* __restrict__ amax, float* __restrict__ out, int accumulate) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float s, inv;
    do_scale(*amax, s, inv);
    double t = 0.0;
    for (int i = 0; i < n; ++i) t += part[i];       // fixed order
    const float v = (float)(t * (double)inv);
    out[0] = accumulate ? out[0] + v : v;
  }
}

inline long up256(long n) { return (n + 255) & ~255L; }

struct Lsa16Ws {
  long amax, stats, tpart, planes, mask, total;
};
Lsa16Ws lsa16_ws(int B, int T, int Tp, int heads, float p) {
  const long BH = (long)B * heads;
  Lsa16Ws w;
  w.amax = 0;
  w.stats = 256;
  w.tpart = w.stats + up256(3 * BH * Tp * (long)sizeof(float));
  w.planes = w.tpart + up256(BH * ((T + 127) / 128) * (long)sizeof(double));
  w.mask = w.planes + 5 * up256(BH * Tp * 64 * 2);
  w.total = w.mask + (p > 0.f ? BH * Tp * (long)Tp / 8 : 0);
  return w;
}

template <typename T, bool DROP>
int lsa16_launch(const Lsa16Args& a, int B, hipStream_t st) {
  const dim3 gp(B * a.H, a.Tp / 64), gp3(B * a.H, a.Tp / 64, 3), grid(B * a.H, (a.T + 127) / 128);
  lsa16_prep_do_kernel<T><<<gp, 256, 0, st>>>(a);
  STEDM_LAUNCH_CHECK();
  lsa16_prep_planes_kernel<T><<<gp3, 256, 0, st>>>(a);
  STEDM_LAUNCH_CHECK();
  lsa16_q_kernel<T, DROP, 0><<<grid, 256, 0, st>>>(a);
  STEDM_LAUNCH_CHECK();
  lsa16_q_kernel<T, DROP, 1><<<grid, 256, 0, st>>>(a);
  STEDM_LAUNCH_CHECK();
  lsa16_kv_kernel<T, DROP><<<grid, 256, 0, st>>>(a);
  STEDM_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" long stedm_lsa_bwd16_ws_bytes(int B, int T, int Tp, int heads, float p) {
  if (B <= 0 || heads <= 0 || T <= 0 || Tp < T || Tp % 128 != 0) return 0;
  return lsa16_ws(B, T, Tp, heads, p).total;
}

extern "C" int stedm_lsa_bwd16(const void* q_hi, const void* k_hi, const void* vt_hi, const float* d_out, float* d_qkv, float* d_temp,
                               int accumulate_temp, float qscale, int B, int T, int Tp, int heads, int mm_dtype, float p, unsigned long long seed,
                               unsigned site, void* ws, void* stream) {
  STEDM_CHECK_ARG(q_hi && k_hi && vt_hi && d_out && d_qkv && d_temp && ws, "lsa_bwd16: null pointer");
  STEDM_CHECK_ARG(B > 0 && heads > 0 && Tp % 128 == 0 && Tp >= T && T > 1, "lsa_bwd16: need Tp %% 128 == 0, Tp >= T > 1");
  STEDM_CHECK_ARG(mm_dtype == STEDM_F16 || mm_dtype == STEDM_BF16, "lsa_bwd16: bad mm_dtype");
  STEDM_CHECK_ARG(p >= 0.f && p < 1.f, "lsa_bwd16: p must be in [0, 1)");
  STEDM_CHECK_ARG(((reinterpret_cast<uintptr_t>(d_out) | reinterpret_cast<uintptr_t>(d_qkv) | reinterpret_cast<uintptr_t>(q_hi) |
                    reinterpret_cast<uintptr_t>(k_hi) | reinterpret_cast<uintptr_t>(vt_hi) | reinterpret_cast<uintptr_t>(ws)) & 15) == 0,
                  "lsa_bwd16: operands must be 16-byte aligned");
  const unsigned thr = (unsigned)lrint((double)p * 65536.0);
  STEDM_CHECK_ARG(thr <= 65535u, "lsa_bwd16: p too close to 1");
  const Lsa16Ws w = lsa16_ws(B, T, Tp, heads, p);
  char* base = reinterpret_cast<char*>(ws);
  const long nbt = (long)B * heads * Tp, plane = up256(nbt * 64 * 2);
  float* stats = reinterpret_cast<float*>(base + w.stats);
  Lsa16Args a{q_hi, k_hi, vt_hi, d_out, d_qkv, reinterpret_cast<unsigned*>(base + w.amax), stats, stats + nbt, stats + 2 * nbt,
              reinterpret_cast<double*>(base + w.tpart), base + w.planes, base + w.planes + plane, base + w.planes + 2 * plane,
              base + w.planes + 3 * plane, base + w.planes + 4 * plane, reinterpret_cast<unsigned*>(base + w.mask), T, Tp, heads, qscale, thr, site,
              seed, p > 0.f ? 1.0f / (1.0f - p) : 1.0f};
  hipStream_t st = as_stream(stream);
  STEDM_HIP_TRY(hipMemsetAsync(a.amax, 0, sizeof(unsigned), st));
  const long n4 = (long)B * T * heads * 16;
  lsa16_amax_kernel<<<(int)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048), 256, 0, st>>>(d_out, n4, a.amax);
  STEDM_LAUNCH_CHECK();
  int rc;
  if (mm_dtype == STEDM_F16) rc = p > 0.f ? lsa16_launch<_Float16, true>(a, B, st) : lsa16_launch<_Float16, false>(a, B, st);
  else rc = p > 0.f ? lsa16_launch<__bf16, true>(a, B, st) : lsa16_launch<__bf16, false>(a, B, st);
  if (rc) return rc;
  lsa16_temp_fold_kernel<<<1, 64, 0, st>>>(a.tpart, B * heads * ((T + 127) / 128), a.amax, d_temp, accumulate_temp);
  STEDM_LAUNCH_CHECK();
  return 0;
}
