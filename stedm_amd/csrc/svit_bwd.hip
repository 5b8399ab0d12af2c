// Backward of the set-ViT style encoder (networks/vit_set.py); the forward is svit.hip. fp32 (the cancelling sum of d temperature is carried
// in fp64), no atomics: every reduction has a fixed order.
//
//   lsa_bwd          : LSA.forward (vit_set.py:52-66) reversed, flash-style (nothing T x T is materialised), from the operand planes the
//                      forward's qkv_pack wrote. Two kernels over 64 x 64 tiles on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32, the
//                      pattern of attn64_bwd_mfma_kernel, attn_bwd.hip), 16-bit operands widened on load (hi, or hi + lo):
//                        q kernel  (sample-head, 64 queries) walks the key tiles twice: first the row statistics - the log-sum-exp as its
//                                  two parts, row maximum and 1 / row sum (P = exp2(s - max) / sum keeps the relative accuracy of the
//                                  exponential, which exp2(s - LSE) loses to the rounding of a large LSE) - and
//                                  D = sum_j Pd dP (= rowsum(dO o O)), online; then dS = P o (keep / (1 - p) dP - D), dQ += dS K and the
//                                  block's partial of d temperature = sum dS o dots;
//                        kv kernel (sample-head, 64 keys) walks the query tiles: dV += Pd^T dO, dK += dS^T Q.
//                      The keep bits of the probability dropout are regenerated from the forward's (seed, site) streams (dropmask.hpp): a
//                      stream belongs to one query and runs along the keys, so the q kernel just follows it, the kv kernel advances it to
//                      its key tile for every query.
//   gelu_bwd         : dpre = dh gelu'(pre), exact erf GELU (FeedForward, vit_set.py:24-31)
//   svit_head_bwd    : mlp_head (LayerNorm, Linear) and the token pool reversed (vit_set.py:191-206, c_old = None)
//   svit_tok_bwd     : stedm_svit_tok_place reversed (d pos_embedding, d cls_token, patch-token rows)
//   svit_patch_gather: the fp32 patch rows stedm_svit_patch_ln16 normalises (operand of the patch LayerNorm's backward)
//   widen16          : 16-bit operand planes (hi, or hi + lo) -> fp32 (the operands of the fp32 weight-gradient GEMMs)
#include <float.h>

#include "common.hpp"
#include "dropmask.hpp"
using namespace stedm;

namespace {

typedef float bwd_f32x16 __attribute__((ext_vector_type(16)));
constexpr int LP = 68;                  // row pitch (floats) of the 64 x 64 LDS tiles: 16-B aligned rows, fragment reads spread over the banks
constexpr int TILE_F = 64 * LP;
constexpr float kLn2 = 0.6931471805599453f;
constexpr int LSA_BWD_LDS = 6 * TILE_F * (int)sizeof(float);

struct LsaBwdArgs {
  const void *qh, *ql, *kh, *kl, *vh, *vl;   // q, k [B*H][Tp][64] (q scaled by exp(temperature) log2 e), vt [B*H][64][Tp]
  const float* dO;                           // [B*T][H*64]
  float* dqkv;                               // [B*T][3*H*64], to_qkv's output order (q | k | v, each '(h d)')
  float* rmax;                               // [B*H][Tp] row maximum of the masked log2-domain logits   } the two parts of the
  float* rinv;                               // [B*H][Tp] 1 / sum_j exp2(s_j - max)                      } row's log-sum-exp
  float* dlt;                                // [B*H][Tp] D
  double* tpart;                             // [B*H * ntiles] partial sums of d temperature
  int T, Tp, H;
  float qscale;                              // exp(temperature) * log2 e
  unsigned thr16, site;
  unsigned long long seed;
  float inv_keep;
};

template <typename T>
__device__ __forceinline__ void widen8(const T* hi, const T* lo, long off, float (&v)[8]) {
  typedef T V8 __attribute__((ext_vector_type(8)));
  const V8 a = *reinterpret_cast<const V8*>(hi + off);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (float)a[j];
  if (lo) {
    const V8 b = *reinterpret_cast<const V8*>(lo + off);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] += (float)b[j];
  }
}

// 64 rows of a [.][64] plane from element offset `base` -> dst [64][LP]; rows >= nvalid are zero (the pad rows of the planes are never read)
template <typename T>
__device__ __forceinline__ void load_rows(const T* hi, const T* lo, long base, int nvalid, float* dst) {
  for (int c = threadIdx.x; c < 512; c += 256) {
    const int row = c >> 3, c8 = (c & 7) * 8;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (row < nvalid) widen8(hi, lo, base + row * 64 + c8, v);
    *reinterpret_cast<float4*>(dst + row * LP + c8) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(dst + row * LP + c8 + 4) = make_float4(v[4], v[5], v[6], v[7]);
  }
}

// 64 keys of the V^T plane [64][Tp] from element offset `base` (row 0, first key) -> dst [key][channel]; keys >= nvalid are zero
template <typename T>
__device__ __forceinline__ void load_vt(const T* hi, const T* lo, long base, int Tp, int nvalid, float* dst) {
  for (int c = threadIdx.x; c < 512; c += 256) {
    const int d = c >> 3, j8 = (c & 7) * 8;
    float v[8];
    widen8(hi, lo, base + (long)d * Tp + j8, v);
#pragma unroll
    for (int u = 0; u < 8; ++u) dst[(j8 + u) * LP + d] = j8 + u < nvalid ? v[u] : 0.f;
  }
}

// 64 rows x 64 channels of dO from row `row0`, channel `hoff` -> dst [64][LP]; rows >= nvalid are zero
__device__ __forceinline__ void load_do(const float* dO, long row0, int ldo, int hoff, int nvalid, float* dst) {
  for (int c = threadIdx.x; c < 1024; c += 256) {
    const int row = c >> 4, c4 = (c & 15) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < nvalid) v = *reinterpret_cast<const float4*>(dO + (row0 + row) * ldo + hoff + c4);
    *reinterpret_cast<float4*>(dst + row * LP + c4) = v;
  }
}

// 32 x 32 tile of A B^T over the 64 channels; a, b: the lane's rows of the two [.][LP] images, at channel 4 * (lane >> 5)
// (MFMA n of a step contracts channels c0 + n and c0 + 4 + n, as attn64_bwd_mfma_kernel)
__device__ __forceinline__ bwd_f32x16 mm_abt(const float* a, const float* b) {
  bwd_f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll 2
  for (int c0 = 0; c0 < 64; c0 += 8) {
    const float4 x = *reinterpret_cast<const float4*>(a + c0), y = *reinterpret_cast<const float4*>(b + c0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.x, y.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.y, y.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.z, y.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x.w, y.w, acc, 0, 0, 0);
  }
  return acc;
}

// acc += A B over 64 contraction rows: a0 = the lane's A element of row 0 (+ lane >> 5), ak its stride along the contraction; bp = the
// lane's B column in a [64][LP] image, at row lane >> 5
__device__ __forceinline__ void mm_acc(bwd_f32x16& acc, const float* a0, int ak, const float* bp) {
#pragma unroll 8
  for (int k0 = 0; k0 < 64; k0 += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[k0 * ak], bp[k0 * LP], acc, 0, 0, 0);
}

// accumulator element e of a lane (r = lane & 31, hh = lane >> 5) is row (e & 3) + 8 (e >> 2) + 4 hh, column r of the 32 x 32 tile
__device__ __forceinline__ void store_tile(float* dst, const bwd_f32x16& acc, int row0, int col0, int r, int hh) {
#pragma unroll
  for (int e = 0; e < 16; ++e) dst[(row0 + (e & 3) + 8 * (e >> 2) + 4 * hh) * LP + col0 + r] = acc[e];
}

// keep bit of key 16 qd + n of a 64-key tile, from the tile's two words of the query's streams (w0: stream 0, w1: stream 1). The forward
// (lsa_flash_kernel) holds key sub * 32 + (e & 3) + 8 (e >> 2) + 4 h of a tile in bit sub * 16 + e of stream h.
__device__ __forceinline__ bool keep_bit(unsigned w0, unsigned w1, int qd, int n) {
  const unsigned w = (n >> 2) & 1 ? w1 : w0;
  return (w >> ((qd >> 1) * 16 + (n & 3) + 8 * (qd & 1) + 4 * (n >> 3))) & 1u;
}

__device__ __forceinline__ void read_row16(const float* p, float (&x)[16]) {
#pragma unroll
  for (int n = 0; n < 4; ++n) {
    const float4 t = *reinterpret_cast<const float4*>(p + 4 * n);
    x[4 * n] = t.x; x[4 * n + 1] = t.y; x[4 * n + 2] = t.z; x[4 * n + 3] = t.w;
  }
}
__device__ __forceinline__ void write_row16(float* p, const float (&x)[16]) {
#pragma unroll
  for (int n = 0; n < 4; ++n) *reinterpret_cast<float4*>(p + 4 * n) = make_float4(x[4 * n], x[4 * n + 1], x[4 * n + 2], x[4 * n + 3]);
}

// ------------------------------------------------------------------------------------------------ LSA backward, query side
// grid (B*H, ceil(T / 64)). Four waves: wave (ti, tj) owns the 32 x 32 tile (ti, tj) of every 64 x 64 product; the row work (softmax
// statistics, dS) is done by four lanes per query row, 16 keys each, the sums meeting by xor-shuffles.
template <typename T, bool DROP>
__global__ void __launch_bounds__(256) lsa_bwd_q_kernel(LsaBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float *sQ = sm, *sG = sm + TILE_F, *sK = sm + 2 * TILE_F, *sV = sm + 3 * TILE_F, *sS = sm + 4 * TILE_F, *sD = sm + 5 * TILE_F;
  __shared__ double red[256];
  const int bh = blockIdx.x, b = bh / a.H, hd = bh % a.H;
  const int i0 = blockIdx.y * 64, nq = min(64, a.T - i0);
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, r = l & 31, hh = l >> 5, ti = w >> 1, tj = w & 1;
  const T* qg[2] = {reinterpret_cast<const T*>(a.qh), reinterpret_cast<const T*>(a.ql)};
  const T* kg[2] = {reinterpret_cast<const T*>(a.kh), reinterpret_cast<const T*>(a.kl)};
  const T* vg[2] = {reinterpret_cast<const T*>(a.vh), reinterpret_cast<const T*>(a.vl)};
  const int HD = a.H * 64;
  load_rows<T>(qg[0], qg[1], ((long)bh * a.Tp + i0) * 64, nq, sQ);
  load_do(a.dO, (long)b * a.T + i0, HD, hd * 64, nq, sG);
  const int row = tid >> 2, qd = tid & 3, gi = i0 + row;
  const bool rowok = row < nq;
  const int ntiles = (a.T + 63) / 64;
  float m_run = -INFINITY, l_run = 0.f, d_run = 0.f, linv = 0.f, dv = 0.f;
  double tsum = 0.0;      // sum dS o dots cancels heavily (every row of dS sums to zero): products and sums in fp64
  bwd_f32x16 dq;
#pragma unroll
  for (int e = 0; e < 16; ++e) dq[e] = 0.f;

  for (int pass = 0; pass < 2; ++pass) {
    U4 st{};
    if (DROP && rowok && qd < 2) st = attn_stream_init((unsigned)gi, (unsigned)bh, a.site, (unsigned)qd, a.seed);
    for (int kt = 0; kt < ntiles; ++kt) {
      const int j0 = kt * 64, nk = min(64, a.T - j0);
      __syncthreads();          // every wave is done with the previous key tile's images before they are overwritten
      load_rows<T>(kg[0], kg[1], ((long)bh * a.Tp + j0) * 64, nk, sK);
      load_vt<T>(vg[0], vg[1], (long)bh * 64 * a.Tp + j0, a.Tp, nk, sV);
      __syncthreads();          // the K / V images of this tile (and, before the first tile, the q / dO images) are complete
      {
        const bwd_f32x16 S = mm_abt(sQ + (32 * ti + r) * LP + 4 * hh, sK + (32 * tj + r) * LP + 4 * hh);
        const bwd_f32x16 P = mm_abt(sG + (32 * ti + r) * LP + 4 * hh, sV + (32 * tj + r) * LP + 4 * hh);
        store_tile(sS, S, 32 * ti, 32 * tj, r, hh);
        store_tile(sD, P, 32 * ti, 32 * tj, r, hh);
      }
      __syncthreads();
      float x[16], dp[16];
      read_row16(sS + row * LP + 16 * qd, x);
      read_row16(sD + row * LP + 16 * qd, dp);
      unsigned w0 = ~0u, w1 = ~0u;
      if (DROP) {               // lane qd = 0 / 1 of a row follows stream 0 / 1; all four lanes of the row take both words from them
        const unsigned mine = (rowok && qd < 2) ? attn_keep_bits(st, a.thr16) : ~0u;
        w0 = __shfl(mine, l & ~3);
        w1 = __shfl(mine, (l & ~3) + 1);
      }
      if (pass == 0) {
        // logits in the log2 domain; the diagonal is masked to -FLT_MAX (vit_set.py:58-60), keys beyond T do not exist
        float mx = -INFINITY;
#pragma unroll
        for (int n = 0; n < 16; ++n) {
          const int col = j0 + 16 * qd + n;
          x[n] = col >= a.T ? -INFINITY : (col == gi ? -FLT_MAX : x[n]);
          mx = fmaxf(mx, x[n]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 1)); mx = fmaxf(mx, __shfl_xor(mx, 2));
        const float m_new = fmaxf(m_run, mx);            // finite from the first tile on (T > 1: it holds a key other than the query)
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        float rs = 0.f, ds = 0.f;
#pragma unroll
        for (int n = 0; n < 16; ++n) {
          const float e = __builtin_amdgcn_exp2f(x[n] - m_new);
          rs += e;
          if (!DROP || keep_bit(w0, w1, qd, n)) ds += e * dp[n];
        }
        rs += __shfl_xor(rs, 1); rs += __shfl_xor(rs, 2);
        ds += __shfl_xor(ds, 1); ds += __shfl_xor(ds, 2);
        l_run = l_run * alpha + rs;
        d_run = d_run * alpha + ds;
        m_run = m_new;
      } else {
        float dsv[16];
#pragma unroll
        for (int n = 0; n < 16; ++n) {
          const int col = j0 + 16 * qd + n;
          const bool valid = rowok && col < a.T && col != gi;
          const float p = valid ? __builtin_amdgcn_exp2f(x[n] - m_run) * linv : 0.f;
          const float g = (!DROP || keep_bit(w0, w1, qd, n)) ? dp[n] * a.inv_keep : 0.f;
          dsv[n] = valid ? p * (g - dv) : 0.f;
          if (valid) tsum += (double)dsv[n] * (double)x[n];
        }
        write_row16(sD + row * LP + 16 * qd, dsv);
        __syncthreads();
        mm_acc(dq, sD + (32 * ti + r) * LP + hh, 1, sK + hh * LP + 32 * tj + r);      // dQ += dS K
      }
    }
    if (pass == 0) {
      linv = 1.0f / l_run;
      dv = d_run * linv * a.inv_keep;
      if (qd == 0 && rowok) { a.rmax[(long)bh * a.Tp + gi] = m_run; a.rinv[(long)bh * a.Tp + gi] = linv; a.dlt[(long)bh * a.Tp + gi] = dv; }
    }
  }
  // q of the planes = q exp(temperature) log2 e: the chain rule through the scale, and log2 -> natural logits
  const float sc = a.qscale * kLn2;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int rl = 32 * ti + (e & 3) + 8 * (e >> 2) + 4 * hh;
    if (rl < nq) a.dqkv[((long)b * a.T + i0 + rl) * (3 * HD) + hd * 64 + 32 * tj + r] = dq[e] * sc;
  }
  red[tid] = tsum;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < 256; ++i) s += red[i];                 // fixed order
    a.tpart[(long)bh * gridDim.y + blockIdx.y] = s * 0.6931471805599453;      // dots = log2-domain logits * ln 2
  }
}

// ------------------------------------------------------------------------------------------------ LSA backward, key side
// grid (B*H, ceil(T / 64)): the block's 64 keys against every query tile. Wave (ti, tj) owns the tile (queries 32 ti.., keys 32 tj..) of
// S / dP as in the q kernel, and rows (keys) 32 ti.., channels 32 tj.. of dK and dV.
template <typename T, bool DROP>
__global__ void __launch_bounds__(256) lsa_bwd_kv_kernel(LsaBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float *sQ = sm, *sG = sm + TILE_F, *sK = sm + 2 * TILE_F, *sV = sm + 3 * TILE_F, *sS = sm + 4 * TILE_F, *sD = sm + 5 * TILE_F;
  const int bh = blockIdx.x, b = bh / a.H, hd = bh % a.H;
  const int kt = blockIdx.y, j0 = kt * 64, nk = min(64, a.T - j0);
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, r = l & 31, hh = l >> 5, ti = w >> 1, tj = w & 1;
  const T* qg[2] = {reinterpret_cast<const T*>(a.qh), reinterpret_cast<const T*>(a.ql)};
  const T* kg[2] = {reinterpret_cast<const T*>(a.kh), reinterpret_cast<const T*>(a.kl)};
  const T* vg[2] = {reinterpret_cast<const T*>(a.vh), reinterpret_cast<const T*>(a.vl)};
  const int HD = a.H * 64;
  load_rows<T>(kg[0], kg[1], ((long)bh * a.Tp + j0) * 64, nk, sK);
  load_vt<T>(vg[0], vg[1], (long)bh * 64 * a.Tp + j0, a.Tp, nk, sV);
  const int row = tid >> 2, qd = tid & 3;
  const int ntiles = (a.T + 63) / 64;
  bwd_f32x16 dk, dvv;
#pragma unroll
  for (int e = 0; e < 16; ++e) { dk[e] = 0.f; dvv[e] = 0.f; }
  for (int qt = 0; qt < ntiles; ++qt) {
    const int i0 = qt * 64, nq = min(64, a.T - i0), gi = i0 + row;
    const bool rowok = row < nq;
    __syncthreads();
    load_rows<T>(qg[0], qg[1], ((long)bh * a.Tp + i0) * 64, nq, sQ);
    load_do(a.dO, (long)b * a.T + i0, HD, hd * 64, nq, sG);
    __syncthreads();
    {
      const bwd_f32x16 S = mm_abt(sQ + (32 * ti + r) * LP + 4 * hh, sK + (32 * tj + r) * LP + 4 * hh);
      const bwd_f32x16 P = mm_abt(sG + (32 * ti + r) * LP + 4 * hh, sV + (32 * tj + r) * LP + 4 * hh);
      store_tile(sS, S, 32 * ti, 32 * tj, r, hh);
      store_tile(sD, P, 32 * ti, 32 * tj, r, hh);
    }
    __syncthreads();
    float x[16], dp[16];
    read_row16(sS + row * LP + 16 * qd, x);
    read_row16(sD + row * LP + 16 * qd, dp);
    unsigned w0 = ~0u, w1 = ~0u;
    if (DROP) {
      unsigned mine = ~0u;
      if (rowok && qd < 2) {     // lane qd = 0 / 1 of a row: stream 0 / 1 of the query. It runs along the keys: advance it to this
        U4 st = attn_stream_init((unsigned)gi, (unsigned)bh, a.site, (unsigned)qd, a.seed);      // block's tile (16 words per tile)
        for (int t = 0; t < 16 * kt; ++t) xs128_next(st);
        mine = attn_keep_bits(st, a.thr16);
      }
      w0 = __shfl(mine, l & ~3);
      w1 = __shfl(mine, (l & ~3) + 1);
    }
    const float m_row = rowok ? a.rmax[(long)bh * a.Tp + gi] : 0.f, linv = rowok ? a.rinv[(long)bh * a.Tp + gi] : 0.f;
    const float dv = rowok ? a.dlt[(long)bh * a.Tp + gi] : 0.f;
    float pdv[16], dsv[16];
#pragma unroll
    for (int n = 0; n < 16; ++n) {
      const int col = j0 + 16 * qd + n;
      const bool valid = rowok && col < a.T && col != gi;
      const bool keep = !DROP || keep_bit(w0, w1, qd, n);
      const float p = valid ? __builtin_amdgcn_exp2f(x[n] - m_row) * linv : 0.f;
      pdv[n] = keep ? p * a.inv_keep : 0.f;
      dsv[n] = valid ? p * ((keep ? dp[n] * a.inv_keep : 0.f) - dv) : 0.f;
    }
    write_row16(sS + row * LP + 16 * qd, pdv);
    write_row16(sD + row * LP + 16 * qd, dsv);
    __syncthreads();
    mm_acc(dvv, sS + hh * LP + 32 * ti + r, LP, sG + hh * LP + 32 * tj + r);     // dV += Pd^T dO
    mm_acc(dk, sD + hh * LP + 32 * ti + r, LP, sQ + hh * LP + 32 * tj + r);      // dK += dS^T Q
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int rl = 32 * ti + (e & 3) + 8 * (e >> 2) + 4 * hh;
    if (rl < nk) {
      float* o = a.dqkv + ((long)b * a.T + j0 + rl) * (3 * HD) + hd * 64 + 32 * tj + r;
      o[HD] = dk[e] * kLn2;           // the q plane carries exp(temperature) log2 e
      o[2 * HD] = dvv[e];
    }
  }
}

__global__ void lsa_bwd_temp_fold_kernel(const double* __restrict__ part, int n, float* __restrict__ out, int accumulate) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += part[i];       // fixed order
    out[0] = accumulate ? out[0] + (float)s : (float)s;
  }
}

template <typename T, bool DROP>
int lsa_bwd_launch(const LsaBwdArgs& a, int B, hipStream_t st) {
  static bool attr = false;
  if (!attr) {
    STEDM_HIP_TRY(hipFuncSetAttribute((const void*)lsa_bwd_q_kernel<T, DROP>, hipFuncAttributeMaxDynamicSharedMemorySize, LSA_BWD_LDS));
    STEDM_HIP_TRY(hipFuncSetAttribute((const void*)lsa_bwd_kv_kernel<T, DROP>, hipFuncAttributeMaxDynamicSharedMemorySize, LSA_BWD_LDS));
    attr = true;
  }
  const dim3 grid(B * a.H, (a.T + 63) / 64);
  lsa_bwd_q_kernel<T, DROP><<<grid, 256, LSA_BWD_LDS, st>>>(a);
  STEDM_LAUNCH_CHECK();
  lsa_bwd_kv_kernel<T, DROP><<<grid, 256, LSA_BWD_LDS, st>>>(a);
  STEDM_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------ elementwise pieces
__global__ void __launch_bounds__(256) gelu_bwd_kernel(const float* __restrict__ pre, const float* dh, float* dpre, long n) {      // (dpre may alias dh)
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float x = pre[i];
    const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752f));
    const float pdf = 0.3989422804014327f * __expf(-0.5f * x * x);
    dpre[i] = dh[i] * (cdf + x * pdf);
  }
}

template <typename T>
__global__ void __launch_bounds__(256) widen16_kernel(const T* __restrict__ hi, const T* __restrict__ lo, float* __restrict__ out, long n) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) out[i] = lo ? (float)hi[i] + (float)lo[i] : (float)hi[i];
}

// rows[(b * ntok + hp * pw + wp)][(p1 * p + p2) * 3 ns + c * ns + s] = img[b][s][hp * p + p1][wp * p + p2][c] (svit_patch_ln16_kernel's gather)
__global__ void __launch_bounds__(256) svit_patch_gather_kernel(const float* __restrict__ img, float* __restrict__ rows, int ns, int H, int W, int p,
                                                                long total) {
  const int C = 3 * ns, pd = p * p * C, pw = W / p, ntok = (H / p) * pw;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int f = (int)(i % pd);
    const long rw = i / pd;
    const int tok = (int)(rw % ntok);
    const long b = rw / ntok;
    const int hp = tok / pw, wp = tok - hp * pw;
    const int px = f / C, ch = f - px * C;
    const int p1 = px / p, p2 = px - p1 * p;
    const int c = ch / ns, s = ch - c * ns;
    rows[i] = img[((((long)b * ns + s) * H + hp * p + p1) * W + wp * p + p2) * 3 + c];
  }
}

// x [B][ntok + 2][dim] gradient -> d pos [ntok + 2][dim] (batch sum, ascending b), d cls [dim] (= the batch sum of token 0),
// d tok [B * ntok][dim] (tokens 2..); token 1 is the constant zero time token
__global__ void __launch_bounds__(256) svit_tok_bwd_kernel(const float* __restrict__ dx, float* __restrict__ dpos, float* __restrict__ dcls,
                                                           float* __restrict__ dtok, int B, int ntok, int dim, int accumulate) {
  const long total = (long)(ntok + 2) * dim;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int t = (int)(i / dim), k = (int)(i - (long)t * dim);
    float s = 0.f;
    for (int b = 0; b < B; ++b) {
      const float v = dx[((long)b * (ntok + 2) + t) * dim + k];
      s += v;
      if (t >= 2) dtok[((long)b * ntok + t - 2) * dim + k] = v;
    }
    dpos[i] = accumulate ? dpos[i] + s : s;
    if (t == 0) dcls[k] = accumulate ? dcls[k] + s : s;
  }
}

// ------------------------------------------------------------------------------------------------ head backward
// block b: pooled row (recomputed from x), LayerNorm statistics, z = LN(pooled) (the Linear's operand), dz = d_out W, the sample's
// dgamma / dbeta rows and d pooled -> ws [4][B][dim] (z | dgamma_b | dbeta_b | dpool)
__global__ void __launch_bounds__(256) svit_head_bwd_kernel(const float* __restrict__ x, int Tn, int dim, int pool, const float* __restrict__ g,
                                                            const float* __restrict__ bt, float eps, const float* __restrict__ wh,
                                                            const float* __restrict__ d_out, int ncls, float* __restrict__ ws, int B) {
  extern __shared__ float sp[];    // [dim] pooled -> xh, [dim] dz g
  __shared__ float red[4];
  float* sd = sp + dim;
  const int b = blockIdx.x;
  const float* px = x + (long)b * Tn * dim;
  for (int n = threadIdx.x; n < dim; n += 256) {
    float s = 0.f;
    if (pool == 1) s = px[n];
    else {
      for (int t = 0; t < Tn; ++t) s += px[(long)t * dim + n];      // fixed order
      s /= (float)Tn;
    }
    sp[n] = s;
  }
  __syncthreads();
  float s1 = 0.f;
  for (int n = threadIdx.x; n < dim; n += 256) s1 += sp[n];
  const float mean = block_sum_256(s1, red) / dim;
  float s2 = 0.f;
  for (int n = threadIdx.x; n < dim; n += 256) { const float d = sp[n] - mean; s2 += d * d; }
  const float rstd = 1.0f / sqrtf(block_sum_256(s2, red) / dim + eps);
  __syncthreads();
  float a1 = 0.f, a2 = 0.f;
  for (int n = threadIdx.x; n < dim; n += 256) {
    const float xh = (sp[n] - mean) * rstd;
    float dz = 0.f;
    for (int c = 0; c < ncls; ++c) dz = fmaf(d_out[(long)b * ncls + c], wh[(long)c * dim + n], dz);
    ws[((long)0 * B + b) * dim + n] = xh * g[n] + bt[n];
    ws[((long)1 * B + b) * dim + n] = dz * xh;
    ws[((long)2 * B + b) * dim + n] = dz;
    const float dxh = dz * g[n];
    sp[n] = xh; sd[n] = dxh;
    a1 += dxh; a2 += dxh * xh;
  }
  const float m1 = block_sum_256(a1, red) / dim;
  const float m2 = block_sum_256(a2, red) / dim;
  for (int n = threadIdx.x; n < dim; n += 256) ws[((long)3 * B + b) * dim + n] = rstd * (sd[n] - m1 - sp[n] * m2);
}

// parameter gradients of the head from the per-sample rows (ascending b): d ln_w, d ln_b [dim]; d W [ncls][dim]; d bias [ncls]
__global__ void __launch_bounds__(256) svit_head_bwd_fold_kernel(const float* __restrict__ ws, const float* __restrict__ d_out, int B, int dim, int ncls,
                                                                 float* __restrict__ dg, float* __restrict__ db, float* __restrict__ dw,
                                                                 float* __restrict__ dbias, int accumulate) {
  const long total = (long)ncls * dim + 2 * dim + ncls;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    float s = 0.f;
    float* dst;
    if (i < (long)ncls * dim) {
      const int c = (int)(i / dim), k = (int)(i - (long)c * dim);
      for (int b = 0; b < B; ++b) s = fmaf(d_out[(long)b * ncls + c], ws[(long)b * dim + k], s);
      dst = dw + i;
    } else if (i < (long)ncls * dim + 2 * dim) {
      const int j = (int)(i - (long)ncls * dim), wsel = j / dim, k = j - wsel * dim;
      for (int b = 0; b < B; ++b) s += ws[((long)(1 + wsel) * B + b) * dim + k];
      dst = (wsel == 0 ? dg : db) + k;
    } else {
      const int c = (int)(i - (long)ncls * dim - 2 * dim);
      for (int b = 0; b < B; ++b) s += d_out[(long)b * ncls + c];
      dst = dbias + c;
    }
    *dst = accumulate ? *dst + s : s;
  }
}

// dx [B][T][dim]: mean pool -> every token gets d pooled / T; cls pool -> token 0 gets it, the others zero
__global__ void __launch_bounds__(256) svit_pool_bwd_kernel(const float* __restrict__ dpool, float* __restrict__ dx, int Tn, int dim, int pool, long total) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int k = (int)(i % dim);
    const long rw = i / dim;
    const int t = (int)(rw % Tn);
    const long b = rw / Tn;
    const float v = dpool[b * dim + k];
    dx[i] = pool == 1 ? (t == 0 ? v : 0.f) : v / (float)Tn;
  }
}

inline int grid_for(long n, int cap = 65536) { return (int)((n + 255) / 256 < cap ? (n + 255) / 256 : cap); }

}  // namespace

extern "C" long stedm_lsa_bwd_ws_floats(int B, int T, int Tp, int heads) {
  return (long)B * heads * (3L * Tp + 2L * ((T + 63) / 64));      // three row arrays, then one fp64 partial per (sample-head, query tile)
}

extern "C" int stedm_lsa_bwd(const void* q_hi, const void* q_lo, const void* k_hi, const void* k_lo, const void* vt_hi, const void* vt_lo,
                             const float* d_out, float* d_qkv, float* d_temp, int accumulate_temp, float qscale, int B, int T, int Tp, int heads,
                             int mm_dtype, float p, unsigned long long seed, unsigned site, float* ws, void* stream) {
  STEDM_CHECK_ARG(q_hi && k_hi && vt_hi && d_out && d_qkv && d_temp && ws, "lsa_bwd: null pointer");
  STEDM_CHECK_ARG((!q_lo && !k_lo && !vt_lo) || (q_lo && k_lo && vt_lo), "lsa_bwd: lo planes come for all of q, k, vt or for none");
  STEDM_CHECK_ARG(B > 0 && heads > 0 && Tp % 128 == 0 && Tp >= T && T > 1, "lsa_bwd: need Tp %% 128 == 0, Tp >= T > 1");
  STEDM_CHECK_ARG(mm_dtype == STEDM_F16 || mm_dtype == STEDM_BF16, "lsa_bwd: bad mm_dtype");
  STEDM_CHECK_ARG(p >= 0.f && p < 1.f, "lsa_bwd: p must be in [0, 1)");
  STEDM_CHECK_ARG(((reinterpret_cast<uintptr_t>(d_out) | reinterpret_cast<uintptr_t>(q_hi) | reinterpret_cast<uintptr_t>(k_hi) |
                    reinterpret_cast<uintptr_t>(vt_hi) | reinterpret_cast<uintptr_t>(q_lo) | reinterpret_cast<uintptr_t>(k_lo) |
                    reinterpret_cast<uintptr_t>(vt_lo) | reinterpret_cast<uintptr_t>(ws)) & 15) == 0, "lsa_bwd: operands must be 16-byte aligned");
  const unsigned thr = (unsigned)lrint((double)p * 65536.0);
  STEDM_CHECK_ARG(thr <= 65535u, "lsa_bwd: p too close to 1");
  const long nbt = (long)B * heads * Tp;
  const int nt = (T + 63) / 64;
  LsaBwdArgs a{q_hi, q_lo, k_hi, k_lo, vt_hi, vt_lo, d_out, d_qkv, ws, ws + nbt, ws + 2 * nbt, reinterpret_cast<double*>(ws + 3 * nbt), T, Tp, heads,
               qscale, thr, site, seed,
               p > 0.f ? 1.0f / (1.0f - p) : 1.0f};
  hipStream_t st = as_stream(stream);
  int rc;
  if (mm_dtype == STEDM_F16) rc = p > 0.f ? lsa_bwd_launch<_Float16, true>(a, B, st) : lsa_bwd_launch<_Float16, false>(a, B, st);
  else rc = p > 0.f ? lsa_bwd_launch<__bf16, true>(a, B, st) : lsa_bwd_launch<__bf16, false>(a, B, st);
  if (rc) return rc;
  lsa_bwd_temp_fold_kernel<<<1, 64, 0, st>>>(a.tpart, B * heads * nt, d_temp, accumulate_temp);
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int stedm_gelu_bwd(const float* pre, const float* dh, float* dpre, long n, void* stream) {
  STEDM_CHECK_ARG(pre && dh && dpre && n > 0, "gelu_bwd: bad args");
  gelu_bwd_kernel<<<grid_for(n), 256, 0, as_stream(stream)>>>(pre, dh, dpre, n);
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int stedm_widen16(const void* hi, const void* lo, float* out, long n, int mm_dtype, void* stream) {
  STEDM_CHECK_ARG(hi && out && n > 0, "widen16: bad args");
  STEDM_CHECK_ARG(mm_dtype == STEDM_F16 || mm_dtype == STEDM_BF16, "widen16: bad mm_dtype");
  if (mm_dtype == STEDM_F16) widen16_kernel<_Float16><<<grid_for(n), 256, 0, as_stream(stream)>>>((const _Float16*)hi, (const _Float16*)lo, out, n);
  else widen16_kernel<__bf16><<<grid_for(n), 256, 0, as_stream(stream)>>>((const __bf16*)hi, (const __bf16*)lo, out, n);
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int stedm_svit_patch_gather(const float* img, int B, int ns, int H, int W, int patch, float* rows, void* stream) {
  STEDM_CHECK_ARG(img && rows && B > 0 && ns > 0 && patch > 0, "svit_patch_gather: bad args");
  STEDM_CHECK_ARG(H % patch == 0 && W % patch == 0, "svit_patch_gather: image not divisible by patch");
  const long total = (long)B * (H / patch) * (W / patch) * patch * patch * 3 * ns;
  svit_patch_gather_kernel<<<grid_for(total), 256, 0, as_stream(stream)>>>(img, rows, ns, H, W, patch, total);
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int stedm_svit_tok_bwd(const float* dx, float* d_pos, float* d_cls, float* d_tok, int B, int ntok, int dim, int accumulate, void* stream) {
  STEDM_CHECK_ARG(dx && d_pos && d_cls && d_tok && B > 0 && ntok > 0 && dim > 0, "svit_tok_bwd: bad args");
  svit_tok_bwd_kernel<<<grid_for((long)(ntok + 2) * dim), 256, 0, as_stream(stream)>>>(dx, d_pos, d_cls, d_tok, B, ntok, dim, accumulate);
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" long stedm_svit_head_bwd_ws_floats(int B, int dim) { return 4L * B * dim; }

extern "C" int stedm_svit_head_bwd(const float* x, int B, int T, int dim, int pool, const float* ln_w, const float* ln_b, float eps, const float* w,
                                   const float* d_out, int ncls, float* dx, float* d_ln_w, float* d_ln_b, float* d_w, float* d_bias, int accumulate,
                                   float* ws, void* stream) {
  STEDM_CHECK_ARG(x && ln_w && ln_b && w && d_out && dx && d_ln_w && d_ln_b && d_w && d_bias && ws, "svit_head_bwd: null pointer");
  STEDM_CHECK_ARG(pool == 0 || pool == 1, "svit_head_bwd: pool must be 0 (mean) or 1 (cls)");
  STEDM_CHECK_ARG(B > 0 && T > 0 && dim > 0 && ncls > 0 && (size_t)2 * dim * sizeof(float) <= 48 * 1024, "svit_head_bwd: bad sizes (dim=%d)", dim);
  hipStream_t st = as_stream(stream);
  svit_head_bwd_kernel<<<B, 256, (size_t)2 * dim * sizeof(float), st>>>(x, T, dim, pool, ln_w, ln_b, eps, w, d_out, ncls, ws, B);
  STEDM_LAUNCH_CHECK();
  svit_head_bwd_fold_kernel<<<grid_for((long)ncls * dim + 2 * dim + ncls), 256, 0, st>>>(ws, d_out, B, dim, ncls, d_ln_w, d_ln_b, d_w, d_bias, accumulate);
  STEDM_LAUNCH_CHECK();
  const long total = (long)B * T * dim;
  svit_pool_bwd_kernel<<<grid_for(total), 256, 0, st>>>(ws + 3L * B * dim, dx, T, dim, pool, total);
  STEDM_LAUNCH_CHECK();
  return 0;
}
