// The end of the training step: the gradient arena's norm and clip coefficient (torch.nn.utils.clip_grad_norm_), AdamW (torch.optim.AdamW)
// with LitEma (ema.py:25-44) over a pointer table in one launch, the same pass for convolution weights that also writes their 16-bit
// fragment-order packs (layouts: wfrag.hpp), and the EMA update alone. HBM-bound fp32 work; the step-dependent scalars come from the host
// or, in a captured step, from a device schedule. No atomics: every reduction has a fixed order.
#include "common.hpp"
#include "wfrag.hpp"

using namespace stedm;

namespace {

// ------------------------------------------------------------------------------------------------ gradient norm
// total_norm = grad_scale * sqrt(sum g^2) over the flat gradient arena and the coefficient of torch.nn.utils.clip_grad_norm_ (stedm_grad_norm).
// Two stages like the losses above: block b owns float4 b * 1024 + lane, + gridDim.x * 1024, ... of the 16-byte aligned body (a fixed
// assignment: no atomics, the same bits every run), block 0 also the at most 3 floats before the first aligned address and the at most 3
// after the last whole float4; squares and sums in fp64 (the square of an fp32 is exact there).
constexpr int GNORM_THREADS = 1024;
constexpr int GNORM_BLOCK_ELEMS = GNORM_THREADS * 4 * 4;      // elements of a block per round of its unrolled stride loop
constexpr int GNORM_MAX_BLOCKS = 512;                         // 2 per CU = 32 waves; few partials: the final launch adds them serially (4 KiB of LDS)
constexpr int GNORM_FINAL_THREADS = 256;
static int gnorm_blocks(long n) {
  const long b = (n + GNORM_BLOCK_ELEMS - 1) / GNORM_BLOCK_ELEMS;
  return (int)(b > GNORM_MAX_BLOCKS ? GNORM_MAX_BLOCKS : b);
}
__device__ __forceinline__ double gnorm_sq4(double s, const float4 a) {
  s = fma((double)a.x, (double)a.x, s); s = fma((double)a.y, (double)a.y, s);
  s = fma((double)a.z, (double)a.z, s); return fma((double)a.w, (double)a.w, s);
}
__global__ void __launch_bounds__(GNORM_THREADS) grad_norm_partial_kernel(const float* __restrict__ g, long n, double* __restrict__ part) {
  __shared__ double red[GNORM_THREADS];
  long head = (long)(((16 - (reinterpret_cast<uintptr_t>(g) & 15)) & 15) >> 2);      // floats before the first 16-byte boundary
  if (head > n) head = n;
  const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g + head);
  const long n4 = (n - head) >> 2;
  const long stride = (long)gridDim.x * GNORM_THREADS;
  long i = (long)blockIdx.x * GNORM_THREADS + threadIdx.x;
  double s = 0.0;
  for (; i + 3 * stride < n4; i += 4 * stride) {           // four independent 16-byte loads in flight per lane
    const float4 a = g4[i], b = g4[i + stride], c = g4[i + 2 * stride], d = g4[i + 3 * stride];
    s = gnorm_sq4(gnorm_sq4(gnorm_sq4(gnorm_sq4(s, a), b), c), d);
  }
  for (; i < n4; i += stride) s = gnorm_sq4(s, g4[i]);
  if (blockIdx.x == 0) {                                    // the unaligned start and the ragged tail: at most 3 floats each
    const long tail0 = head + 4 * n4;
    if ((long)threadIdx.x < head) { const double x = (double)g[threadIdx.x]; s = fma(x, x, s); }
    if (tail0 + threadIdx.x < n) { const double x = (double)g[tail0 + threadIdx.x]; s = fma(x, x, s); }
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = GNORM_THREADS / 2; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}
// One block: the partials in index order, then out = {total_norm, clip_coef, flag of a non-finite sum or norm}. clip_coef = min(max_norm / (total_norm + 1e-6), 1)
// in fp32 as torch forms it, written so that a NaN quotient stays NaN (fminf would return 1); max_norm <= 0: norm reporting only, coefficient 1.
__global__ void __launch_bounds__(GNORM_FINAL_THREADS) grad_norm_final_kernel(const double* __restrict__ part, int nb, float grad_scale, float max_norm,
                                                                        float* __restrict__ out) {
  __shared__ double sh[GNORM_MAX_BLOCKS];
  for (int i = threadIdx.x; i < nb; i += GNORM_FINAL_THREADS) sh[i] = part[i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int i = 0; i < nb; ++i) s += sh[i];
  const float norm = (float)((double)grad_scale * sqrt(s));
  float coef = 1.0f;
  if (max_norm > 0.f) {
    const float c = __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f));
    coef = c >= 1.0f ? 1.0f : c;
  }
  out[0] = norm;
  out[1] = coef;
  out[2] = isfinite(s) && isfinite(norm) ? 0.f : 1.f;      // (a finite sum can still overflow the fp32 norm: coefficient 0 then, flagged too)
}

// ------------------------------------------------------------------------------------------------ optimizer
// AdamW (torch.optim.AdamW semantics) + LitEma (ema.py:25-44) over many tensors in one launch. table[t] = {p, g, m, v, ema, n};
// chunk_tensor[blockIdx.x] / chunk_off[blockIdx.x] map a block to 4096 elements of one tensor.
struct OptTensor { float* p; const float* g; float* m; float* v; float* ema; long n; };
// one element of torch.optim.AdamW (decoupled weight decay first, bias corrections bc1 = 1 - beta1^t, bc2_sqrt = sqrt(1 - beta2^t))
__device__ __forceinline__ void adamw_one(float& p, float g_raw, float& m, float& v, float lr, float beta1, float beta2, float eps, float wd, float bc1,
                                          float bc2_sqrt, float grad_scale) {
  const float g = g_raw * grad_scale;
  float pn = p * (1.0f - lr * wd);
  m = beta1 * m + (1.0f - beta1) * g;
  v = beta2 * v + (1.0f - beta2) * g * g;
  const float denom = sqrtf(v) / bc2_sqrt + eps;
  pn -= (lr / bc1) * (m / denom);
  p = pn;
}
__global__ void __launch_bounds__(256) adamw_ema_kernel(const OptTensor* __restrict__ table, const int* __restrict__ chunk_tensor,
                                                        const long* __restrict__ chunk_off, float lr, float beta1, float beta2, float eps, float wd, float bc1,
                                                        float bc2_sqrt, float ema_decay, float grad_scale, const float* __restrict__ sched,
                                                        const int* __restrict__ sched_idx, const float* __restrict__ clip_coef) {
  if (clip_coef) grad_scale = __fmul_rn(grad_scale, *clip_coef);      // stedm_grad_norm's coefficient, read once per block; 1.0f leaves the scale's bits
  if (sched) {      // graph replay: this step's row of the host-built schedule {bc1, sqrt(bc2), ema_decay, lr} (stedm_adamw_ema_sched)
    const float* r = sched + 4 * (long)*sched_idx;
    bc1 = r[0]; bc2_sqrt = r[1]; ema_decay = r[2]; lr = r[3];
  }
  const OptTensor t = table[chunk_tensor[blockIdx.x]];
  const long o0 = chunk_off[blockIdx.x];
  const uintptr_t al = reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(t.g) | reinterpret_cast<uintptr_t>(t.m) |
                       reinterpret_cast<uintptr_t>(t.v) | reinterpret_cast<uintptr_t>(t.ema);
  if (o0 + 4096 <= t.n && (al & 15) == 0) {      // a whole chunk of 16-B aligned streams: 16 B per lane and access
    const bool has_e = t.ema != nullptr;
#pragma unroll 2
    for (int k = 0; k < 4; ++k) {
      const long i = o0 + (k * 256 + threadIdx.x) * 4;
      const float4 p4 = *reinterpret_cast<const float4*>(t.p + i), g4 = *reinterpret_cast<const float4*>(t.g + i);
      const float4 m4 = *reinterpret_cast<const float4*>(t.m + i), v4 = *reinterpret_cast<const float4*>(t.v + i);
      float4 e4 = make_float4(0.f, 0.f, 0.f, 0.f);
      if (has_e) e4 = *reinterpret_cast<const float4*>(t.ema + i);
      float pv[4] = {p4.x, p4.y, p4.z, p4.w}, mv[4] = {m4.x, m4.y, m4.z, m4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w};
      const float gv[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) adamw_one(pv[j], gv[j], mv[j], vv[j], lr, beta1, beta2, eps, wd, bc1, bc2_sqrt, grad_scale);
      *reinterpret_cast<float4*>(t.p + i) = make_float4(pv[0], pv[1], pv[2], pv[3]);
      *reinterpret_cast<float4*>(t.m + i) = make_float4(mv[0], mv[1], mv[2], mv[3]);
      *reinterpret_cast<float4*>(t.v + i) = make_float4(vv[0], vv[1], vv[2], vv[3]);
      if (has_e) {
        float ev[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) ev[j] = ev[j] - (1.0f - ema_decay) * (ev[j] - pv[j]);
        *reinterpret_cast<float4*>(t.ema + i) = make_float4(ev[0], ev[1], ev[2], ev[3]);
      }
    }
    return;
  }
  for (int k = 0; k < 16; ++k) {
    const long i = o0 + k * 256 + threadIdx.x;
    if (i >= t.n) return;
    float p = t.p[i], m = t.m[i], v = t.v[i];
    adamw_one(p, t.g[i], m, v, lr, beta1, beta2, eps, wd, bc1, bc2_sqrt, grad_scale);
    t.p[i] = p; t.m[i] = m; t.v[i] = v;
    if (t.ema) { const float s = t.ema[i]; t.ema[i] = s - (1.0f - ema_decay) * (s - p); }
  }
}

// AdamW + EMA for convolution weights that ALSO writes the 16-bit fragment-order copies the next forward / backward read (the packs of
// stedm_pack_frag_multi: forward order and the flipped / transposed dgrad order, 32x32x16 and 16x16x32 fragment forms), so the optimizer's own
// pass over the weights replaces the re-pack launches and their extra read. A block owns a 32 (cout) x 32 (cin) x taps piece of an OIHW
// filter: rows of 32 * taps contiguous floats in, the updated values kept in LDS, and every fragment vector (8 consecutive channels of one
// row and tap) that lies inside the piece written from there — a piece holds whole fragments of all four forms.
struct FusedPackOut { void* out; int transposed, flip, m16, f16; };
struct FusedOptDesc {
  float* p; const float* g; float* m; float* v; float* ema;
  int cout, cin, taps, blk0, nout, pad_;
  FusedPackOut o[4];
};
static_assert(sizeof(FusedPackOut) == 24 && sizeof(FusedOptDesc) == 160, "FusedOptDesc layout is part of the ABI (stedm_adamw_ema_pack)");

template <int ROWS, int CIW>
__global__ void __launch_bounds__(256) adamw_ema_pack_kernel(const FusedOptDesc* __restrict__ descs, const int nd, float lr, float beta1, float beta2,
                                                             float eps, float wd, float bc1, float bc2_sqrt, float ema_decay, float grad_scale,
                                                             const float* __restrict__ sched, const int* __restrict__ sched_idx,
                                                             const float* __restrict__ clip_coef) {
  extern __shared__ float ftile[];        // [ROWS][CIW * taps + 1]
  if (clip_coef) grad_scale = __fmul_rn(grad_scale, *clip_coef);
  if (sched) {
    const float* r = sched + 4 * (long)*sched_idx;
    bc1 = r[0]; bc2_sqrt = r[1]; ema_decay = r[2]; lr = r[3];
  }
  int lo = 0, hi = nd - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].blk0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const FusedOptDesc& d = descs[lo];
  const int bid = blockIdx.x - d.blk0;
  const int taps = d.taps, cin = d.cin, cout = d.cout;
  const int ncb = cin / CIW;
  const int co0 = (bid / ncb) * ROWS, ci0 = (bid % ncb) * CIW;
  const int run = CIW * taps, pitch = run + 1, r4 = run >> 2;
  float* const P = d.p; const float* const G = d.g; float* const M = d.m; float* const V = d.v; float* const E = d.ema;
  const bool has_e = E != nullptr;
#pragma unroll 2
  for (int idx = threadIdx.x; idx < ROWS * r4; idx += 256) {
    const int row = idx / r4, r0 = (idx - row * r4) * 4;
    const long off = ((long)(co0 + row) * cin + ci0) * taps + r0;
    const float4 p4 = *reinterpret_cast<const float4*>(P + off), g4 = *reinterpret_cast<const float4*>(G + off);
    const float4 m4 = *reinterpret_cast<const float4*>(M + off), v4 = *reinterpret_cast<const float4*>(V + off);
    float4 e4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (has_e) e4 = *reinterpret_cast<const float4*>(E + off);
    float pv[4] = {p4.x, p4.y, p4.z, p4.w}, mv[4] = {m4.x, m4.y, m4.z, m4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w};
    const float gv[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) adamw_one(pv[j], gv[j], mv[j], vv[j], lr, beta1, beta2, eps, wd, bc1, bc2_sqrt, grad_scale);
    *reinterpret_cast<float4*>(P + off) = make_float4(pv[0], pv[1], pv[2], pv[3]);
    *reinterpret_cast<float4*>(M + off) = make_float4(mv[0], mv[1], mv[2], mv[3]);
    *reinterpret_cast<float4*>(V + off) = make_float4(vv[0], vv[1], vv[2], vv[3]);
    if (has_e) {
      float ev[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) ev[j] = ev[j] - (1.0f - ema_decay) * (ev[j] - pv[j]);
      *reinterpret_cast<float4*>(E + off) = make_float4(ev[0], ev[1], ev[2], ev[3]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) ftile[row * pitch + r0 + j] = pv[j];
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int oi = 0; oi < d.nout; ++oi) {
    const FusedPackOut po = d.o[oi];
    const int fr = po.m16 ? FragM16::FR : FragM32::FR, fc = po.m16 ? FragM16::KC : FragM32::KC;      // fragment rows x channels (wfrag.hpp)
    const int Rn = po.transposed ? CIW : ROWS, Rc = po.transposed ? ROWS : CIW;   // the piece in the pack's (row n, channel c) coordinates
    const int n_base = po.transposed ? ci0 : co0, c_base = po.transposed ? co0 : ci0;
    const int nch = (po.transposed ? cout : cin) / fc;                       // channel chunks of the pack
    const int nfn = Rn / fr, nfrag = nfn * (Rc / fc) * taps;
    for (int f = wave; f < nfrag; f += 4) {
      const int tap = f % taps, ff = f / taps, fn = ff % nfn, fcx = ff / nfn;
      const int nl = fn * fr + (po.m16 ? FragM16::lane_row(lane) : FragM32::lane_row(lane));
      const int cl = fcx * fc + (po.m16 ? FragM16::lane_c(lane, taps) : FragM32::lane_c(lane, taps));
      const int ts = po.flip ? taps - 1 - tap : tap;        // source tap
      const float* src = po.transposed ? ftile + cl * pitch + nl * taps + ts : ftile + nl * pitch + cl * taps + ts;
      const int es = po.transposed ? pitch : taps;
      float x[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = src[e * es];
      const int n = n_base + nl, c = c_base + cl;
      const long at = po.m16 ? frag_at<FragM16>(n, c, tap, nch, taps) : frag_at<FragM32>(n, c, tap, nch, taps);
      if (po.f16) {
        typedef _Float16 H8 __attribute__((ext_vector_type(8)));
        H8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (_Float16)x[e];
        *reinterpret_cast<H8*>(reinterpret_cast<_Float16*>(po.out) + at) = o;
      } else {
        typedef __bf16 B8 __attribute__((ext_vector_type(8)));
        B8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (__bf16)x[e];
        *reinterpret_cast<B8*>(reinterpret_cast<__bf16*>(po.out) + at) = o;
      }
    }
  }
}


// LitEma.forward alone (ema.py:25-44, called from on_train_batch_end, ddpm.py:369-371): shadow -= (1 - decay) * (shadow - p) over the
// optimizer's pointer table; tensors without a shadow are skipped.
__global__ void __launch_bounds__(256) ema_update_kernel(const OptTensor* __restrict__ table, const int* __restrict__ chunk_tensor,
                                                         const long* __restrict__ chunk_off, float one_minus_decay) {
  const OptTensor t = table[chunk_tensor[blockIdx.x]];
  if (!t.ema) return;
  const long o0 = chunk_off[blockIdx.x];
  for (int k = 0; k < 16; ++k) {
    const long i = o0 + k * 256 + threadIdx.x;
    if (i >= t.n) return;
    const float s = t.ema[i];
    t.ema[i] = s - one_minus_decay * (s - t.p[i]);
  }
}

}  // namespace

// The gradient arena's norm and clip coefficient (see grad_norm_partial_kernel): ws = stedm_grad_norm_blocks(n) doubles, out = 3 floats on the device.
extern "C" int stedm_grad_norm_blocks(long n) { return n > 0 ? gnorm_blocks(n) : 0; }

extern "C" int stedm_grad_norm(const float* g, long n, float grad_scale, float max_norm, double* ws, float* out, void* stream) {
  STEDM_CHECK_ARG(g && ws && out && n > 0 && (reinterpret_cast<uintptr_t>(g) & 3) == 0, "grad_norm: bad args");
  const int nb = gnorm_blocks(n);
  grad_norm_partial_kernel<<<nb, GNORM_THREADS, 0, as_stream(stream)>>>(g, n, ws);
  grad_norm_final_kernel<<<1, GNORM_FINAL_THREADS, 0, as_stream(stream)>>>(ws, nb, grad_scale, max_norm, out);
  STEDM_LAUNCH_CHECK();
  return 0;
}

// The four optimizer entry points exist in two forms: *_clip takes clip_coef, a DEVICE float (out[1] of stedm_grad_norm) that multiplies grad_scale
// inside the kernel, so a clipped step needs no host read; the plain forms pass NULL and keep their bits.
extern "C" int stedm_adamw_ema_clip(const void* table, const int* chunk_tensor, const long* chunk_off, int nchunks, float lr, float beta1, float beta2,
                                    float eps, float weight_decay, int step, float ema_decay, float grad_scale, const float* clip_coef, void* stream) {
  STEDM_CHECK_ARG(table && chunk_tensor && chunk_off && nchunks > 0 && step >= 1, "adamw_ema: bad args");
  const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
  const float bc2 = (float)(1.0 - pow((double)beta2, (double)step));
  adamw_ema_kernel<<<nchunks, 256, 0, as_stream(stream)>>>((const OptTensor*)table, chunk_tensor, chunk_off, lr, beta1, beta2, eps, weight_decay, bc1, sqrtf(bc2),
                                                          ema_decay, grad_scale, nullptr, nullptr, clip_coef);
  STEDM_LAUNCH_CHECK();
  return 0;
}
extern "C" int stedm_adamw_ema(const void* table, const int* chunk_tensor, const long* chunk_off, int nchunks, float lr, float beta1, float beta2, float eps,
                               float weight_decay, int step, float ema_decay, float grad_scale, void* stream) {
  return stedm_adamw_ema_clip(table, chunk_tensor, chunk_off, nchunks, lr, beta1, beta2, eps, weight_decay, step, ema_decay, grad_scale, nullptr, stream);
}

// The two optimizer passes with the step-dependent scalars read on the device: sched [n][4] = {1 - beta1^s, sqrt(1 - beta2^s), ema decay of step s,
// learning rate of step s} built by the host for a window of steps, *sched_idx = the row of the step being replayed (advanced by stedm_step_advance
// inside the captured step). A captured training step (UNetTrainer.capture_step) replays with nothing but that index changing.
extern "C" int stedm_adamw_ema_sched_clip(const void* table, const int* chunk_tensor, const long* chunk_off, int nchunks, float beta1, float beta2, float eps,
                                          float weight_decay, const float* sched, const int* sched_idx, float grad_scale, const float* clip_coef,
                                          void* stream) {
  STEDM_CHECK_ARG(table && chunk_tensor && chunk_off && nchunks > 0 && sched && sched_idx, "adamw_ema_sched: bad args");
  adamw_ema_kernel<<<nchunks, 256, 0, as_stream(stream)>>>((const OptTensor*)table, chunk_tensor, chunk_off, 0.f, beta1, beta2, eps, weight_decay, 1.f, 1.f, 0.f,
                                                          grad_scale, sched, sched_idx, clip_coef);
  STEDM_LAUNCH_CHECK();
  return 0;
}
extern "C" int stedm_adamw_ema_sched(const void* table, const int* chunk_tensor, const long* chunk_off, int nchunks, float beta1, float beta2, float eps,
                                     float weight_decay, const float* sched, const int* sched_idx, float grad_scale, void* stream) {
  return stedm_adamw_ema_sched_clip(table, chunk_tensor, chunk_off, nchunks, beta1, beta2, eps, weight_decay, sched, sched_idx, grad_scale, nullptr, stream);
}

// piece geometry of stedm_adamw_ema_pack: a tensor takes (cout / rows) * (cin / ciw) blocks. 32 x 32, 64 x 32, 32 x 64 and 64 x 64 measured the
// same on the north-star U-Net: the pass is bound by its 40 bytes per weight (234.6 M weights in 1.72 ms = 5.4 TB/s; the plain kernel moves
// its 36 bytes per weight at 5.5 TB/s), not by the segment length (tools/bench_opt.py)
constexpr int kOptRows = 32, kOptCiw = 32;
extern "C" int stedm_adamw_ema_pack_piece(int* rows, int* ciw) {
  STEDM_CHECK_ARG(rows && ciw, "adamw_ema_pack_piece: null pointer");
  *rows = kOptRows; *ciw = kOptCiw;
  return 0;
}

extern "C" int stedm_adamw_ema_pack_clip(const void* descs, int ndesc, int total_blocks, float lr, float beta1, float beta2, float eps, float weight_decay,
                                         int step, float ema_decay, float grad_scale, const float* clip_coef, void* stream) {
  STEDM_CHECK_ARG(descs && ndesc > 0 && total_blocks > 0 && step >= 1, "adamw_ema_pack: bad args");
  const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
  const float bc2 = (float)(1.0 - pow((double)beta2, (double)step));
  const size_t lds = (size_t)kOptRows * (kOptCiw * 9 + 1) * sizeof(float);
  adamw_ema_pack_kernel<kOptRows, kOptCiw><<<total_blocks, 256, lds, as_stream(stream)>>>((const FusedOptDesc*)descs, ndesc, lr, beta1, beta2, eps, weight_decay,
                                                                                          bc1, sqrtf(bc2), ema_decay, grad_scale, nullptr, nullptr, clip_coef);
  STEDM_LAUNCH_CHECK();
  return 0;
}
extern "C" int stedm_adamw_ema_pack(const void* descs, int ndesc, int total_blocks, float lr, float beta1, float beta2, float eps, float weight_decay,
                                    int step, float ema_decay, float grad_scale, void* stream) {
  return stedm_adamw_ema_pack_clip(descs, ndesc, total_blocks, lr, beta1, beta2, eps, weight_decay, step, ema_decay, grad_scale, nullptr, stream);
}

extern "C" int stedm_adamw_ema_pack_sched_clip(const void* descs, int ndesc, int total_blocks, float beta1, float beta2, float eps, float weight_decay,
                                               const float* sched, const int* sched_idx, float grad_scale, const float* clip_coef, void* stream) {
  STEDM_CHECK_ARG(descs && ndesc > 0 && total_blocks > 0 && sched && sched_idx, "adamw_ema_pack_sched: bad args");
  const size_t lds = (size_t)kOptRows * (kOptCiw * 9 + 1) * sizeof(float);
  adamw_ema_pack_kernel<kOptRows, kOptCiw><<<total_blocks, 256, lds, as_stream(stream)>>>((const FusedOptDesc*)descs, ndesc, 0.f, beta1, beta2, eps, weight_decay,
                                                                                          1.f, 1.f, 0.f, grad_scale, sched, sched_idx, clip_coef);
  STEDM_LAUNCH_CHECK();
  return 0;
}
extern "C" int stedm_adamw_ema_pack_sched(const void* descs, int ndesc, int total_blocks, float beta1, float beta2, float eps, float weight_decay,
                                          const float* sched, const int* sched_idx, float grad_scale, void* stream) {
  return stedm_adamw_ema_pack_sched_clip(descs, ndesc, total_blocks, beta1, beta2, eps, weight_decay, sched, sched_idx, grad_scale, nullptr, stream);
}

extern "C" int stedm_ema_update(const void* table, const int* chunk_tensor, const long* chunk_off, int nchunks, float ema_decay, void* stream) {
  STEDM_CHECK_ARG(table && chunk_tensor && chunk_off && nchunks > 0 && ema_decay >= 0.f && ema_decay <= 1.f, "ema_update: bad args");
  ema_update_kernel<<<nchunks, 256, 0, as_stream(stream)>>>((const OptTensor*)table, chunk_tensor, chunk_off, 1.0f - ema_decay);
  STEDM_LAUNCH_CHECK();
  return 0;
}
