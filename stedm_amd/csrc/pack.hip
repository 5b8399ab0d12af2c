// Weight packing: fp32 filters -> the 16-bit copies the convolution kernels read ([cout][tap][cin] planes, MFMA fragment orders, the
// sub-pixel and space-to-depth derived filters), and the space-to-depth activation planes. The layouts are stated in wfrag.hpp.
#include "common.hpp"
#include "wfrag.hpp"

using namespace stedm;

static int grid_for(long total, int cap) { return (int)((total + 255) / 256 < cap ? (total + 255) / 256 : cap); }

// ------------------------------------------------------------------------------------------------
// Planes: OIHW fp32 -> [cout][tap][cin] 16-bit hi (+ lo = round(w - float(hi))).
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void pack_conv_weight_kernel(const float* __restrict__ w, T* __restrict__ hi, T* __restrict__ lo, int cout,
                                        int cin, int taps, long sn, long sc, int flip) {
  const long total = (long)cout * taps * cin;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ci = (int)(i % cin);
    const long r = i / cin;
    const int tap = (int)(r % taps);
    const int co = (int)(r / taps);
    T h, l;
    round_hi_lo(w[(long)co * sn + (long)ci * sc + (flip ? taps - 1 - tap : tap)], h, l);
    hi[i] = h;
    if (lo) lo[i] = l;
  }
}

static void launch_pack_planes(const float* w, void* hi, void* lo, int cout, int cin, int taps, long sn, long sc, int flip, int mm_dtype, hipStream_t st) {
  const int grid = grid_for((long)cout * cin * taps, 4096);
  with_mm_dtype(mm_dtype, [&](auto t) {
    using T = decltype(t);
    pack_conv_weight_kernel<T><<<grid, 256, 0, st>>>(w, (T*)hi, (T*)lo, cout, cin, taps, sn, sc, flip);
  });
}

extern "C" int stedm_pack_conv_weight(const float* w, void* w_hi, void* w_lo, int cout, int cin, int ks, int mm_dtype,
                                      void* stream) {
  STEDM_CHECK_ARG(w && w_hi, "pack_conv_weight: null pointer");
  STEDM_CHECK_ARG(ks == 1 || ks == 3, "pack_conv_weight: ks must be 1 or 3 (got %d)", ks);
  STEDM_CHECK_ARG(mm_dtype == STEDM_F16 || mm_dtype == STEDM_BF16, "pack_conv_weight: bad mm_dtype %d", mm_dtype);
  launch_pack_planes(w, w_hi, w_lo, cout, cin, ks * ks, (long)cin * ks * ks, ks * ks, 0, mm_dtype, as_stream(stream));
  STEDM_LAUNCH_CHECK();
  return 0;
}

// Sub-pixel upsample planes [4 parities][cout][4 taps][cin]: the 3x3 taps that read the same low-res pixel, pre-summed (subpixel_weight)
template <typename T>
__global__ void pack_conv_weight_up_kernel(const float* __restrict__ w, T* __restrict__ hi, T* __restrict__ lo, int cout, int cin) {
  const long total = (long)4 * cout * 4 * cin;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ci = (int)(i % cin);
    long r = i / cin;
    const int tap = (int)(r % 4); r /= 4;
    const int co = (int)(r % cout);
    const int par = (int)(r / cout);
    T h, l;
    round_hi_lo(subpixel_weight(w, co, cin, ci, par, tap), h, l);
    hi[i] = h;
    if (lo) lo[i] = l;
  }
}

extern "C" int stedm_pack_conv_weight_up(const float* w, void* w_hi, void* w_lo, int cout, int cin, int mm_dtype, void* stream) {
  STEDM_CHECK_ARG(w && w_hi, "pack_conv_weight_up: null pointer");
  STEDM_CHECK_ARG(mm_dtype == STEDM_F16 || mm_dtype == STEDM_BF16, "pack_conv_weight_up: bad mm_dtype %d", mm_dtype);
  const int grid = grid_for((long)16 * cout * cin, 4096);
  with_mm_dtype(mm_dtype, [&](auto t) {
    using T = decltype(t);
    pack_conv_weight_up_kernel<T><<<grid, 256, 0, as_stream(stream)>>>(w, (T*)w_hi, (T*)w_lo, cout, cin);
  });
  STEDM_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Fragment orders (FragM32 / FragM16, wfrag.hpp) of a 3x3 / 1x1 filter from an arbitrarily strided source.
// ------------------------------------------------------------------------------------------------
// One block = 2 Frag::FR rows x Frag::KC channels x taps of one 128-row tile (two fragments per tap): the source values go through LDS so
// that both the gather from the source (runs along its contiguous index: (ci, tap) for an OIHW filter, (n, tap) for the transposed forms)
// and the 16-B fragment stores are coalesced.
constexpr int kPackTileFloats = 64 * (16 * 9 + 1);     // the largest tile of the four (taps, Frag) forms: 64 rows x (16 x 9 + 1)

// block `bid` of one tensor's pack; `traw`: kPackTileFloats floats of LDS
template <typename T, int taps, typename Frag>
__device__ __forceinline__ void pack_frag_block(const float* __restrict__ w, T* __restrict__ out, const int cout, const int cin, const long sn,
                                                const long sc, const int flip, const int bid, float* traw, T* __restrict__ out_lo = nullptr) {
  typedef T V8 __attribute__((ext_vector_type(8)));
  constexpr int NR = 2 * Frag::FR, KC = Frag::KC, NSUB = 128 / NR;     // rows (two fragments) and channels per block, blocks per 128-row tile
  constexpr int PITCH = KC * taps + 1;
  static_assert(NR * PITCH <= kPackTileFloats, "pack tile");
  float (*tile)[PITCH] = reinterpret_cast<float (*)[PITCH]>(traw);
  const int nch = cin / KC;
  const int half = bid % NSUB;
  const int chunk = (bid / NSUB) % nch, tn = (bid / NSUB) / nch;
  const int n0 = tn * 128 + half * NR, ci0 = chunk * KC;
  const int per = NR * KC * taps;
  const bool n_fast = sn <= sc;       // which source index is contiguous
  // 16-B loads along the contiguous source run when the layout allows it (rows inside the matrix, 16-B aligned runs): the pack is a
  // pure stream, its speed is the bytes in flight
  const bool vec = n0 + NR <= cout && (n_fast ? (sn == taps && (sc * 4) % 16 == 0) : (sc == taps && (sn * 4) % 16 == 0)) &&
                   ((reinterpret_cast<uintptr_t>(w) & 15) == 0) && ((n_fast ? NR : KC) * taps) % 4 == 0;
  if (vec) {
    const int run = (n_fast ? NR : KC) * taps;          // contiguous floats per outer index (ci for n_fast, n otherwise)
    const int nouter = n_fast ? KC : NR;
    for (int v4 = threadIdx.x; v4 < nouter * (run / 4); v4 += 256) {
      const int o = v4 / (run / 4), r0 = (v4 - o * (run / 4)) * 4;
      const float* src = n_fast ? w + (long)n0 * sn + (long)(ci0 + o) * sc + r0 : w + (long)(n0 + o) * sn + (long)ci0 * sc + r0;
      const float4 f = *reinterpret_cast<const float4*>(src);
      const float fv[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = r0 + j, a = r / taps, ts = r - a * taps;       // a = n_local (n_fast) or ci_local; ts = source tap
        const int tap = flip ? taps - 1 - ts : ts;
        if (n_fast) tile[a][o * taps + tap] = fv[j];
        else tile[o][a * taps + tap] = fv[j];
      }
    }
  } else
  for (int idx = threadIdx.x; idx < per; idx += 256) {
    int row, cil, tap;
    if (n_fast) { cil = idx / (NR * taps); const int r = idx - cil * NR * taps; row = r / taps; tap = r - row * taps; }
    else { row = idx / (KC * taps); const int r = idx - row * KC * taps; cil = r / taps; tap = r - cil * taps; }
    const int n = n0 + row;
    tile[row][cil * taps + tap] = n < cout ? w[(long)n * sn + (long)(ci0 + cil) * sc + (flip ? taps - 1 - tap : tap)] : 0.f;
  }
  __syncthreads();
  // stores: (tap, fragment of the block, lane) -> one 16-B vector of 8 consecutive channels
  for (int v = threadIdx.x; v < taps * 2 * 64; v += 256) {
    const int lane = v & 63, ql = (v >> 6) & 1, tap = v >> 7;
    const int row = ql * Frag::FR + Frag::lane_row(lane), c8 = Frag::lane_c(lane, taps);
    V8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (T)tile[row][(c8 + e) * taps + tap];
    const long at = frag_at<Frag>(n0 + row, ci0 + c8, tap, nch, taps);
    *reinterpret_cast<V8*>(out + at) = o;
    if (out_lo) {     // 3-product mode: the second stream holds w - hi
      V8 l;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        T h, lo;
        round_hi_lo(tile[row][(c8 + e) * taps + tap], h, lo);
        l[e] = lo;
      }
      *reinterpret_cast<V8*>(out_lo + at) = l;
    }
  }
}

template <typename T, int taps, typename Frag>
__global__ void __launch_bounds__(256) pack_conv_weight_frag_kernel(const float* __restrict__ w, T* __restrict__ out, int cout, int cin, long sn, long sc,
                                                                    int flip, T* __restrict__ out_lo) {
  __shared__ float traw[kPackTileFloats];
  pack_frag_block<T, taps, Frag>(w, out, cout, cin, sn, sc, flip, blockIdx.x, traw, out_lo);
}

// hl: the hi stream is followed by the lo stream of the 3-product mode, out = [2][pack]
template <typename Frag>
static void launch_pack_frag(const float* w, void* out, int cout, int cin, int taps, long sn, long sc, int flip, bool hl, int mm_dtype, hipStream_t st) {
  const int grid = ((cout + 127) / 128) * (cin / Frag::KC) * (64 / Frag::FR);      // blocks of two fragments x taps
  const long total = (long)((cout + 127) / 128) * (cin / Frag::KC) * taps * Frag::NFRAG * 512;
  with_mm_dtype(mm_dtype, [&](auto t) {
    using T = decltype(t);
    T* const o = (T*)out;
    T* const lo = hl ? o + total : nullptr;
    if (taps == 9) pack_conv_weight_frag_kernel<T, 9, Frag><<<grid, 256, 0, st>>>(w, o, cout, cin, sn, sc, flip, lo);
    else pack_conv_weight_frag_kernel<T, 1, Frag><<<grid, 256, 0, st>>>(w, o, cout, cin, sn, sc, flip, lo);
  });
}

// Many tensors in ONE launch (the training step re-packs every convolution's weights after each optimizer step: ~130 packs of a few
// microseconds each were launch-bound). descs[i].blk0 = first block of tensor i (ascending); a block finds its tensor by binary search.
struct PackDesc {
  const float* w;
  void* out;
  long sn, sc;
  int cout, cin, taps, flip, m16, blk0;
};
static_assert(sizeof(PackDesc) == 56, "PackDesc layout is part of the ABI (stedm_pack_frag_multi)");

template <typename T>
__global__ void __launch_bounds__(256) pack_frag_multi_kernel(const PackDesc* __restrict__ descs, const int nd) {
  __shared__ float traw[kPackTileFloats];
  int lo = 0, hi = nd - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].blk0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const PackDesc d = descs[lo];
  const int bid = blockIdx.x - d.blk0;
  T* out = reinterpret_cast<T*>(d.out);
  if (d.m16) {
    if (d.taps == 9) pack_frag_block<T, 9, FragM16>(d.w, out, d.cout, d.cin, d.sn, d.sc, d.flip, bid, traw);
    else pack_frag_block<T, 1, FragM16>(d.w, out, d.cout, d.cin, d.sn, d.sc, d.flip, bid, traw);
  } else {
    if (d.taps == 9) pack_frag_block<T, 9, FragM32>(d.w, out, d.cout, d.cin, d.sn, d.sc, d.flip, bid, traw);
    else pack_frag_block<T, 1, FragM32>(d.w, out, d.cout, d.cin, d.sn, d.sc, d.flip, bid, traw);
  }
}

extern "C" int stedm_pack_frag_multi(const void* descs, int nd, int total_blocks, int mm_dtype, void* stream) {
  STEDM_CHECK_ARG(descs && nd > 0 && total_blocks > 0, "pack_frag_multi: bad args");
  STEDM_CHECK_ARG(mm_dtype == STEDM_F16 || mm_dtype == STEDM_BF16, "pack_frag_multi: bad mm_dtype %d", mm_dtype);
  with_mm_dtype(mm_dtype, [&](auto t) {
    pack_frag_multi_kernel<decltype(t)><<<total_blocks, 256, 0, as_stream(stream)>>>(reinterpret_cast<const PackDesc*>(descs), nd);
  });
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int stedm_pack_conv_weight_frag(const float* w, void* out, int cout, int cin, int ks, int mm_dtype, void* stream) {
  STEDM_CHECK_ARG(w && out && cin % 16 == 0 && (ks == 1 || ks == 3), "pack_conv_weight_frag: bad args (cin %% 16, ks 1 or 3)");
  STEDM_CHECK_ARG(mm_dtype == STEDM_F16 || mm_dtype == STEDM_BF16, "pack_conv_weight_frag: bad mm_dtype %d", mm_dtype);
  launch_pack_frag<FragM32>(w, out, cout, cin, ks * ks, (long)cin * ks * ks, ks * ks, 0, false, mm_dtype, as_stream(stream));
  STEDM_LAUNCH_CHECK();
  return 0;
}

// Same packs from an arbitrarily strided source: element (n, ci, tap) = w[n*sn + ci*sc + (flip ? taps-1-tap : tap)]. The backward pass
// packs the dgrad filter (n = forward cin, ci = forward cout, taps reversed) straight from the OIHW parameter, and dY^T of the
// wgrad GEMM (n = channel, ci = pixel) straight from the NHWC gradient. Any of w_hi / w_lo / w_frag may be NULL.
extern "C" int stedm_pack_conv_weight_strided(const float* w, long sn, long sc, int flip, void* w_hi, void* w_lo, void* w_frag, int cout, int cin, int ks,
                                              int mm_dtype, void* stream) {
  STEDM_CHECK_ARG(w && (w_hi || w_frag) && (ks == 1 || ks == 3), "pack_conv_weight_strided: bad args");
  STEDM_CHECK_ARG(!w_frag || cin % 16 == 0, "pack_conv_weight_strided: fragment order needs cin %% 16 == 0");
  STEDM_CHECK_ARG(mm_dtype == STEDM_F16 || mm_dtype == STEDM_BF16, "pack_conv_weight_strided: bad mm_dtype %d", mm_dtype);
  if (w_hi) launch_pack_planes(w, w_hi, w_lo, cout, cin, ks * ks, sn, sc, flip, mm_dtype, as_stream(stream));
  if (w_frag) launch_pack_frag<FragM32>(w, w_frag, cout, cin, ks * ks, sn, sc, flip, false, mm_dtype, as_stream(stream));
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int stedm_pack_conv_weight_frag16(const float* w, long sn, long sc, int flip, void* out, int cout, int cin, int ks, int mm_dtype, void* stream) {
  STEDM_CHECK_ARG(w && out && cin % 32 == 0 && cout > 0 && (ks == 1 || ks == 3), "pack_conv_weight_frag16: bad args (cin %% 32, ks 1 or 3)");
  STEDM_CHECK_ARG(mm_dtype == STEDM_F16 || mm_dtype == STEDM_BF16, "pack_conv_weight_frag16: bad mm_dtype %d", mm_dtype);
  launch_pack_frag<FragM16>(w, out, cout, cin, ks * ks, sn, sc, flip, false, mm_dtype, as_stream(stream));
  STEDM_LAUNCH_CHECK();
  return 0;
}

// hi and lo fragment streams of the 3-product mode: out = [2][total] elements, total = ceil(cout / 128) * (cin / 32) * 9 * 8 * 512
extern "C" int stedm_pack_conv_weight_frag16_hl(const float* w, long sn, long sc, int flip, void* out, int cout, int cin, int mm_dtype, void* stream) {
  STEDM_CHECK_ARG(w && out && cin % 32 == 0 && cout > 0, "pack_conv_weight_frag16_hl: bad args (cin %% 32)");
  STEDM_CHECK_ARG(mm_dtype == STEDM_F16 || mm_dtype == STEDM_BF16, "pack_conv_weight_frag16_hl: bad mm_dtype %d", mm_dtype);
  launch_pack_frag<FragM16>(w, out, cout, cin, 9, sn, sc, flip, true, mm_dtype, as_stream(stream));
  STEDM_LAUNCH_CHECK();
  return 0;
}

// ... of a 1x1 filter (skip_connection, qkv, proj_out in the 3-product modes): out = [2][ceil(cout / 128)][cin / 32][1][8][512]
extern "C" int stedm_pack_conv_weight_frag16_hl1(const float* w, long sn, long sc, int flip, void* out, int cout, int cin, int mm_dtype, void* stream) {
  STEDM_CHECK_ARG(w && out && cin % 32 == 0 && cout > 0, "pack_conv_weight_frag16_hl1: bad args (cin %% 32)");
  STEDM_CHECK_ARG(mm_dtype == STEDM_F16 || mm_dtype == STEDM_BF16, "pack_conv_weight_frag16_hl1: bad mm_dtype %d", mm_dtype);
  launch_pack_frag<FragM16>(w, out, cout, cin, 1, sn, sc, flip, true, mm_dtype, as_stream(stream));
  STEDM_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Derived 2x2 filters of an OIHW 3x3, in fragment order (4 taps), one element per thread step.
// ------------------------------------------------------------------------------------------------
// UP: the four parity filters of the sub-pixel upsample, out = [4 parities][pack over cin channels]; else the space-to-depth Downsample
// filter (STEDM_CONV_S2D), out = [pack over 4 * cin channels], channel = parity block * cin + c. HL: followed by the lo stream (value - hi,
// rounded) of the 3-product modes (conv_rs.inc RS_SUBM).
template <typename T, typename Frag, bool UP, bool HL>
__global__ void pack_derived_frag_kernel(const float* __restrict__ w, T* __restrict__ out, int cout, int cin, long per_parity, long total, int pad_br) {
  const int nch = (UP ? cin : 4 * cin) / Frag::KC;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int par = UP ? (int)(i / per_parity) : 0;
    const FragCoord k = frag_coord<Frag>(i - par * per_parity, nch, 4);
    float v = 0.f;
    if (UP) {
      if (k.n < cout) v = subpixel_weight(w, k.n, cin, k.ci, par, k.tap);
    } else {
      const int pb = k.ci / cin, c = k.ci - pb * cin;          // parity block of the space-to-depth planes, channel inside it
      const Tap2 t = s2d_tap(pb, k.tap, pad_br);
      if (k.n < cout && t.dy >= 0 && t.dx >= 0) v = w[((long)k.n * cin + c) * 9 + t.dy * 3 + t.dx];
    }
    T h, l;
    round_hi_lo(v, h, l);
    out[i] = h;
    if (HL) out[total + i] = l;
  }
}

template <typename Frag, bool UP, bool HL>
static void launch_pack_derived(const float* w, void* out, int cout, int cin, int pad_br, int mm_dtype, hipStream_t st) {
  const long per = (long)((cout + 127) / 128) * ((UP ? cin : 4 * cin) / Frag::KC) * 4 * Frag::NFRAG * 512, total = UP ? 4 * per : per;
  const int grid = grid_for(total, 8192);
  with_mm_dtype(mm_dtype, [&](auto t) {
    using T = decltype(t);
    pack_derived_frag_kernel<T, Frag, UP, HL><<<grid, 256, 0, st>>>(w, (T*)out, cout, cin, per, total, pad_br);
  });
}

extern "C" int stedm_pack_conv_weight_up_frag(const float* w, void* out, int cout, int cin, int mm_dtype, void* stream) {
  STEDM_CHECK_ARG(w && out && cin % 32 == 0, "pack_conv_weight_up_frag: bad args (cin %% 32)");
  STEDM_CHECK_ARG(mm_dtype == STEDM_F16 || mm_dtype == STEDM_BF16, "pack_conv_weight_up_frag: bad mm_dtype %d", mm_dtype);
  launch_pack_derived<FragM32, true, false>(w, out, cout, cin, 0, mm_dtype, as_stream(stream));
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int stedm_pack_conv_weight_s2d_frag(const float* w, void* out, int cout, int cin, int mm_dtype, int pad_br, void* stream) {
  STEDM_CHECK_ARG(w && out && cin % 8 == 0, "pack_conv_weight_s2d_frag: bad args (cin %% 8)");
  STEDM_CHECK_ARG(mm_dtype == STEDM_F16 || mm_dtype == STEDM_BF16, "pack_conv_weight_s2d_frag: bad mm_dtype %d", mm_dtype);
  launch_pack_derived<FragM32, false, false>(w, out, cout, cin, pad_br, mm_dtype, as_stream(stream));
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int stedm_pack_conv_weight_up_frag16_hl(const float* w, void* out, int cout, int cin, int mm_dtype, void* stream) {
  STEDM_CHECK_ARG(w && out && cin % 32 == 0 && cout > 0, "pack_conv_weight_up_frag16_hl: bad args (cin %% 32)");
  STEDM_CHECK_ARG(mm_dtype == STEDM_F16 || mm_dtype == STEDM_BF16, "pack_conv_weight_up_frag16_hl: bad mm_dtype %d", mm_dtype);
  launch_pack_derived<FragM16, true, true>(w, out, cout, cin, 0, mm_dtype, as_stream(stream));
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int stedm_pack_conv_weight_s2d_frag16_hl(const float* w, void* out, int cout, int cin, int mm_dtype, int pad_br, void* stream) {
  STEDM_CHECK_ARG(w && out && cin % 8 == 0 && cout > 0, "pack_conv_weight_s2d_frag16_hl: bad args (cin %% 8)");
  STEDM_CHECK_ARG(mm_dtype == STEDM_F16 || mm_dtype == STEDM_BF16, "pack_conv_weight_s2d_frag16_hl: bad mm_dtype %d", mm_dtype);
  launch_pack_derived<FragM16, false, true>(w, out, cout, cin, pad_br, mm_dtype, as_stream(stream));
  STEDM_LAUNCH_CHECK();
  return 0;
}

// NHWC fp32 -> space-to-depth 16-bit planes [B][H/2][W/2][4C]; thread = one channel quad of one input pixel
template <typename T>
__global__ void __launch_bounds__(256) space_to_depth16_kernel(const float* __restrict__ x, T* __restrict__ hi, T* __restrict__ lo, int C, int H, int W,
                                                               long total_q, unsigned* ovf) {
  typedef T V4 __attribute__((ext_vector_type(4)));
  const int Q = C >> 2;
  unsigned bad = 0u;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total_q; i += (long)gridDim.x * blockDim.x) {
    const int q = (int)(i % Q);
    long pix = i / Q;
    const int xx = (int)(pix % W); pix /= W;
    const int yy = (int)(pix % H);
    const long b = pix / H;
    const float4 v = *reinterpret_cast<const float4*>(x + i * 4);
    const float fv[4] = {v.x, v.y, v.z, v.w};
    const long o = ((((b * (H >> 1) + (yy >> 1)) * (W >> 1) + (xx >> 1)) * 4 + ((yy & 1) * 2 + (xx & 1))) * (long)C >> 2) + q;
    V4 h4, l4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      T h, l;
      round_hi_lo(fv[j], h, l);
      h4[j] = h; l4[j] = l;
    }
    reinterpret_cast<V4*>(hi)[o] = h4;
    bad |= f16_over_v4<T>(h4);
    if (lo) reinterpret_cast<V4*>(lo)[o] = l4;
  }
  f16_guard_commit(ovf, bad, STEDM_F16G_S2D);
}

extern "C" int stedm_space_to_depth16(const float* x, int C, int B, int H, int W, void* out_hi, void* out_lo, int mm_dtype, void* stream) {
  STEDM_CHECK_ARG(x && out_hi && C > 0 && C % 4 == 0 && B > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0, "space_to_depth16: bad args (C %% 4, even H/W)");
  STEDM_CHECK_ARG(mm_dtype == STEDM_F16 || mm_dtype == STEDM_BF16, "space_to_depth16: bad mm_dtype %d", mm_dtype);
  const long total_q = (long)B * H * W * (C / 4);
  unsigned* const ovf = mm_dtype == STEDM_F16 ? f16_guard_flag() : nullptr;      // the overflow guard watches fp16 planes only
  with_mm_dtype(mm_dtype, [&](auto t) {
    using T = decltype(t);
    space_to_depth16_kernel<T><<<grid_for(total_q, 16384), 256, 0, as_stream(stream)>>>(x, (T*)out_hi, (T*)out_lo, C, H, W, total_q, ovf);
  });
  STEDM_LAUNCH_CHECK();
  return 0;
}
