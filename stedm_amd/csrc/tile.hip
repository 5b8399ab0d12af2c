// Patch-distributed first stage (ddpm.py:567-654, 709-766, 829-866; stedm_amd/tiling.py): gather overlapping crops, stitch the first stage's
// crop outputs with border-distance weights. Both kernels stream: one thread per 4 (or 1) consecutive x, 16 B per lane where the crop width,
// the x stride and the row pitch are multiples of 4 floats (crop boundaries then fall on 4-element groups), a scalar path otherwise.
#include "common.hpp"

using namespace stedm;

namespace {

template <int VEC>
__device__ __forceinline__ void load_v(const float* __restrict__ p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = *p;
  }
}

template <int VEC>
__device__ __forceinline__ void store_v(float* __restrict__ p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    *p = v[0];
  }
}

// image_to_uint8_kernel's conversion (post.hip) on a register value: add, then multiply, no FMA contraction, C-style truncation
__device__ __forceinline__ unsigned to_u8(float v) {
  v = fminf(fmaxf(v, -1.0f), 1.0f);
  return (unsigned)(uint8_t)(int)__fmul_rn(__fadd_rn(v, 1.0f), 127.5f);
}

// tiles[i][bc][y][x] = x[bc][ly*sy + y][lx*sx + x] for crop l = l0 + i = ly*Lx + lx. blockIdx.x: plane i*BC + bc; blockIdx.y, threadIdx.x: the
// plane's elements in groups of VEC.
template <int VEC>
__global__ void unfold_tiles_kernel(const float* __restrict__ x, float* __restrict__ tiles, int BC, int H, int W, int kh, int kw, int sy,
                                    int sx, int Lx, int l0) {
  const int kwv = kw / VEC;
  const int idx = (int)(blockIdx.y * blockDim.x + threadIdx.x);
  if (idx >= kh * kwv) return;
  const int y = idx / kwv, xv = idx - y * kwv;
  const long plane = blockIdx.x;
  const int i = (int)(plane / BC), bc = (int)(plane - (long)i * BC);
  const int l = l0 + i, ly = l / Lx, lx = l - ly * Lx;
  float v[VEC];
  load_v<VEC>(x + ((long)bc * H + (ly * sy + y)) * W + lx * sx + xv * VEC, v);
  store_v<VEC>(tiles + (plane * kh + y) * (long)kw + xv * VEC, v);
}

// One thread per (b, Y, VEC consecutive X): the covering crops in ascending (ly, lx), channels in chunks of 4 so that a crop's weight is read
// once per chunk. weight = w_tile * w_tie[l] rounded first (get_weighting, ddpm.py:601), products and sums rounded one by one, one division.
template <int VEC>
__global__ void fold_blend_kernel(const float* __restrict__ tiles, const float* __restrict__ w_tile, const float* __restrict__ w_tie,
                                  float* __restrict__ out, uint8_t* __restrict__ out_u8, int B, int C, int th, int tw, int sy, int sx, int Ly,
                                  int Lx, int Ho, int Wo, long total) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int Wv = Wo / VEC;
  const long row = idx / Wv;
  const int X = (int)(idx - row * Wv) * VEC;
  const int b = (int)(row / Ho), Y = (int)(row - (long)b * Ho);
  const int ly_lo = Y < th ? 0 : (Y - th) / sy + 1, ly_hi = min(Ly - 1, Y / sy);
  const int lx_lo = X < tw ? 0 : (X - tw) / sx + 1, lx_hi = min(Lx - 1, X / sx);
  const long plane = (long)th * tw;
  for (int c0 = 0; c0 < C; c0 += 4) {
    float acc[4][VEC], den[VEC];
#pragma unroll
    for (int p = 0; p < VEC; ++p) {
      den[p] = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j][p] = 0.f;
    }
    for (int ly = ly_lo; ly <= ly_hi; ++ly) {
      for (int lx = lx_lo; lx <= lx_hi; ++lx) {
        const int l = ly * Lx + lx;
        const long off = (long)(Y - ly * sy) * tw + (X - lx * sx);
        const float tie = w_tie[l];
        float w[VEC];
        load_v<VEC>(w_tile + off, w);
#pragma unroll
        for (int p = 0; p < VEC; ++p) {
          w[p] = __fmul_rn(w[p], tie);
          den[p] = __fadd_rn(den[p], w[p]);
        }
        const float* src = tiles + (((long)l * B + b) * C + c0) * plane + off;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (c0 + j < C) {
            float o[VEC];
            load_v<VEC>(src + j * plane, o);
#pragma unroll
            for (int p = 0; p < VEC; ++p) acc[j][p] = __fadd_rn(acc[j][p], __fmul_rn(o[p], w[p]));
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int p = 0; p < VEC; ++p) acc[j][p] = __fdiv_rn(acc[j][p], den[p]);
    if (out != nullptr) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c0 + j < C) store_v<VEC>(out + (((long)b * C + c0 + j) * Ho + Y) * Wo + X, acc[j]);
    }
    if (out_u8 != nullptr) {
      uint8_t* dst = out_u8 + (row * Wo + X) * C + c0;      // NHWC: pixel (b, Y, X + p) at + p*C
      if (VEC == 4 && C == 3) {
        // 4 pixels x 3 channels = 12 contiguous bytes at a multiple of 12: three dword stores
        unsigned word[3] = {0u, 0u, 0u};
#pragma unroll
        for (int p = 0; p < VEC; ++p)
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const int k = p * 3 + j;
            word[k >> 2] |= to_u8(acc[j][p]) << ((k & 3) * 8);
          }
        unsigned* d32 = reinterpret_cast<unsigned*>(dst);
        d32[0] = word[0]; d32[1] = word[1]; d32[2] = word[2];
      } else {
#pragma unroll
        for (int p = 0; p < VEC; ++p)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (c0 + j < C) dst[(long)p * C + j] = (uint8_t)to_u8(acc[j][p]);
      }
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" int stedm_unfold_tiles(const float* x, float* tiles, int B, int C, int H, int W, int kh, int kw, int sy, int sx, int l0, int nl,
                                  void* stream) {
  STEDM_CHECK_ARG(x && tiles && B > 0 && C > 0 && H > 0 && W > 0, "unfold_tiles: bad args");
  STEDM_CHECK_ARG(kh > 0 && kw > 0 && kh <= H && kw <= W && sy > 0 && sx > 0, "unfold_tiles: crop %d x %d, stride %d x %d over %d x %d", kh, kw,
                  sy, sx, H, W);
  const long Ly = (H - kh) / sy + 1, Lx = (W - kw) / sx + 1;
  STEDM_CHECK_ARG(l0 >= 0 && nl > 0 && (long)l0 + nl <= Ly * Lx, "unfold_tiles: crops %d .. %ld outside the %ld x %ld grid", l0,
                  (long)l0 + nl - 1, Ly, Lx);
  const long planes = (long)nl * B * C;
  STEDM_CHECK_ARG((long)kh * kw < (1L << 31) && planes < (1L << 31) && (long)B * C < (1L << 31), "unfold_tiles: shape too large");
  const bool vec = (kw % 4 == 0) && (sx % 4 == 0) && (W % 4 == 0) && aligned16(x) && aligned16(tiles);
  const long per = (long)kh * (kw / (vec ? 4 : 1));
  const long by = (per + 255) / 256;
  STEDM_CHECK_ARG(by <= 65535, "unfold_tiles: crop %d x %d too large for one launch", kh, kw);
  const dim3 grid((unsigned)planes, (unsigned)by);
  if (vec)
    unfold_tiles_kernel<4><<<grid, 256, 0, as_stream(stream)>>>(x, tiles, B * C, H, W, kh, kw, sy, sx, (int)Lx, l0);
  else
    unfold_tiles_kernel<1><<<grid, 256, 0, as_stream(stream)>>>(x, tiles, B * C, H, W, kh, kw, sy, sx, (int)Lx, l0);
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int stedm_fold_blend(const float* tiles, const float* w_tile, const float* w_tie, float* out, unsigned char* out_u8, int B, int C,
                                int th, int tw, int sy, int sx, int Ly, int Lx, void* stream) {
  STEDM_CHECK_ARG(tiles && w_tile && w_tie && (out || out_u8) && B > 0 && C > 0, "fold_blend: bad args (out or out_u8 must be given)");
  STEDM_CHECK_ARG(th > 0 && tw > 0 && Ly > 0 && Lx > 0 && sy > 0 && sx > 0, "fold_blend: tile %d x %d, stride %d x %d, grid %d x %d", th, tw, sy,
                  sx, Ly, Lx);
  STEDM_CHECK_ARG((sy <= th || Ly == 1) && (sx <= tw || Lx == 1), "fold_blend: stride %d x %d larger than the tile %d x %d leaves pixels no crop covers",
                  sy, sx, th, tw);
  const long Ho = (long)(Ly - 1) * sy + th, Wo = (long)(Lx - 1) * sx + tw;
  STEDM_CHECK_ARG(Ho < (1L << 31) && Wo < (1L << 31) && (long)Ly * Lx < (1L << 31) && (long)B * Ho < (1L << 31), "fold_blend: shape too large");
  const bool vec = (tw % 4 == 0) && (sx % 4 == 0 || Lx == 1) && aligned16(tiles) && aligned16(w_tile) && (out == nullptr || aligned16(out)) &&
                   (out_u8 == nullptr || (reinterpret_cast<uintptr_t>(out_u8) & 3u) == 0);
  const long total = (long)B * Ho * (Wo / (vec ? 4 : 1));
  const long blocks = (total + 255) / 256;
  STEDM_CHECK_ARG(blocks < (1L << 31), "fold_blend: output too large for one launch");
  if (vec)
    fold_blend_kernel<4><<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(tiles, w_tile, w_tie, out, out_u8, B, C, th, tw, sy, sx, Ly, Lx, (int)Ho,
                                                                         (int)Wo, total);
  else
    fold_blend_kernel<1><<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(tiles, w_tile, w_tie, out, out_u8, B, C, th, tw, sy, sx, Ly, Lx, (int)Ho,
                                                                         (int)Wo, total);
  STEDM_LAUNCH_CHECK();
  return 0;
}
