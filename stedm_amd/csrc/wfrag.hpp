// The 16-bit weight layouts the convolution kernels read, stated once: the two MFMA fragment orders, the sub-pixel tap fold, the
// space-to-depth tap map and the hi / lo split. Index arithmetic and one rounding; no kernels. Writers: pack.hip (stedm_pack_*) and the
// optimizer pass of opt.hip (adamw_ema_pack_kernel). Plain torch restatement: tests/refs_pack.py.
#pragma once
#include "common.hpp"

namespace stedm {

#define STEDM_HD __host__ __device__ __forceinline__

// A fragment = one wave-wide 16-B load = one MFMA B operand: 64 lanes x 8 consecutive channels of one row and tap, 1 KiB contiguous.
// A pack is [tn = n / 128][chunk = c / KC][tap][f = fragment of the 128-row tile][lane][e]; rows beyond cout are zero.
struct FragCoord { int n, ci, tap; };

// 32x32x16 kind (stedm_pack_conv_weight_frag; conv_rs.inc):
//   out[tn][chunk][tap][q][lane][e] = W[n = tn*128 + q*32 + (lane&31)][ci = chunk*16 + (lane>>5)*8 + e][tap]
struct FragM32 {
  static constexpr int FR = 32, KC = 16, NFRAG = 4;     // rows per fragment, channels per chunk, fragments per 128-row tile
  static STEDM_HD int lane_row(int lane) { return lane & 31; }
  static STEDM_HD int lane_c(int lane, int /*taps*/) { return (lane >> 5) * 8; }      // channel offset of the lane's 8-vector inside its chunk
  static STEDM_HD int lane_of(int n, int c, int /*taps*/) { return (n & 31) + 32 * ((c >> 3) & 1); }
};

// 16x16x32 kind (stedm_pack_conv_weight_frag16; conv_rs.inc RS_3X3M / RS_1X1M / RS_SUBM):
//   out[tn][chunk32][tap][f][lane][e] = W[n = tn*128 + f*16 + (lane&15)][ci = chunk*32 + kofs(lane>>4, taps) + e][tap]
// kofs(g) = 8 g for a 1x1; 16 (g&1) + 8 (g>>1) for a filter with taps (a 3x3, and the 2x2 derived filters), whose reader takes two 16-channel
// (plane, piece) halves per chunk.
struct FragM16 {
  static constexpr int FR = 16, KC = 32, NFRAG = 8;
  static STEDM_HD int kofs(int g, int taps) { return taps == 1 ? 8 * g : 16 * (g & 1) + 8 * (g >> 1); }
  static STEDM_HD int kgrp(int c, int taps) { return taps == 1 ? (c >> 3) & 3 : ((c >> 4) & 1) + 2 * ((c >> 3) & 1); }     // kofs(kgrp(c)) = c & 24
  static STEDM_HD int lane_row(int lane) { return lane & 15; }
  static STEDM_HD int lane_c(int lane, int taps) { return kofs(lane >> 4, taps); }
  static STEDM_HD int lane_of(int n, int c, int taps) { return (n & 15) + 16 * kgrp(c, taps); }
};

// element offset of the 8-vector that holds (n, c .. c+7, tap); c a multiple of 8, nch = channels / KC
template <typename Frag>
STEDM_HD long frag_at(int n, int c, int tap, int nch, int taps) {
  return ((((long)(n >> 7) * nch + (unsigned)c / Frag::KC) * taps + tap) * Frag::NFRAG + (n & 127) / Frag::FR) * 512 + Frag::lane_of(n, c, taps) * 8;
}

// the inverse, for the elementwise kernels: flat element index of one pack -> (n, ci, tap)
template <typename Frag>
STEDM_HD FragCoord frag_coord(long i, int nch, int taps) {
  const int e = (int)(i & 7), lane = (int)((i >> 3) & 63);
  unsigned long r = (unsigned long)i >> 9;
  const int f = (int)(r % Frag::NFRAG); r /= Frag::NFRAG;
  const int tap = (int)(r % taps); r /= taps;
  const int chunk = (int)(r % nch), tn = (int)(r / nch);
  return {tn * 128 + f * Frag::FR + Frag::lane_row(lane), chunk * Frag::KC + Frag::lane_c(lane, taps) + e, tap};
}

// Sub-pixel upsample (nearest x2 + 3x3 as four parity 2x2 convolutions): the 3x3 rows dy0..dy1 and columns dx0..dx1 that land on low-res
// neighbour tap = a*2 + b for output parity par = py*2 + px
struct TapRange { int dy0, dy1, dx0, dx1; };
STEDM_HD TapRange subpixel_taps(int par, int tap) {
  const int py = par >> 1, px = par & 1, a = tap >> 1, b = tap & 1;
  return {py == 0 ? (a == 0 ? 0 : 1) : (a == 0 ? 0 : 2), py == 0 ? (a == 0 ? 0 : 2) : (a == 0 ? 1 : 2),
          px == 0 ? (b == 0 ? 0 : 1) : (b == 0 ? 0 : 2), px == 0 ? (b == 0 ? 0 : 2) : (b == 0 ? 1 : 2)};
}

// the pre-summed tap of an OIHW 3x3 filter; the order (from 0.f, dy outer, dx inner) is part of the bits
STEDM_HD float subpixel_weight(const float* __restrict__ w, int n, int cin, int ci, int par, int tap) {
  const TapRange t = subpixel_taps(par, tap);
  float v = 0.f;
  for (int dy = t.dy0; dy <= t.dy1; ++dy)
    for (int dx = t.dx0; dx <= t.dx1; ++dx) v += w[((long)n * cin + ci) * 9 + dy * 3 + dx];
  return v;
}

// Space-to-depth Downsample (stride-2 3x3 as a 2x2 conv over the 4 parity blocks of the planes): the 3x3 tap that tap = a*2 + b of the 2x2
// filter applies to parity block par = py*2 + px; negative = none.
// symmetric pad 1: plane rows (y-1, y) hold image rows 2y-2 .. 2y+1, the filter covers 2y-1 .. 2y+1;
// bottom/right pad (pad_br): plane rows (y, y+1) hold image rows 2y .. 2y+3, the filter covers 2y .. 2y+2
struct Tap2 { int dy, dx; };
STEDM_HD Tap2 s2d_tap(int par, int tap, int pad_br) {
  const int py = par >> 1, px = par & 1, a = tap >> 1, b = tap & 1;
  return {pad_br ? (a == 0 ? py : (py == 0 ? 2 : -1)) : (a == 0 ? (py == 1 ? 0 : -1) : (py == 0 ? 1 : 2)),
          pad_br ? (b == 0 ? px : (px == 0 ? 2 : -1)) : (b == 0 ? (px == 1 ? 0 : -1) : (px == 0 ? 1 : 2))};
}

// the 3-product split: v = hi + lo up to the rounding of lo
template <typename T>
STEDM_HD void round_hi_lo(float v, T& hi, T& lo) {
  hi = (T)v;
  lo = (T)(v - (float)hi);
}

// calls f with a value of the operand type mm_dtype names (the caller has checked it is STEDM_F16 or STEDM_BF16)
template <typename F>
inline void with_mm_dtype(int mm_dtype, F&& f) {
  if (mm_dtype == STEDM_F16) f(_Float16{});
  else f(__bf16{});
}

}  // namespace stedm
