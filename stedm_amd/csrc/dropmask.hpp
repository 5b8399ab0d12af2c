// Keep-mask streams of the train-mode dropout sites (networks/vit_set.py:28-30, 43/62, 49, 187) — the definition is in
// include/stedm_hip.h ("train-mode dropout"); the parity tests rebuild the same streams in numpy.
#pragma once
#include <stdint.h>

namespace stedm {

struct U4 { uint32_t x, y, z, w; };

// Philox4x32-10 (Salmon et al., SC'11): counter c, key (k0, k1)
__device__ __forceinline__ U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

// elementwise sites: the eight 16-bit uniforms of elements 8 g .. 8 g + 7 (field j = half (j & 1) of word j >> 1)
// (step: the fourth counter word - 0 at the sViT sites, the forward counter of the U-Net's ResBlock sites)
__device__ __forceinline__ U4 drop_group(uint64_t g, uint32_t site, uint64_t seed, uint32_t step = 0u) {
  return philox4x32_10(U4{(uint32_t)g, (uint32_t)(g >> 32), site, step}, (uint32_t)seed, (uint32_t)(seed >> 32));
}
__device__ __forceinline__ uint32_t drop_u16(const U4& r, int j) {
  const uint32_t w = (j >> 1) == 0 ? r.x : (j >> 1) == 1 ? r.y : (j >> 1) == 2 ? r.z : r.w;
  return (w >> (16 * (j & 1))) & 0xFFFFu;
}

// ResBlock sites of the U-Net (include/stedm_hip.h, "train-mode dropout": site 0x55000000 + k): what a GroupNorm pass needs to regenerate
// the keep mask of out_layers[2] from the counters - in the forward on the activation, in the backward on its gradient; no mask is stored.
struct DropArgs {
  uint64_t seed;
  uint32_t site, step;
  const int32_t* step_ptr;   // optional DEVICE word added to `step` when the kernel runs (a captured launch replays with new masks)
  uint32_t thr16;
  float inv_keep;            // (float)(1.0 / (1.0 - p))
};
__device__ __forceinline__ uint32_t drop_step_of(const DropArgs& d) { return d.step + (d.step_ptr ? (uint32_t)*d.step_ptr : 0u); }
// four values against the two output words that hold their uniforms (fields 0 .. 3 or 4 .. 7 of a group): keep ? v * inv_keep : +0
__device__ __forceinline__ void drop_apply(float& v0, float& v1, float& v2, float& v3, uint32_t w0, uint32_t w1, const DropArgs& d) {
  v0 = (w0 & 0xFFFFu) >= d.thr16 ? v0 * d.inv_keep : 0.f;
  v1 = (w0 >> 16) >= d.thr16 ? v1 * d.inv_keep : 0.f;
  v2 = (w1 & 0xFFFFu) >= d.thr16 ? v2 * d.inv_keep : 0.f;
  v3 = (w1 >> 16) >= d.thr16 ? v3 * d.inv_keep : 0.f;
}
// the four values of elements e .. e + 3 (e % 4 == 0: one half of an element group)
__device__ __forceinline__ void drop_quad(float& v0, float& v1, float& v2, float& v3, uint64_t e, const DropArgs& d, uint32_t step) {
  const U4 r = drop_group(e >> 3, d.site, d.seed, step);
  drop_apply(v0, v1, v2, v3, (e & 4u) ? r.z : r.x, (e & 4u) ? r.w : r.y, d);
}

// attention site: one xorshift128 stream (Marsaglia 2003) per (query, sample-head, key half), seeded by Philox
__device__ __forceinline__ U4 attn_stream_init(uint32_t q, uint32_t bh, uint32_t site, uint32_t h, uint64_t seed) {
  return philox4x32_10(U4{q, bh, site, h}, (uint32_t)seed, (uint32_t)(seed >> 32));
}
__device__ __forceinline__ uint32_t xs128_next(U4& s) {
  const uint32_t t = s.x ^ (s.x << 11);
  s.x = s.y; s.y = s.z; s.z = s.w;
  s.w = s.w ^ (s.w >> 19) ^ t ^ (t >> 8);
  return s.w;
}
// keep bits of one 64-key tile: bit i = (u_i >= thr16); the 16 words drawn are the bit-planes of 32 uniforms, most significant first.
// thr16 is wave-uniform: the plane loop is scalar-branched (bit-sliced comparator, 1-3 vector ops per plane)
__device__ __forceinline__ uint32_t attn_keep_bits(U4& s, uint32_t thr16) {
  uint32_t lt = 0u, eq = ~0u;
#pragma unroll
  for (int k = 15; k >= 0; --k) {
    const uint32_t b = xs128_next(s);
    if (thr16 & (1u << k)) { lt |= eq & ~b; eq &= b; }
    else eq &= ~b;
  }
  return ~lt;
}

// per-sample normal noise (stedm_philox_normal, include/stedm_hip.h): the four N(0, 1) values of element group g of the row of sample `sid`.
// Philox4x32-10(counter {g, stream, 0x4E524D4C, 0}, key {seed, sid}); Box-Muller on the word pairs with u = (w + 0.5) 2^-32, fp32 arithmetic
// with the hardware log / sin / cos. Shared by every kernel that draws these rows, so that all of them give the same bits.
__device__ __forceinline__ void philox_normal4(uint32_t g, uint32_t stream, uint32_t seed, uint32_t sid, float z[4]) {
  const U4 r = philox4x32_10(U4{g, stream, 0x4E524D4Cu, 0u}, seed, sid);
  const float k = 2.3283064365386963e-10f;     // 2^-32
  const float u0 = ((float)r.x + 0.5f) * k, u1 = ((float)r.y + 0.5f) * k, u2 = ((float)r.z + 0.5f) * k, u3 = ((float)r.w + 0.5f) * k;
  const float ra = sqrtf(-2.0f * __logf(fminf(fmaxf(u0, 1.1641532e-10f), 0.99999994f))), rb = sqrtf(-2.0f * __logf(fminf(fmaxf(u2, 1.1641532e-10f), 0.99999994f)));
  z[0] = ra * __cosf(6.283185307179586f * u1); z[1] = ra * __sinf(6.283185307179586f * u1);
  z[2] = rb * __cosf(6.283185307179586f * u3); z[3] = rb * __sinf(6.283185307179586f * u3);
}

// element e of a sample's row of stedm_philox_normal (the value philox_normal4 gives it in its group of four)
__device__ __forceinline__ float philox_normal1(uint32_t e, uint32_t stream, uint32_t seed, uint32_t sid) {
  float z[4];
  philox_normal4(e >> 2, stream, seed, sid, z);
  const uint32_t j = e & 3u;
  return j == 0 ? z[0] : j == 1 ? z[1] : j == 2 ? z[2] : z[3];
}

// DDIM noise dropout (stedm_ddim_step_ex, include/stedm_hip.h): the 16-bit uniform of element e of sample `sid`'s row at iteration `iter` =
// field (e & 7) of Philox4x32-10(counter {e >> 3, 0x20000 + iter, 0x44524F50, 0}, key {seed, sid}); the element is kept iff u16 >= thr16.
constexpr uint32_t DDIM_DROP_WORD = 0x44524F50u;      // "DROP"
__device__ __forceinline__ bool ddim_drop_keep(uint32_t e, uint32_t iter, uint32_t seed, uint32_t sid, uint32_t thr16) {
  const U4 r = philox4x32_10(U4{e >> 3, 0x20000u + iter, DDIM_DROP_WORD, 0u}, seed, sid);
  return drop_u16(r, (int)(e & 7u)) >= thr16;
}

}  // namespace stedm
