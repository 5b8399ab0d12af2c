// SiLU and its derivative as the training backward evaluates them, accurate in the negative tail: silu_tail_f and silu_grad on top of
// sigmoid_up. Used by the GroupNorm backward kernels (gn_bwd.hip) and by silu_kernel (bwd.hip), which must agree bit for bit.
#pragma once

namespace stedm {

// sigmoid(y) / down, with down = 2^-32 below y = -64 and 1 elsewhere. v_rcp_f32 flushes a denormal result and v_exp_f32 overflows past
// 88.7, so the plain rcp(1 + exp(-y)) is 0 below y = -87.3, where y * sigmoid(y) and silu'(y) are still normal numbers (down to y = -92.5).
// Scaling the denominator by a power of two keeps the reciprocal normal down to y = -110 and changes no bit for y >= -64.
__device__ __forceinline__ float sigmoid_up(float y, float& down) {
  const bool tail = y < -64.0f;
  down = tail ? 0x1p-32f : 1.0f;
  const float e = __builtin_amdgcn_exp2f(fmaf(-y, 1.44269504088896340736f, tail ? -32.0f : 0.0f));   // exp(-y) * down
  return __builtin_amdgcn_rcpf(down + e);
}

// y * sigmoid(y), accurate in the negative tail too (common.hpp's silu_f, which the fused forward epilogues use, flushes to 0 there)
__device__ __forceinline__ float silu_tail_f(float y) {
  float down;
  const float su = sigmoid_up(y, down);
  return (y * su) * down;
}

__device__ __forceinline__ float silu_grad(float y) {
  float down;
  const float su = sigmoid_up(y, down);
  return (su * (1.0f + y * (1.0f - su * down))) * down;
}

}  // namespace stedm
