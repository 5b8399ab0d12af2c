// Per-element arithmetic that the DDIM update (sampler.hip) and quantize_x0's second half of it (vq.hip) share.
#pragma once

namespace stedm {

// sqrt(a_prev) x0 + dir e as stedm_ddim_step has always computed it: both products rounded, then the sum. Spelled out so that no form of
// either kernel, and no later compiler, contracts it into an FMA.
__device__ __forceinline__ float ddim_base_rounded(float sqrt_ap, float x0, float dir_c, float e) {
#pragma clang fp contract(off)
  return sqrt_ap * x0 + dir_c * e;
}

}  // namespace stedm
