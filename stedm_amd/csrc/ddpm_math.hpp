// Per-element arithmetic of the ancestral DDPM step (stedm_ddpm_step / stedm_ddpm_step_ex, include/stedm_hip.h), shared by its two
// launches: the quantising pre-pass (vq.hip) and the elementwise update (sampler.hip). Every product and sum is rounded on its own
// (contraction off), so with equal inputs torch's CPU arithmetic gives the same bits.
#pragma once

namespace stedm {

// predict_start_from_noise (ddpm.py:219-223) and p_mean_variance's clamp (:1069-1070)
__device__ __forceinline__ float ddpm_predict_x0(float xv, float e, float sr, float srm1, bool clip) {
#pragma clang fp contract(off)
  float q = sr * xv - srm1 * e;
  if (clip) q = q < -1.0f ? -1.0f : (q > 1.0f ? 1.0f : q);            // clamp_(-1, 1); NaN passes through, as in torch
  return q;
}

// q_posterior's mean (ddpm.py:225-232)
__device__ __forceinline__ float ddpm_posterior_mean(float q, float xv, float c1, float c2) {
#pragma clang fp contract(off)
  return c1 * q + c2 * xv;
}

// p_sample's noise (ddpm.py:1099-1101): (z temperature) keep / (1 - p); keep_scale = 1 without dropout, else (float)(1 / (1 - p)) or 0
__device__ __forceinline__ float ddpm_shaped_noise(float z, float temperature, float keep_scale) {
#pragma clang fp contract(off)
  return (z * temperature) * keep_scale;
}

// p_sample's return value (ddpm.py:1107-1110), sigma = nonzero(t) exp(0.5 logvar) from the table
__device__ __forceinline__ float ddpm_add_noise(float mean, float sig, float n) {
#pragma clang fp contract(off)
  return mean + sig * n;
}

// The pre-pass of stedm_ddpm_step_ex with a codebook (vq.hip): x0_out = the predicted x0 snapped to its nearest codebook row.
int ddpm_quantize_x0_launch(const float* x, const float* eps, const float* table, const int32_t* step_idx, const int64_t* t, int T, int clip,
                            const float* codebook, int n_e, int e_dim, int B, long HW, float* x0_out, long long* idx_out, hipStream_t st);

}  // namespace stedm
