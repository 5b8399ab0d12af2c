// KL first stage (AutoencoderKL, ldm/models/autoencoder.py:285-342): the posterior's sampling step.
//   gauss_sample   DiagonalGaussianDistribution.sample / .mode (ldm/modules/distributions/distributions.py:24-37, 61-62) fused with the
//                  scale of LatentDiffusion.get_first_stage_encoding (ddpm.py:552): moments NCHW [B][2C][HW] (channels [0, C) the mean,
//                  [C, 2C) the log-variance) -> z [B][C][HW] = scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise)
// The rest of the stage (Encoder / Decoder, the 1x1 glue convs) runs on the kernels the VQ stage uses.
// Every product and sum is rounded on its own (no contraction), the exponential is the accurate expf: the given-noise form and the
// in-kernel draw give the same bits for the same noise, and torch's unfused CPU expression is met to the last ulp of expf.
#include "common.hpp"
#include "dropmask.hpp"
using namespace stedm;

namespace {

// torch.clamp(logvar, -30, 20): a NaN stays a NaN
__device__ __forceinline__ float gauss_clamp_logvar(float lv) { return lv < -30.0f ? -30.0f : (lv > 20.0f ? 20.0f : lv); }

__device__ __forceinline__ float gauss_sample1(float mean, float logvar, float noise, float scale) {
#pragma clang fp contract(off)
  const float sd = expf(0.5f * gauss_clamp_logvar(logvar));
  const float t = sd * noise;
  const float s = mean + t;
  return scale * s;
}

// A sample's mean and log-variance are two consecutive rows of n = C HW floats, its z one row of n. Grid (ceil(n / 4 / 256), B): one
// thread = group g of four consecutive elements of sample b's row - the group of philox_normal4, so the draw costs one Philox block per
// thread and is stedm_philox_normal's row bit for bit. VEC (n % 4 == 0 and every operand 16-byte aligned): float4 loads and stores;
// otherwise the scalar form, any n, the elements past the row's end neither read nor written.
// MODE 0: noise given; 1: noise drawn (row id0 + b, stream STEDM_STREAM_POSTERIOR); 2: the distribution's mode, z = scale * mean
template <bool VEC, int MODE>
__global__ void __launch_bounds__(256) gauss_sample_kernel(const float* __restrict__ moments, const float* __restrict__ noise, float* __restrict__ z,
                                                           int n, float scale, unsigned id0, unsigned seed) {
  const int b = blockIdx.y;
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (4 * (long)g >= n) return;
  const float* pm = moments + (long)b * 2 * n + 4 * (long)g;
  const long o = (long)b * n + 4 * (long)g;
  const int live = n - 4 * g < 4 ? n - 4 * g : 4;     // elements of this group inside the row
  float m[4], lv[4] = {0.f, 0.f, 0.f, 0.f}, nz[4] = {0.f, 0.f, 0.f, 0.f}, out[4];
  if (VEC) {
    const float4 q = *reinterpret_cast<const float4*>(pm);
    m[0] = q.x; m[1] = q.y; m[2] = q.z; m[3] = q.w;
    if (MODE != 2) {
      const float4 l = *reinterpret_cast<const float4*>(pm + n);
      lv[0] = l.x; lv[1] = l.y; lv[2] = l.z; lv[3] = l.w;
    }
    if (MODE == 0) {
      const float4 e = *reinterpret_cast<const float4*>(noise + o);
      nz[0] = e.x; nz[1] = e.y; nz[2] = e.z; nz[3] = e.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      m[j] = j < live ? pm[j] : 0.f;
      if (MODE != 2) lv[j] = j < live ? pm[n + j] : 0.f;
      if (MODE == 0) nz[j] = j < live ? noise[o + j] : 0.f;
    }
  }
  if (MODE == 1) philox_normal4((unsigned)g, STEDM_STREAM_POSTERIOR, seed, id0 + (unsigned)b, nz);
#pragma unroll
  for (int j = 0; j < 4; ++j) out[j] = MODE == 2 ? scale * m[j] : gauss_sample1(m[j], lv[j], nz[j], scale);
  if (VEC) {
    *reinterpret_cast<float4*>(z + o) = make_float4(out[0], out[1], out[2], out[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < live) z[o + j] = out[j];
  }
}

}  // namespace

extern "C" int stedm_gauss_sample(const float* moments, const float* noise, float* z, int B, int C, long HW, float scale, int mode, long first_id,
                                  unsigned long long seed, void* stream) {
  STEDM_CHECK_ARG(moments && z, "gauss_sample: null pointer");
  STEDM_CHECK_ARG(B > 0 && B <= 65535 && C > 0 && HW > 0 && (long)C * HW <= 0x3FFFFFFFL, "gauss_sample: bad shape B=%d C=%d HW=%ld", B, C, HW);
  STEDM_CHECK_ARG(mode == 0 || mode == 1, "gauss_sample: mode %d (0: sample, 1: the distribution's mode)", mode);
  STEDM_CHECK_ARG(first_id >= 0 && first_id + B <= (1L << 32), "gauss_sample: sample ids %ld + %d outside [0, 2^32]", first_id, B);
  const int n = (int)((long)C * HW);
  const dim3 grid((unsigned)(((n + 3) / 4 + 255) / 256), (unsigned)B);
  const uintptr_t bits = (uintptr_t)moments | (uintptr_t)noise | (uintptr_t)z;
  const bool vec = n % 4 == 0 && bits % 16 == 0;
  const int m = mode == 1 ? 2 : (noise ? 0 : 1);
  hipStream_t st = as_stream(stream);
  const unsigned id0 = (unsigned)first_id, sd = (unsigned)(seed & 0xFFFFFFFFull);
#define LAUNCH(V, M) gauss_sample_kernel<V, M><<<grid, 256, 0, st>>>(moments, noise, z, n, scale, id0, sd)
  if (vec) {
    if (m == 0) LAUNCH(true, 0); else if (m == 1) LAUNCH(true, 1); else LAUNCH(true, 2);
  } else {
    if (m == 0) LAUNCH(false, 0); else if (m == 1) LAUNCH(false, 1); else LAUNCH(false, 2);
  }
#undef LAUNCH
  STEDM_LAUNCH_CHECK();
  return 0;
}
