// The conv-less resampling layers of conv_resample=False (include/stedm_hip.h): the 2x2 average pool of Downsample (openaimodel.py:156-173)
// and the nearest x2 of Upsample without its convolution (:113-132), NHWC fp32. Both are bandwidth-bound producers of a tensor the next
// GroupNorm reads, so they leave its channel statistics on the way (the format of gn.hip's gn_chan_stats_kernel) and spare the separate pass.
#include "common.hpp"

namespace stedm {

// One geometry for both kernels, that of gn_chan_stats_kernel: grid (B, slots, blocks of qbs channel quads), 256 threads = QB quads x
// (256 / QB) pixel lanes. A slot is a run of `slab_px` pixels of the LOW-resolution grid [Hl][Wl] - the pool's output, the replicate's
// input - and each thread walks its pixels at stride 256 / QB with 16-byte accesses along C.
// POOL:  hi [B][2Hl][2Wl][C] -> lo [B][Hl][Wl][C], lo = 0.25 * (((a00 + a01) + a10) + a11); statistics of lo.
// !POOL: lo [B][Hl][Wl][C] -> hi [B][2Hl][2Wl][C], each of the four (+)= scale * lo; statistics of hi = 4 x those of scale * lo.
template <bool POOL>
__global__ void __launch_bounds__(256) resample2x2_kernel(const float* __restrict__ in, float* __restrict__ out, int Hl, int Wl, int C, int slab_px,
                                                          float scale, int accumulate, float* __restrict__ cs, int qbs) {
  __shared__ __attribute__((aligned(16))) float cpart[256 * 8];   // [npl][QB][8]
  const int b = blockIdx.x, slab = blockIdx.y, nslab = gridDim.y;
  const int Q = C >> 2, t = threadIdx.x, HWl = Hl * Wl;
  const int qb0 = blockIdx.z * qbs, QB = min(qbs, Q - qb0);   // qbs in {8, 16, 32, 64}
  const int npl = 256 / QB, tq = t % QB, tp = t / QB;
  const int px0 = min(HWl, slab * slab_px), px1 = min(HWl, px0 + slab_px);
  const long rowh = (long)2 * Wl * C;                          // one row of the high-resolution tensor
  const long c0 = (long)(qb0 + tq) * 4;
  const float* pin = in + (long)b * HWl * C * (POOL ? 4 : 1) + c0;
  float* pout = out + (long)b * HWl * C * (POOL ? 1 : 4) + c0;
  float s[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
  if (tp < npl) {
#pragma unroll 4
    for (int pix = px0 + tp; pix < px1; pix += npl) {
      const int y = pix / Wl, x = pix - y * Wl;
      const long ol = (long)pix * C, oh = (long)2 * y * rowh + (long)2 * x * C;
      float4 v;
      if constexpr (POOL) {
        const float* p = pin + oh;
        const float4 a0 = *reinterpret_cast<const float4*>(p), a1 = *reinterpret_cast<const float4*>(p + C);
        const float4 a2 = *reinterpret_cast<const float4*>(p + rowh), a3 = *reinterpret_cast<const float4*>(p + rowh + C);
        v = make_float4(0.25f * (((a0.x + a1.x) + a2.x) + a3.x), 0.25f * (((a0.y + a1.y) + a2.y) + a3.y),
                        0.25f * (((a0.z + a1.z) + a2.z) + a3.z), 0.25f * (((a0.w + a1.w) + a2.w) + a3.w));
        *reinterpret_cast<float4*>(pout + ol) = v;
      } else {
        const float4 a = *reinterpret_cast<const float4*>(pin + ol);
        v = make_float4(scale * a.x, scale * a.y, scale * a.z, scale * a.w);
        float* p = pout + oh;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float4* d = reinterpret_cast<float4*>(p + (k >> 1) * rowh + (k & 1) * C);
          float4 r = v;
          if (accumulate) { const float4 o = *d; r.x += o.x; r.y += o.y; r.z += o.z; r.w += o.w; }
          *d = r;
        }
      }
      s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
      q[0] += v.x * v.x; q[1] += v.y * v.y; q[2] += v.z * v.z; q[3] += v.w * v.w;
    }
  }
  if (cs == nullptr) return;        // (uniform over the block)
  if (tp < npl) {
    float* d = cpart + (tp * QB + tq) * 8;
#pragma unroll
    for (int j = 0; j < 4; ++j) { d[j] = s[j]; d[4 + j] = q[j]; }
  }
  __syncthreads();
  if (t < QB) {
    float su[4] = {0.f, 0.f, 0.f, 0.f}, sq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int l = 0; l < npl; ++l) {   // fixed order (unrolled: the LDS reads of eight lanes' partials are in flight together)
      const float4* d = reinterpret_cast<const float4*>(cpart + (l * QB + t) * 8);
      const float4 ds = d[0], dq = d[1];
      su[0] += ds.x; su[1] += ds.y; su[2] += ds.z; su[3] += ds.w;
      sq[0] += dq.x; sq[1] += dq.y; sq[2] += dq.z; sq[3] += dq.w;
    }
    const float m = POOL ? 1.f : 4.f;   // four copies of every value: exact
    float4* dst = reinterpret_cast<float4*>(cs + (((long)b * nslab + slab) * C + (qb0 + t) * 4) * 2);
    dst[0] = make_float4(m * su[0], m * sq[0], m * su[1], m * sq[1]);
    dst[1] = make_float4(m * su[2], m * sq[2], m * su[3], m * sq[3]);
  }
}

// channel quads per block: 64 (1 KiB per pixel and block) unless that leaves the chip short of four blocks per CU; never under 8 (128 B)
static int resample_qbs(int B, int nslab, int Q) {
  long cus = stedm_device_cus();
  if (cus <= 0) cus = 256;
  int qbs = 64;
  while (qbs > 8 && (long)B * nslab * ((Q + qbs - 1) / qbs) < 4 * cus) qbs >>= 1;
  return qbs;
}

template <bool POOL>
static int resample_launch(const char* name, const float* in, float* out, int B, int Hl, int Wl, int C, float scale, int accumulate, float* chan_stats,
                           int nslab, void* stream) {
  const long HWl = (long)Hl * Wl;
  // a slot is 256 pixels of the tensor the statistics describe: 256 low-resolution pixels for the pool, 64 for the replicate
  const int slab_px = POOL ? 256 : 64;
  const long want = (HWl + slab_px - 1) / slab_px;          // = stedm_gn_chan_nslab(Hout * Wout)
  STEDM_CHECK_ARG(want <= 65535, "%s: tensor too large for the launch geometry", name);
  STEDM_CHECK_ARG(((uintptr_t)in | (uintptr_t)out | (uintptr_t)chan_stats) % 16 == 0, "%s: in, out and chan_stats must be 16-byte aligned", name);
  STEDM_CHECK_ARG(chan_stats == nullptr || nslab == (int)want, "%s: nslab %d, the statistics of this shape take stedm_gn_chan_nslab(Hout * Wout) = %ld slots",
                  name, nslab, want);
  const int Q = C / 4, qbs = resample_qbs(B, (int)want, Q);
  dim3 grid(B, (unsigned)want, (Q + qbs - 1) / qbs);
  resample2x2_kernel<POOL><<<grid, 256, 0, as_stream(stream)>>>(in, out, Hl, Wl, C, slab_px, scale, accumulate, chan_stats, qbs);
  STEDM_LAUNCH_CHECK();
  return 0;
}

}  // namespace stedm

using namespace stedm;

extern "C" int stedm_avgpool2x2(const float* in, float* out, int B, int H, int W, int C, float* chan_stats, int nslab, void* stream) {
  STEDM_CHECK_ARG(in && out && B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "avgpool2x2: bad args (C %% 4)");
  STEDM_CHECK_ARG(H % 2 == 0 && W % 2 == 0, "avgpool2x2: H and W must be even, got %d x %d", H, W);
  return resample_launch<true>("avgpool2x2", in, out, B, H / 2, W / 2, C, 1.f, 0, chan_stats, nslab, stream);
}

extern "C" int stedm_replicate2x2(const float* in, float* out, int B, int H, int W, int C, float scale, int accumulate, float* chan_stats, int nslab,
                                  void* stream) {
  STEDM_CHECK_ARG(in && out && B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "replicate2x2: bad args (C %% 4)");
  STEDM_CHECK_ARG(chan_stats == nullptr || !accumulate, "replicate2x2: chan_stats needs accumulate == 0");
  return resample_launch<false>("replicate2x2", in, out, B, H, W, C, scale, accumulate, chan_stats, nslab, stream);
}
