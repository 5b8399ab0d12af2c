// The conv-less resampling layers of conv_resample=False (include/stedm_hip.h): the 2x2 average pool of Downsample (openaimodel.py:156-173)
// and the nearest x2 of Upsample without its convolution (:113-132), NHWC fp32. Both are bandwidth-bound producers of a tensor the next
// GroupNorm reads, so they leave its channel statistics on the way (the format of gn.hip's gn_chan_stats_kernel) and spare the separate pass.
#include "common.hpp"
#include "gn_fold.hpp"

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

// ================================================================================================
// GroupNorm + activation + 2x2 resample into the 16-bit operand planes, and the resampled raw input: the front of ResBlock(up / down)
// ================================================================================================
// (openaimodel.py:268-275: h = h_upd(in_layers[:-1](x)), x = x_upd(x).) One read of x [B][H][W][C] gives both branches at the new resolution:
//   a  = act((x - mean) * (rstd * gamma) + beta)        the table rows, the order and the functions of gn_apply16c_v8_kernel (gn.hip)
//   MODE 1 (pool):    planes [B][H/2][W/2][C] = split16(0.25 * (((a00 + a01) + a10) + a11)), xr the same expression on raw x (= stedm_avgpool2x2)
//   MODE 2 (nearest): planes [B][2H][2W][C] = split16(a) at the four positions (2y + dy, 2x + dx), xr = x there (= stedm_replicate2x2, scale 1)
// Geometry: grid (B, runs of low-resolution pixels); a block folds its sample's statistics (gn_fold.hpp, all groups in one fold: the order of
// the apply kernels' pixel-run blocks, so mean / rstd carry their bits), builds the table [3][C] in LDS and streams its run. A lane loads
// coalesced float4 quads and owns TWO cursors (quads e and e + 256 of the block's iteration); lane pairs swap one 8-B half before the plane
// stores, as in gn_apply16c_v8_kernel, so every access is 16 B per lane: the even lane stores the octet of cursor 0, the odd lane that of
// cursor 1. The pool has 8 loads per lane in flight, the nearest 2 loads against 12 - 16 stores (it is bound by its writes).
// The fp16 guard's switch is the one of the normalised planes (gn_build_table): an average of four in-range values stays in range.
struct GnResampleArgs {
  const float* x;
  const float* cs;
  int C, nslab, groups, HW, act;    // HW: pixels of x
  const float* gamma;
  const float* beta;
  float eps;
  int Hl, Wl;                       // the low-resolution grid: the pool's output, the nearest's input
  void* out_hi;
  void* out_lo;
  float* xr;
  float* mr;
  unsigned* ovf;
};

template <typename T, int MODE>
__global__ void __launch_bounds__(256) gn_apply16c_resample_kernel(GnResampleArgs a, int run) {
  typedef T V4 __attribute__((ext_vector_type(4)));
  constexpr bool POOL = MODE == 1;
  __shared__ double dsu[256], dsq[256];
  __shared__ float lmean[64], lrstd[64];
  extern __shared__ __attribute__((aligned(16))) float tab[];   // [3][C]: mean, rstd * gamma, beta per channel
  const int b = blockIdx.x, sl = blockIdx.y;
  const int C = a.C, Q = C >> 2, cpg = C / a.groups;
  const int HWl = a.Hl * a.Wl;
  const int px0 = sl * run, px1 = min(HWl, px0 + run);
  const int total = (px1 - px0) * Q;                            // quads of this block, even (C % 8 == 0)
  const long rowh = (long)2 * a.Wl * C;                         // one row of the high-resolution tensor
  const float* pin = a.x + (long)b * a.HW * C;
  float* pxr = a.xr ? a.xr + (long)b * HWl * C * (POOL ? 1 : 4) : nullptr;
  uint2* oh = reinterpret_cast<uint2*>(a.out_hi) + (long)b * HWl * Q * (POOL ? 1 : 4);      // 8-B units (one quad of 16-bit values)
  uint2* ol = a.out_lo ? reinterpret_cast<uint2*>(a.out_lo) + (long)b * HWl * Q * (POOL ? 1 : 4) : nullptr;
  const GnPartials part{a.cs, a.nslab, C, nullptr, 0, 0, a.groups, a.HW, a.eps, a.mr};
  const bool guard = a.ovf != nullptr && __is_same(T, _Float16);
  gn_fold_block<false>(part, b, b, 0, a.groups, sl == 0, dsu, dsq, lmean, lrstd);
  const bool norm_over = gn_build_table(tab, lmean, lrstd, a.gamma, a.beta, C, cpg, a.HW, 0, C, guard);
  unsigned bad = 0u;
  const bool odd = threadIdx.x & 1;
  auto pair16 = [&](uint2 q0, uint2 q1) {       // gn_apply16c_v8_kernel's exchange: {even lane's quad, odd lane's quad} of the cursor this lane owns
    const uint2 give = odd ? q0 : q1;
    uint2 got;
    got.x = __shfl_xor(give.x, 1, 64); got.y = __shfl_xor(give.y, 1, 64);
    uint4 r;
    if (odd) { r.x = got.x; r.y = got.y; r.z = q1.x; r.w = q1.y; }
    else { r.x = q0.x; r.y = q0.y; r.z = got.x; r.w = got.y; }
    return r;
  };
  auto norm4 = [&](float4 w, const float4& mn, const float4& sc, const float4& bt) {
    w.x = (w.x - mn.x) * sc.x + bt.x; w.y = (w.y - mn.y) * sc.y + bt.y; w.z = (w.z - mn.z) * sc.z + bt.z; w.w = (w.w - mn.w) * sc.w + bt.w;
    if (a.act == 1) { w.x = silu_f(w.x); w.y = silu_f(w.y); w.z = silu_f(w.z); w.w = silu_f(w.w); }
    return w;
  };
  auto pool4 = [](const float4& a0, const float4& a1, const float4& a2, const float4& a3) {
    return make_float4(0.25f * (((a0.x + a1.x) + a2.x) + a3.x), 0.25f * (((a0.y + a1.y) + a2.y) + a3.y),
                       0.25f * (((a0.z + a1.z) + a2.z) + a3.z), 0.25f * (((a0.w + a1.w) + a2.w) + a3.w));
  };
  constexpr int NL = POOL ? 4 : 1;
  for (int i0 = 0; i0 < total; i0 += 512) {     // (block-uniform trip count: the exchange below runs in every lane)
    bool live[2];
    int pix[2], q[2];
    float4 v[2][NL];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int e = i0 + (int)threadIdx.x + k * 256;
      live[k] = e < total;                      // (total and 256 are even: a lane pair is live or dead together)
      const int ee = live[k] ? e : 0;           // a dead cursor re-reads the block's first quad and stores nothing
      pix[k] = px0 + ee / Q; q[k] = ee % Q;
      const int y = pix[k] / a.Wl, x = pix[k] - y * a.Wl;
      if constexpr (POOL) {
        const float* p = pin + (long)2 * y * rowh + (long)2 * x * C + q[k] * 4;
        v[k][0] = *reinterpret_cast<const float4*>(p); v[k][1] = *reinterpret_cast<const float4*>(p + C);
        v[k][2] = *reinterpret_cast<const float4*>(p + rowh); v[k][3] = *reinterpret_cast<const float4*>(p + rowh + C);
      } else {
        v[k][0] = *reinterpret_cast<const float4*>(pin + (long)pix[k] * C + q[k] * 4);
      }
    }
    uint2 oq[2], olq[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int c = q[k] * 4;
      const float4 mn = *reinterpret_cast<const float4*>(tab + c);
      const float4 sc = *reinterpret_cast<const float4*>(tab + C + c);
      const float4 bt = *reinterpret_cast<const float4*>(tab + 2 * C + c);
      float4 w;
      if constexpr (POOL) {
        w = pool4(norm4(v[k][0], mn, sc, bt), norm4(v[k][1], mn, sc, bt), norm4(v[k][2], mn, sc, bt), norm4(v[k][3], mn, sc, bt));
        if (pxr && live[k]) *reinterpret_cast<float4*>(pxr + (long)pix[k] * C + c) = pool4(v[k][0], v[k][1], v[k][2], v[k][3]);
      } else {
        w = norm4(v[k][0], mn, sc, bt);
        if (pxr && live[k]) {
          const int y = pix[k] / a.Wl, x = pix[k] - y * a.Wl;
          float* p = pxr + (long)2 * y * rowh + (long)2 * x * C + c;
          *reinterpret_cast<float4*>(p) = v[k][0]; *reinterpret_cast<float4*>(p + C) = v[k][0];
          *reinterpret_cast<float4*>(p + rowh) = v[k][0]; *reinterpret_cast<float4*>(p + rowh + C) = v[k][0];
        }
      }
      V4 lo;
      oq[k] = __builtin_bit_cast(uint2, split16<T>(w, ol != nullptr, lo));
      if (norm_over && live[k]) bad |= f16_over4<T>(oq[k]);
      if (ol) olq[k] = __builtin_bit_cast(uint2, lo);
    }
    // my cursor: 0 on even lanes, 1 on odd lanes; the 16-B destination starts at the even lane's quad of it
    const bool mlive = odd ? live[1] : live[0];
    const int mpix = odd ? pix[1] : pix[0], mq = (odd ? q[1] : q[0]) & ~1;
    const uint4 so = pair16(oq[0], oq[1]);
    uint4 sl4 = make_uint4(0u, 0u, 0u, 0u);
    if (ol) sl4 = pair16(olq[0], olq[1]);
    if (mlive) {
      if constexpr (POOL) {
        const long o = (long)mpix * Q + mq;
        *reinterpret_cast<uint4*>(oh + o) = so;
        if (ol) *reinterpret_cast<uint4*>(ol + o) = sl4;
      } else {
        const int y = mpix / a.Wl, x = mpix - y * a.Wl;
        const long rq = (long)2 * a.Wl * Q;     // one high-resolution row, in quads
        const long o = (long)2 * y * rq + (long)2 * x * Q + mq;
        *reinterpret_cast<uint4*>(oh + o) = so; *reinterpret_cast<uint4*>(oh + o + Q) = so;
        *reinterpret_cast<uint4*>(oh + o + rq) = so; *reinterpret_cast<uint4*>(oh + o + rq + Q) = so;
        if (ol) {
          *reinterpret_cast<uint4*>(ol + o) = sl4; *reinterpret_cast<uint4*>(ol + o + Q) = sl4;
          *reinterpret_cast<uint4*>(ol + o + rq) = sl4; *reinterpret_cast<uint4*>(ol + o + rq + Q) = sl4;
        }
      }
    }
  }
  if (norm_over) f16_guard_commit(a.ovf, bad, STEDM_F16G_NORM);
}

template <int MODE>
static int gn_resample_launch(const GnResampleArgs& a, int B, int mm_dtype, void* stream) {
  // Low-resolution pixels per block, the rule of gn_apply16c_launch on the bytes of x a block reads: runs of 128 KiB of fp32 input (every
  // block folds the statistics and builds the table first, a cost that grows with C) unless that leaves fewer than three blocks per CU.
  const long HWl = (long)a.Hl * a.Wl;
  long cus = stedm_device_cus();
  if (cus <= 0) cus = 256;
  const long src_px = (long)a.C * (MODE == 1 ? 4 : 1);                          // floats of x per low-resolution pixel
  const long want = (128 * 256 + src_px - 1) / src_px;
  long per_sample = (HWl + want - 1) / want;
  const long need = (3 * cus + B - 1) / B;
  if (per_sample < need) per_sample = need;
  if (per_sample > HWl) per_sample = HWl;
  const long run = (HWl + per_sample - 1) / per_sample;
  const long ny = (HWl + run - 1) / run;
  STEDM_CHECK_ARG(ny <= 65535, "gn_apply16c_resample: tensor too large for the launch geometry");
  dim3 grid(B, (unsigned)ny);
  const size_t lds = (size_t)3 * a.C * sizeof(float);
  if (mm_dtype == STEDM_F16) gn_apply16c_resample_kernel<_Float16, MODE><<<grid, 256, lds, as_stream(stream)>>>(a, (int)run);
  else gn_apply16c_resample_kernel<__bf16, MODE><<<grid, 256, lds, as_stream(stream)>>>(a, (int)run);
  STEDM_LAUNCH_CHECK();
  return 0;
}

}  // namespace stedm

using namespace stedm;

extern "C" int stedm_gn_apply16c_resample(const float* x, int C, const float* cs, int nslab, const float* gamma, const float* beta, float eps, int groups,
                                          int act, int B, int H, int W, int mode, void* out_hi, void* out_lo, float* xr, float* mean_rstd, int mm_dtype,
                                          void* stream) {
  STEDM_CHECK_ARG(x && cs && gamma && beta && out_hi, "gn_apply16c_resample: null pointer");
  STEDM_CHECK_ARG(mode == 1 || mode == 2, "gn_apply16c_resample: mode must be 1 (pool) or 2 (nearest), got %d", mode);
  STEDM_CHECK_ARG(B > 0 && H > 0 && W > 0 && nslab > 0, "gn_apply16c_resample: bad B / H / W / nslab");
  STEDM_CHECK_ARG(C > 0 && C % 8 == 0 && (size_t)3 * C * sizeof(float) <= 48 * 1024, "gn_apply16c_resample: need C %% 8 == 0 and C <= 4096 (C=%d)", C);
  STEDM_CHECK_ARG(groups > 0 && groups <= 64 && C % groups == 0, "gn_apply16c_resample: need groups <= 64 and C %% groups == 0");
  STEDM_CHECK_ARG(mode != 1 || (H % 2 == 0 && W % 2 == 0), "gn_apply16c_resample: the pool needs even H and W, got %d x %d", H, W);
  STEDM_CHECK_ARG((long)H * W <= (1L << 28), "gn_apply16c_resample: sample too large");
  STEDM_CHECK_ARG(mm_dtype == STEDM_F16 || mm_dtype == STEDM_BF16, "gn_apply16c_resample: bad mm_dtype");
  STEDM_CHECK_ARG(((uintptr_t)x | (uintptr_t)out_hi | (uintptr_t)out_lo | (uintptr_t)xr) % 16 == 0, "gn_apply16c_resample: x, the planes and xr must be 16-byte aligned");
  GnResampleArgs a{x, cs, C, nslab, groups, H * W, act, gamma, beta, eps, mode == 1 ? H / 2 : H, mode == 1 ? W / 2 : W, out_hi, out_lo, xr, mean_rstd,
                   mm_dtype == STEDM_F16 ? f16_guard_flag() : nullptr};
  return mode == 1 ? gn_resample_launch<1>(a, B, mm_dtype, stream) : gn_resample_launch<2>(a, B, mm_dtype, stream);
}

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
