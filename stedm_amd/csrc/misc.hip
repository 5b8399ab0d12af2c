// Error plumbing, transposes, graph helpers, embedding path, im2col. The sampler kernels are in sampler.hip, the 16-bit packs in pack.hip.
#include <stdarg.h>

#include "common.hpp"
#include "sgemm.hpp"

namespace stedm {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
static unsigned* g_f16_guard[64] = {nullptr};
unsigned* f16_guard_flag() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  return g_f16_guard[dev];
}
}  // namespace stedm
using namespace stedm;

extern "C" int stedm_f16_guard_set(void* flag_words) {
  int dev = 0;
  STEDM_HIP_TRY(hipGetDevice(&dev));
  STEDM_CHECK_ARG(dev >= 0 && dev < 64, "f16_guard_set: device index %d out of range", dev);
  STEDM_CHECK_ARG(((uintptr_t)flag_words & 15) == 0, "f16_guard_set: the flag words must be 16-byte aligned");
  stedm::g_f16_guard[dev] = reinterpret_cast<unsigned*>(flag_words);
  return 0;
}

extern "C" int stedm_abi_version(void) { return STEDM_ABI_VERSION; }
extern "C" const char* stedm_last_error(void) { return g_err; }
extern "C" int stedm_device_cus(void) {
  int dev = 0;
  hipDeviceProp_t p;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&p, dev) != hipSuccess) {
    set_error("no HIP device");
    return -1;
  }
  return p.multiProcessorCount;
}

__global__ void transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int rows, int cols) {
  __shared__ float tile[32][33];
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
  for (int j = threadIdx.y; j < 32; j += 8) {
    const int r = by + j, c = bx + threadIdx.x;
    if (r < rows && c < cols) tile[j][threadIdx.x] = in[(long)r * cols + c];
  }
  __syncthreads();
  for (int j = threadIdx.y; j < 32; j += 8) {
    const int c = bx + j, r = by + threadIdx.x;
    if (r < rows && c < cols) out[(long)c * rows + r] = tile[threadIdx.x][j];
  }
}

extern "C" int stedm_transpose_f32(const float* in, float* out, int rows, int cols, void* stream) {
  STEDM_CHECK_ARG(in && out && rows > 0 && cols > 0, "transpose: bad args");
  dim3 grid((cols + 31) / 32, (rows + 31) / 32), block(32, 8);
  transpose_kernel<<<grid, block, 0, as_stream(stream)>>>(in, out, rows, cols);
  STEDM_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Embedding path
// ------------------------------------------------------------------------------------------------
// out[b][n] = act_out( bias[n] + sum_k act_in(x[b][k]) * wt[k][n] ),  wt K-major ([K][N]).
// Block = 64 outputs x 4 K-slices (256 threads), up to 8 batch rows per block share each weight read;
// the K split keeps the dependent-load chain short (these GEMVs are latency-, not bandwidth-bound).
constexpr int LIN_ROWS = 8;
constexpr int LIN_KC = 1024;   // K chunk staged in LDS
__global__ void __launch_bounds__(256) linear_kernel(const float* __restrict__ x, const float* __restrict__ wt,
                                                     const float* __restrict__ bias, float* __restrict__ out, int B, int K, int N,
                                                     int act_in, int act_out) {
  __shared__ float sx[LIN_ROWS * LIN_KC];
  __shared__ float part[4 * LIN_ROWS * 64];
  const int b0 = blockIdx.y * LIN_ROWS;
  const int nl = threadIdx.x & 63, ks = threadIdx.x >> 6;
  const int n = blockIdx.x * 64 + nl;
  float acc[LIN_ROWS];
#pragma unroll
  for (int r = 0; r < LIN_ROWS; ++r) acc[r] = 0.f;
  for (int kc = 0; kc < K; kc += LIN_KC) {
    const int kn = min(LIN_KC, K - kc);
    __syncthreads();
    for (int i = threadIdx.x; i < LIN_ROWS * kn; i += 256) {
      const int r = i / kn, k = i - r * kn;
      float v = (b0 + r < B) ? x[(long)(b0 + r) * K + kc + k] : 0.f;
      sx[r * LIN_KC + k] = act_in == 1 ? silu_f(v) : (act_in == 2 ? fmaxf(v, 0.f) : v);
    }
    __syncthreads();
    if (n < N) {
      const int per = (kn + 3) / 4;
      const int k0 = ks * per, k1 = min(kn, k0 + per);
#pragma unroll 8      // (eight weight loads in flight per thread: one per iteration made the B = 64 embedding Linears 40 us each, all latency)
      for (int k = k0; k < k1; ++k) {
        const float w = wt[(long)(kc + k) * N + n];
#pragma unroll
        for (int r = 0; r < LIN_ROWS; ++r) acc[r] = fmaf(sx[r * LIN_KC + k], w, acc[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < LIN_ROWS; ++r) part[(ks * LIN_ROWS + r) * 64 + nl] = acc[r];
  __syncthreads();
  if (ks == 0 && n < N) {
    const float bv = bias ? bias[n] : 0.f;
#pragma unroll
    for (int r = 0; r < LIN_ROWS; ++r) {
      if (b0 + r < B) {
        float v = bv + ((part[(0 * LIN_ROWS + r) * 64 + nl] + part[(1 * LIN_ROWS + r) * 64 + nl]) +
                        (part[(2 * LIN_ROWS + r) * 64 + nl] + part[(3 * LIN_ROWS + r) * 64 + nl]));
        out[(long)(b0 + r) * N + n] = act_out == 1 ? silu_f(v) : (act_out == 2 ? fmaxf(v, 0.f) : v);
      }
    }
  }
}

// Few-row form (B <= ROWS, N % 4 == 0): the GEMV is a pure weight stream, so the block keeps many 16-B loads in flight -
// 16 output quads x 16 K-slices, 8 independent loads per thread - and adds the 16 slice partials in a fixed order.
template <int ROWS>
__global__ void __launch_bounds__(256) linear_rows_kernel(const float* __restrict__ x, const float* __restrict__ wt,
                                                          const float* __restrict__ bias, float* __restrict__ out, int B, int K, int N,
                                                          int act_in, int act_out) {
  extern __shared__ float lsm[];
  float* sx = lsm;                         // [ROWS][K]
  float* part = lsm + ROWS * K;            // [16][ROWS][64]
  x += (long)blockIdx.y * ROWS * K;        // blockIdx.y: block of ROWS rows
  out += (long)blockIdx.y * ROWS * N;
  B = min(ROWS, B - (int)blockIdx.y * ROWS);
  const int q = threadIdx.x & 15, ks = threadIdx.x >> 4;
  const int n = blockIdx.x * 64 + q * 4;
#pragma unroll 4      // (unconditional loads from a clamped row, several in flight: a load inside the bounds branch is waited for at its join)
  for (int i = threadIdx.x; i < ROWS * K; i += 256) {
    const int r = i / K, k = i - r * K;
    float v = x[(long)min(r, B - 1) * K + k];
    v = r < B ? v : 0.f;
    sx[i] = act_in == 1 ? silu_f(v) : (act_in == 2 ? fmaxf(v, 0.f) : v);
  }
  __syncthreads();
  float acc[ROWS][4];
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[r][j] = 0.f;
  if (n < N) {
    const int per = (K + 15) / 16;
    const int k0 = ks * per, k1 = min(K, k0 + per);
#pragma unroll 8
    for (int k = k0; k < k1; ++k) {
      const float4 w = *reinterpret_cast<const float4*>(wt + (long)k * N + n);
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        const float xv = sx[r * K + k];
        acc[r][0] = fmaf(xv, w.x, acc[r][0]); acc[r][1] = fmaf(xv, w.y, acc[r][1]);
        acc[r][2] = fmaf(xv, w.z, acc[r][2]); acc[r][3] = fmaf(xv, w.w, acc[r][3]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < ROWS; ++r)
#pragma unroll
    for (int j = 0; j < 4; ++j) part[(ks * ROWS + r) * 64 + q * 4 + j] = acc[r][j];
  __syncthreads();
  const int nl = threadIdx.x & 63, r = threadIdx.x >> 6;      // 64 outputs x up to 4 rows per pass
  for (int rr = r; rr < ROWS && rr < B; rr += 4) {
    const int nn = blockIdx.x * 64 + nl;
    if (nn < N) {
      float v = bias ? bias[nn] : 0.f;
      for (int s2 = 0; s2 < 16; ++s2) v += part[(s2 * ROWS + rr) * 64 + nl];   // fixed order
      out[(long)rr * N + nn] = act_out == 1 ? silu_f(v) : (act_out == 2 ? fmaxf(v, 0.f) : v);
    }
  }
}

static int launch_linear(const float* x, const float* wt, const float* bias, float* out, int B, int K, int N, int act_in,
                         int act_out, hipStream_t st) {
  if (N % 4 == 0 && B <= 2 && (size_t)(2 * K + 16 * 2 * 64) * sizeof(float) <= 64 * 1024) {
    const size_t lds = (size_t)(2 * K + 16 * 2 * 64) * sizeof(float);
    linear_rows_kernel<2><<<(N + 63) / 64, 256, lds, st>>>(x, wt, bias, out, B, K, N, act_in, act_out);
    STEDM_LAUNCH_CHECK();
    return 0;
  }
  // 3 rows and more: the same weight stream in blocks of 8 rows (blockIdx.y), x rows resident in LDS — while the weights are re-read by few
  // enough row blocks (measured on MI355X, tools/bench_linear.py: B = 64: 7.7 / 9.9 / 38.8 us for 128 -> 512, 512 -> 512, 512 -> 10368 against
  // 9.4 / 25.9 / 53.8 us on the tiled GEMM below; B = 256, N = 10368: 136 against 85 us)
  if (N % 4 == 0 && (long)((B + 7) / 8) * ((N + 63) / 64) <= 2048 && (size_t)(8 * K + 16 * 8 * 64) * sizeof(float) <= 64 * 1024) {
    const size_t lds = (size_t)(8 * K + 16 * 8 * 64) * sizeof(float);
    linear_rows_kernel<8><<<dim3((N + 63) / 64, (B + 7) / 8), 256, lds, st>>>(x, wt, bias, out, B, K, N, act_in, act_out);
    STEDM_LAUNCH_CHECK();
    return 0;
  }
  if (B > LIN_ROWS) {      // many rows and a wide output: the tiled GEMM (sgemm.hpp), x read once per column tile
    stedm::SgemmArgs g{x, (long)K, 0, wt, (long)N, 0, out, (long)N, B, N, K, 1.0f, 0.0f, K, nullptr, bias, act_in, act_out};
    stedm::sgemm_launch(g, 1, st);
    STEDM_LAUNCH_CHECK();
    return 0;
  }
  dim3 grid((N + 63) / 64, (B + LIN_ROWS - 1) / LIN_ROWS);
  linear_kernel<<<grid, 256, 0, st>>>(x, wt, bias, out, B, K, N, act_in, act_out);
  STEDM_LAUNCH_CHECK();
  return 0;
}

// sinusoid [B][mc]: cos half first (util.py:166). T: int64 (training, DDIM) or float (DPM-Solver's fractional model times,
// dpm_solver.py:246-253); the argument t * freq is formed in fp32 either way (util.py:165 `timesteps[:, None].float() * freqs`), so an
// integer-valued float t gives the bits of the int64 path. Precise cosf / sinf: the arguments reach ~1000 rad.
template <typename T>
__global__ void sinusoid_kernel(const T* __restrict__ t, const float* __restrict__ freqs, float* __restrict__ te, int mc) {
  const int b = blockIdx.x, half = mc / 2;
  const float tv = (float)t[b];
  for (int i = threadIdx.x; i < half; i += blockDim.x) {
    const float a = tv * freqs[i];
    te[(long)b * mc + i] = cosf(a);
    te[(long)b * mc + half + i] = sinf(a);
  }
  if ((mc & 1) && threadIdx.x == 0) te[(long)b * mc + mc - 1] = 0.f;
}

// emb [B][ted]; ws: caller-provided scratch of B*(mc+ted) floats (sinusoid + hidden layer).
template <typename T>
static int time_embed_impl(const T* t, const float* freqs, const float* w0t, const float* b0, const float* w2t, const float* b2, float* emb,
                           float* ws, int B, int mc, int ted, void* stream) {
  STEDM_CHECK_ARG(t && freqs && w0t && b0 && w2t && b2 && emb && ws, "time_embed: null pointer");
  STEDM_CHECK_ARG(B > 0 && mc > 0 && ted > 0, "time_embed: bad sizes B=%d mc=%d ted=%d", B, mc, ted);
  float* te = ws;
  float* h1 = ws + (size_t)B * mc;
  hipStream_t st = as_stream(stream);
  sinusoid_kernel<T><<<B, 64, 0, st>>>(t, freqs, te, mc);
  STEDM_LAUNCH_CHECK();
  int rc = launch_linear(te, w0t, b0, h1, B, mc, ted, 0, 1, st);
  if (rc) return rc;
  return launch_linear(h1, w2t, b2, emb, B, ted, ted, 0, 0, st);
}

extern "C" int stedm_time_embed(const int64_t* t, const float* freqs, const float* w0t, const float* b0, const float* w2t,
                                const float* b2, float* emb, float* ws, int B, int mc, int ted, void* stream) {
  return time_embed_impl(t, freqs, w0t, b0, w2t, b2, emb, ws, B, mc, ted, stream);
}

extern "C" int stedm_time_embed_f32(const float* t, const float* freqs, const float* w0t, const float* b0, const float* w2t,
                                    const float* b2, float* emb, float* ws, int B, int mc, int ted, void* stream) {
  return time_embed_impl(t, freqs, w0t, b0, w2t, b2, emb, ws, B, mc, ted, stream);
}

// generic small Linear with optional input / output activation (0 none, 1 SiLU, 2 ReLU): Agg_Linear agg_blocks.py:14-18
extern "C" int stedm_linear(const float* x, const float* wt, const float* bias, float* out, int B, int k, int n, int act_in,
                            int act_out, void* stream) {
  STEDM_CHECK_ARG(x && wt && out && B > 0 && k > 0 && n > 0, "linear: bad args");
  return launch_linear(x, wt, bias, out, B, k, n, act_in, act_out, as_stream(stream));
}

extern "C" int stedm_emb_proj(const float* emb, const float* wt, const float* bias, float* out, int B, int k, int ntot,
                              void* stream) {
  STEDM_CHECK_ARG(emb && wt && bias && out, "emb_proj: null pointer");
  STEDM_CHECK_ARG(B > 0 && k > 0 && ntot > 0, "emb_proj: bad sizes B=%d k=%d ntot=%d", B, k, ntot);
  return launch_linear(emb, wt, bias, out, B, k, ntot, 1, 0, as_stream(stream));
}

// ------------------------------------------------------------------------------------------------
// Graph helpers
// ------------------------------------------------------------------------------------------------
extern "C" int stedm_graph_begin(void* stream) {
  STEDM_HIP_TRY(hipStreamBeginCapture(as_stream(stream), hipStreamCaptureModeThreadLocal));
  return 0;
}
extern "C" int stedm_graph_end(void* stream, void** graph_exec_out) {
  STEDM_CHECK_ARG(graph_exec_out, "graph_end: null out pointer");
  hipGraph_t g = nullptr;
  STEDM_HIP_TRY(hipStreamEndCapture(as_stream(stream), &g));
  hipGraphExec_t ge = nullptr;
  hipError_t e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess) {
    set_error("hipGraphInstantiate failed: %s", hipGetErrorString(e));
    return 2;
  }
  *graph_exec_out = (void*)ge;
  return 0;
}
extern "C" int stedm_graph_launch(void* graph_exec, void* stream) {
  STEDM_CHECK_ARG(graph_exec, "graph_launch: null graph");
  STEDM_HIP_TRY(hipGraphLaunch((hipGraphExec_t)graph_exec, as_stream(stream)));
  return 0;
}
extern "C" int stedm_graph_destroy(void* graph_exec) {
  if (graph_exec) STEDM_HIP_TRY(hipGraphExecDestroy((hipGraphExec_t)graph_exec));
  return 0;
}

// ------------------------------------------------------------------------------------------------ row-major im2col (16-bit), generic-shape fallback
// The implicit-GEMM kernels tile the output grid in runs of 128 / 256 pixels that must align with image rows (conv_geometry): latent widths
// that are not powers of two (96 x 96, 40 x 40, 24 x 24: anything UNetModel of the reference accepts, openaimodel.py:761-806 only needs
// H, W divisible by 4) have no such tiling. For those a 3x3 convolution runs as im2col + flat GEMM: dst [B][Ho][Wo][9 C] with column
// tap * C + c = src [b][sy][sx][c] (0 outside), then the 1x1 kind over K = 9 C with the ordinary [cout][tap][cin] weight planes (same
// contraction order as the tiled kernels' planes; every epilogue of the 1x1 kind applies). 9x the activation bytes: a correctness path.
// mode 0: stride 1 pad 1; 1: stride 2 pad 1 (Downsample.op, openaimodel.py:164-166); 2: nearest x2 then stride 1 pad 1 (Upsample, :129-131).
__global__ void __launch_bounds__(256) im2col_rows16_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, int B, int Hs, int Ws, int C8, int Ho, int Wo, int mode) {
  const long total = (long)B * Ho * Wo * 9 * C8;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c8 = (int)(i % C8);
    long r = i / C8;
    const int tap = (int)(r % 9); r /= 9;
    const int x = (int)(r % Wo); r /= Wo;
    const int y = (int)(r % Ho);
    const int b = (int)(r / Ho);
    const int dy = tap / 3 - 1, dx = tap % 3 - 1;
    int sy, sx;
    bool ok;
    if (mode == 1) { sy = 2 * y + dy; sx = 2 * x + dx; ok = sy >= 0 && sy < Hs && sx >= 0 && sx < Ws; }
    else if (mode == 2) { const int uy = y + dy, ux = x + dx; ok = uy >= 0 && uy < Ho && ux >= 0 && ux < Wo; sy = uy >> 1; sx = ux >> 1; }
    else { sy = y + dy; sx = x + dx; ok = sy >= 0 && sy < Hs && sx >= 0 && sx < Ws; }
    dst[i] = ok ? src[(((long)b * Hs + sy) * Ws + sx) * C8 + c8] : make_uint4(0u, 0u, 0u, 0u);
  }
}

extern "C" int stedm_im2col_rows16(const void* src16, void* dst16, int B, int Hs, int Ws, int C, int mode, void* stream) {
  STEDM_CHECK_ARG(src16 && dst16 && B > 0 && Hs > 0 && Ws > 0 && C > 0 && C % 8 == 0 && mode >= 0 && mode <= 2, "im2col_rows16: bad arguments (C %% 8 == 0)");
  const int Ho = mode == 1 ? (Hs - 1) / 2 + 1 : (mode == 2 ? 2 * Hs : Hs), Wo = mode == 1 ? (Ws - 1) / 2 + 1 : (mode == 2 ? 2 * Ws : Ws);
  const long total = (long)B * Ho * Wo * 9 * (C / 8);
  const long blocks = (total + 255) / 256;
  im2col_rows16_kernel<<<(int)(blocks < 65536 ? blocks : 65536), 256, 0, as_stream(stream)>>>((const uint4*)src16, (uint4*)dst16, B, Hs, Ws, C / 8, Ho, Wo, mode);
  STEDM_LAUNCH_CHECK();
  return 0;
}
