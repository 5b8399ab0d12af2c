// The sampler kernels: the DDIM update, the step counter helpers, the DPM-Solver++(2M) and PLMS updates, per-sample normal noise, the mask
// blend and the ancestral DDPM step. (The general DPM-Solver is in dpm.hip.)
#include <initializer_list>
#include <type_traits>

#include "common.hpp"
#include "dropmask.hpp"
#include "ddim_math.hpp"
#include "ddpm_math.hpp"

using namespace stedm;

// ------------------------------------------------------------------------------------------------
// DDIM update + rescaled CFG (ddim.py:179-210). stedm_ddim_step, stedm_ddim_step_ex and stedm_ddim_step_rows run one kernel,
// ddim_step_kernel<Form, R, DRAW, EXT>: thread = (col, part); part strides the C H rows of column w, so a thread's sums run over
// r = part, part + parts, ... and the parts of a column meet in LDS. The rescale statistic of ddim.py:182-183 is a std over (C,H) for
// every column on its own, so columns are independent and the Form only says how they are laid over workgroups:
//   DdimScalarForm  one workgroup per sample, 256 / W parts of W columns (W <= 256), the guidance scale a launch argument;
//   DdimRowsForm    one workgroup per (sample, chunk of 16 columns), 16 parts: any W, ceil(W / 16) workgroups per sample and nothing
//                   exchanged between them. scales[b] is read here, from device memory: a captured launch replays with whatever the
//                   array then holds. scales[b] == 1 (or e_u NULL): the reference's unguided branch (ddim.py:170-171), e = e_c; e_u is
//                   not read and no statistic is computed.
//   R > 0   a thread's R rows of every operand are held in registers (one round of independent loads);
//   R == 0  the looped form: three passes over e_c / e_u.
//   DRAW    the step noise z of element e of sample b is drawn here: row first_id + b of stedm_philox_normal, stream 1 + iteration
//           (iteration = n_iters - 1 - *step_idx), instead of being read from `noise`;
//   EXT     the reference's temperature and noise dropout (ddim.py:206-208, each product rounded on its own: ((sigma z) T) keep / (1 - p)),
//           then x_prev = (sqrt(a_prev) x0 + dir) + noise; optional outputs of the guided eps and of that noise term.
// Contraction is off and every fusion is spelled out, so a result's bits do not depend on R, DRAW or EXT, nor on the compiler. They do
// depend on the Form, in the three expressions its k... constants name: each entry keeps the pairing it has always had.
// x_prev may alias x and eps_out may alias e_c, element for element (the samplers step in place): a thread reads its elements of every
// operand before it writes them and no other thread touches them, and none of the four is declared __restrict__.
// ------------------------------------------------------------------------------------------------
struct DdimEx {
  float* eps_out;            // guided eps after the rescale (ddim.py:184); may alias e_c element for element
  float* noise_out;          // the noise term that was added (EXT only)
  float temperature, drop_scale;
  uint32_t thr16, seed, id0;
  int n_iters;
  int drop;                  // noise_dropout > 0 (thr16 may still be 0 for p < 2^-17: then every element is kept, and scaled)
};

struct DdimScalarForm {
  static constexpr bool kExactR = true;          // R > 0: every thread owns exactly R rows (the host dispatches so), no guard
  static constexpr bool kFusedCombine = false;   // (e_w ratio) phi and (1 - phi) e_c both rounded, then the sum
  static constexpr bool kFusedDir = true;        // dir = sqrt(fma(-sigma, sigma, 1 - a_prev))
  static constexpr bool kSwap01 = true;          // R > 0: the squares of a thread's first two rows enter as fma(d0, d0, d1 d1)
  float s;
  __device__ int sample() const { return blockIdx.x; }
  __device__ int first_col() const { return 0; }
  __device__ int cols(int W) const { return W; }
  __device__ int parts(int W) const { return 256 / W; }
  __device__ bool owns(int w, int part, int W) const { return part < 256 / W; }       // 256 % W threads idle
  __device__ float scale(int b, const float* e_u, bool& guided) const {
    guided = e_u != nullptr;
    return s;
  }
};

struct DdimRowsForm {
  static constexpr int kChunk = 16;              // columns per workgroup: 16 fp32 = the 64-byte segment a quarter-wave reads from one row
  static constexpr bool kExactR = false;         // R = ceil(C H / 16): the last rows and the columns past W are guarded
  static constexpr bool kFusedCombine = true;    // fma(e_w ratio, phi, (1 - phi) e_c)
  static constexpr bool kFusedDir = false;       // dir = sqrt((1 - a_prev) - sigma sigma), the product rounded
  static constexpr bool kSwap01 = false;
  const float* scales;       // DEVICE [B]
  int nchunk;                // ceil(W / kChunk)
  __device__ int sample() const { return blockIdx.x / nchunk; }
  __device__ int first_col() const { return (blockIdx.x % nchunk) * kChunk; }
  __device__ int cols(int) const { return kChunk; }
  __device__ int parts(int) const { return 256 / kChunk; }
  __device__ bool owns(int w, int, int W) const { return w < W; }
  __device__ float scale(int b, const float* e_u, bool& guided) const {
    const float s = scales[b];
    guided = e_u != nullptr && s != 1.0f;          // uniform over the workgroup
    return s;
  }
};

__device__ __forceinline__ float ddim_ew(float ec, float eu, float s) {          // e_u + s (e_c - e_u)
#pragma clang fp contract(off)
  return __builtin_fmaf(s, ec - eu, eu);
}

template <bool FUSED>
__device__ __forceinline__ float ddim_guided(float ec, float eu, float s, float ratio, float phi) {
#pragma clang fp contract(off)
  const float rescaled = ddim_ew(ec, eu, s) * ratio, keep = (1.0f - phi) * ec;
  if constexpr (FUSED) return __builtin_fmaf(rescaled, phi, keep);
  else return rescaled * phi + keep;
}

__device__ __forceinline__ float ddim_shaped_noise(float xp, float sigma, float z, float temperature, float keep_scale) {
#pragma clang fp contract(off)       // every product and sum rounded on its own, as torch does (ddim.py:206-210)
  return xp + ((sigma * z) * temperature) * keep_scale;
}

// x_prev of element o (element e of sample b's row) from xp = sqrt(a_prev) x0 + dir; the noise, temperature and dropout of DRAW / EXT
template <bool DRAW, bool EXT>
__device__ __forceinline__ float ddim_add_noise(float xp, float sigma, const float* noise, float nzv, long o, int e, int b, float eg,
                                                const DdimEx& ex, int idx) {
  if constexpr (EXT) {
    if (ex.eps_out) ex.eps_out[o] = eg;
  }
  if (!(DRAW || noise)) return xp;
  const uint32_t iter = (uint32_t)(ex.n_iters - 1 - idx), sid = ex.id0 + (uint32_t)b;
  float z = nzv;
  if constexpr (DRAW) z = philox_normal1((uint32_t)e, 1u + iter, ex.seed, sid);
  if constexpr (!EXT) {
    return __builtin_fmaf(sigma, z, xp);
  } else {
    const float ks = !ex.drop ? 1.0f : ddim_drop_keep((uint32_t)e, iter, ex.seed, sid, ex.thr16) ? ex.drop_scale : 0.0f;
    const float out = ddim_shaped_noise(xp, sigma, z, ex.temperature, ks);
    if (ex.noise_out) ex.noise_out[o] = ddim_shaped_noise(0.0f, sigma, z, ex.temperature, ks);
    return out;
  }
}

// std_(c,h)(e_c) / std_(c,h)(e_w) of this thread's column (unbiased: torch.std's default, ddim.py:183). each(swap01, f) calls f(e_c, e_u)
// on the thread's rows in their order, the first two exchanged if swap01. Column totals: the parts' sums added in the order of part.
template <bool SWAP01, class Each>
__device__ __forceinline__ float ddim_rescale_ratio(const Each& each, float s, int CH, int parts, int cols, int col) {
#pragma clang fp contract(off)
  __shared__ float red[2][256];
  __shared__ float ratio_s[256];
  float sc = 0.f, sw = 0.f;
  each(false, [&](float ec, float eu) {
    sc += ec;
    sw += ddim_ew(ec, eu, s);
  });
  red[0][threadIdx.x] = sc;
  red[1][threadIdx.x] = sw;
  __syncthreads();
  float mc = 0.f, mw = 0.f;
  for (int p = 0; p < parts; ++p) {
    mc += red[0][p * cols + col];
    mw += red[1][p * cols + col];
  }
  mc /= (float)CH;
  mw /= (float)CH;
  __syncthreads();
  float qc = 0.f, qw = 0.f;
  each(SWAP01, [&](float ec, float eu) {
    const float dc = ec - mc, dw = ddim_ew(ec, eu, s) - mw;
    qc = __builtin_fmaf(dc, dc, qc);
    qw = __builtin_fmaf(dw, dw, qw);
  });
  red[0][threadIdx.x] = qc;
  red[1][threadIdx.x] = qw;
  __syncthreads();
  if (threadIdx.x < cols) {
    float vc = 0.f, vw = 0.f;
    for (int p = 0; p < parts; ++p) {
      vc += red[0][p * cols + threadIdx.x];
      vw += red[1][p * cols + threadIdx.x];
    }
    ratio_s[threadIdx.x] = sqrtf(vc / (float)(CH - 1)) / sqrtf(vw / (float)(CH - 1));
  }
  __syncthreads();
  return ratio_s[col];
}

template <class Form, int R, bool DRAW, bool EXT>
__global__ void __launch_bounds__(256) ddim_step_kernel(const float* x, const float* e_c, const float* __restrict__ e_u,
                                                        const float* __restrict__ noise, const float* __restrict__ coefs,
                                                        const int32_t* __restrict__ step_idx, float phi, float* x_prev,
                                                        float* __restrict__ pred_x0, int C, int H, int W, Form form, DdimEx ex) {
#pragma clang fp contract(off)
  const int cols = form.cols(W), parts = form.parts(W);
  const int col = threadIdx.x % cols, part = threadIdx.x / cols;
  const int b = form.sample(), w = form.first_col() + col;
  const bool mine = form.owns(w, part, W);
  const int idx = step_idx ? *step_idx : 0;
  const float a_t = coefs[idx * 4 + 0], a_prev = coefs[idx * 4 + 1], sigma = coefs[idx * 4 + 2], sq1m = coefs[idx * 4 + 3];
  const int CH = C * H;
  const long base = (long)b * CH * W;
  bool guided;
  const float s = form.scale(b, e_u, guided);
  const bool noisy = !DRAW && noise != nullptr;
  const float sqrt_at = sqrtf(a_t), sqrt_ap = sqrtf(a_prev);
  const float dir_c = sqrtf(Form::kFusedDir ? __builtin_fmaf(-sigma, sigma, 1.0f - a_prev) : 1.0f - a_prev - sigma * sigma);

  // x_prev / pred_x0 of row r of this thread's column from the operands' values there
  auto finish = [&](int r, float xv, float ec, float eu, float nzv, float ratio) {
    const long o = base + (long)r * W + w;
    const float e = guided ? ddim_guided<Form::kFusedCombine>(ec, eu, s, ratio, phi) : ec;
    const float x0 = __builtin_fmaf(-sq1m, e, xv) / sqrt_at;
    const float xp = ddim_add_noise<DRAW, EXT>(ddim_base_rounded(sqrt_ap, x0, dir_c, e), sigma, noise, nzv, o, r * W + w, b, e, ex, idx);
    x_prev[o] = xp;
    if (pred_x0) pred_x0[o] = x0;
  };

  if constexpr (R > 0) {
    float ec[R], xv[R], eu[R] = {}, nz[R];      // eu: passed to finish also when unguided, where it is not used
    bool ok[R];                                 // kept as an array: recomputed at each use, the masks cost 14 VGPRs and spilled SGPRs at R = 24
#pragma unroll
    for (int j = 0; j < R; ++j) ok[j] = Form::kExactR || (mine && part + j * parts < CH);
    auto at = [&](int j) { return base + (long)(part + j * parts) * W + w; };
#pragma unroll
    for (int j = 0; j < R; ++j) ec[j] = ok[j] ? e_c[at(j)] : 0.0f;
#pragma unroll
    for (int j = 0; j < R; ++j) xv[j] = ok[j] ? x[at(j)] : 0.0f;
    if (guided) {
#pragma unroll
      for (int j = 0; j < R; ++j) eu[j] = ok[j] ? e_u[at(j)] : 0.0f;
    }
    if (noisy) {
#pragma unroll
      for (int j = 0; j < R; ++j) nz[j] = ok[j] ? noise[at(j)] : 0.0f;
    }
    float ratio = 1.0f;
    if (guided)
      ratio = ddim_rescale_ratio<Form::kSwap01>([&](bool swap01, auto f) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
          const int k = swap01 && j < 2 ? 1 - j : j;
          if (ok[k]) f(ec[k], eu[k]);
        }
      }, s, CH, parts, cols, col);
#pragma unroll
    for (int j = 0; j < R; ++j)
      if (ok[j]) finish(part + j * parts, xv[j], ec[j], eu[j], noisy ? nz[j] : 0.0f, ratio);
  } else {
    float ratio = 1.0f;
    if (guided)
      ratio = ddim_rescale_ratio<false>([&](bool, auto f) {
        if (mine)
          for (int r = part; r < CH; r += parts) f(e_c[base + (long)r * W + w], e_u[base + (long)r * W + w]);
      }, s, CH, parts, cols, col);
    if (mine)
      for (int r = part; r < CH; r += parts) {
        const long o = base + (long)r * W + w;
        finish(r, x[o], e_c[o], guided ? e_u[o] : 0.0f, noisy ? noise[o] : 0.0f, ratio);
      }
  }
}

struct DdimOperands {      // host side: what the three entries hand to the launch
  const float *x, *e_c, *e_u, *noise, *coefs;
  const int32_t* step_idx;
  float phi;
  float *x_prev, *pred_x0;
  int C, H, W;
};

// launches the instantiation with R rows per thread; Rs lists the ones the entry's dispatch can select
template <class Form, bool DRAW, bool EXT, int... Rs>
static void launch_ddim_step(int R, unsigned grid, const Form& form, const DdimOperands& a, const DdimEx& ex, hipStream_t st) {
  auto go = [&](auto r) {
    ddim_step_kernel<Form, decltype(r)::value, DRAW, EXT><<<grid, 256, 0, st>>>(a.x, a.e_c, a.e_u, a.noise, a.coefs, a.step_idx, a.phi, a.x_prev,
                                                                                a.pred_x0, a.C, a.H, a.W, form, ex);
    return true;
  };
  (void)((R == Rs && go(std::integral_constant<int, Rs>{})) || ...);
}

// scalar entries: registers when the 256 threads tile the sample exactly with 16 (32 x 32 x 4, the bench's latents), 4 (16 x 16 x 4) or 8
// rows each, looped otherwise
template <bool DRAW, bool EXT>
static void launch_ddim_scalar(float s, int B, const DdimOperands& a, const DdimEx& ex, hipStream_t st) {
  const int parts = 256 / a.W, CH = a.C * a.H;
  const int per = 256 % a.W == 0 && CH % parts == 0 ? CH / parts : 0;
  launch_ddim_step<DdimScalarForm, DRAW, EXT, 0, 4, 8, 16>(per == 16 || per == 4 || per == 8 ? per : 0, (unsigned)B, DdimScalarForm{s}, a, ex, st);
}

// x_prev may alias x, element for element (and, in _ex, eps_out may alias e_c)
extern "C" int stedm_ddim_step(const float* x, const float* e_c, const float* e_u, const float* noise, const float* coefs,
                               const int32_t* step_idx, float cfg_scale, float rescale_phi, float* x_prev, float* pred_x0,
                               int B, int C, int H, int W, void* stream) {
  STEDM_CHECK_ARG(x && e_c && coefs && x_prev, "ddim_step: null pointer");
  STEDM_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && W <= 256, "ddim_step: bad shape B=%d C=%d H=%d W=%d (W <= 256)", B, C, H, W);
  STEDM_CHECK_ARG(!e_u || C * H > 1, "ddim_step: std over (C,H) needs C*H > 1");
  launch_ddim_scalar<false, false>(cfg_scale, B, {x, e_c, e_u, noise, coefs, step_idx, rescale_phi, x_prev, pred_x0, C, H, W}, DdimEx{},
                                   as_stream(stream));
  STEDM_LAUNCH_CHECK();
  return 0;
}

// x_prev may alias x and eps_out may alias e_c, element for element
extern "C" int stedm_ddim_step_ex(const float* x, const float* e_c, const float* e_u, const float* noise, const float* coefs,
                                  const int32_t* step_idx, int n_iters, float cfg_scale, float rescale_phi, int draw, float temperature,
                                  float noise_dropout, long first_id, unsigned long long seed, float* x_prev, float* pred_x0, float* eps_out,
                                  float* noise_out, int B, int C, int H, int W, void* stream) {
  STEDM_CHECK_ARG(x && e_c && coefs && x_prev, "ddim_step_ex: null pointer");
  STEDM_CHECK_ARG(B > 0 && B <= 65535 && C > 0 && H > 0 && W > 0 && W <= 256, "ddim_step_ex: bad shape B=%d C=%d H=%d W=%d (W <= 256)", B, C, H, W);
  STEDM_CHECK_ARG(!e_u || C * H > 1, "ddim_step_ex: std over (C,H) needs C*H > 1");
  STEDM_CHECK_ARG(!(draw && noise), "ddim_step_ex: a given noise tensor and the in-kernel draw exclude each other");
  STEDM_CHECK_ARG(noise_dropout >= 0.0f && noise_dropout < 1.0f, "ddim_step_ex: noise_dropout %g outside [0, 1)", (double)noise_dropout);
  const unsigned thr = (unsigned)lrint((double)noise_dropout * 65536.0);
  const bool drop = noise_dropout > 0.0f;
  STEDM_CHECK_ARG(!((draw || drop) && !step_idx), "ddim_step_ex: the in-kernel draw and the dropout need the device step index");
  STEDM_CHECK_ARG(!((draw || drop) && n_iters <= 0), "ddim_step_ex: the in-kernel draw and the dropout need n_iters > 0 (got %d)", n_iters);
  STEDM_CHECK_ARG(first_id >= 0 && first_id + B <= (1L << 32), "ddim_step_ex: sample ids %ld + %d outside [0, 2^32]", first_id, B);
  const DdimEx ex{eps_out, noise_out, temperature, (float)(1.0 / (1.0 - (double)noise_dropout)), thr, (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)first_id,
                 n_iters, drop ? 1 : 0};
  const DdimOperands a{x, e_c, e_u, noise, coefs, step_idx, rescale_phi, x_prev, pred_x0, C, H, W};
  const bool ext = temperature != 1.0f || drop || eps_out || noise_out;
  hipStream_t st = as_stream(stream);
  if (draw && ext) launch_ddim_scalar<true, true>(cfg_scale, B, a, ex, st);
  else if (draw) launch_ddim_scalar<true, false>(cfg_scale, B, a, ex, st);
  else if (ext) launch_ddim_scalar<false, true>(cfg_scale, B, a, ex, st);
  else launch_ddim_scalar<false, false>(cfg_scale, B, a, ex, st);
  STEDM_LAUNCH_CHECK();
  return 0;
}

// One guidance scale per sample (DdimRowsForm). x_prev may alias x, element for element.
template <bool DRAW>
static void launch_ddim_rows(const DdimRowsForm& form, int B, const DdimOperands& a, const DdimEx& ex, hipStream_t st) {
  const int per = (a.C * a.H + 15) / 16;      // a thread's rows
  // 2: 8 x 8 x 4 and smaller; 4: 16 x 16 x 4; 8: 32 x 32 x 4 (the bench's latents); 16: 64 x 64 x 4; 24: 128 x 128 x 3 (the reference's native latents)
  const int R = per <= 2 ? 2 : per <= 4 ? 4 : per <= 8 ? 8 : per <= 16 ? 16 : per <= 24 ? 24 : 0;
  launch_ddim_step<DdimRowsForm, DRAW, false, 0, 2, 4, 8, 16, 24>(R, (unsigned)((long)B * form.nchunk), form, a, ex, st);
}

extern "C" int stedm_ddim_step_rows(const float* x, const float* e_c, const float* e_u, const float* noise, const float* coefs,
                                    const int32_t* step_idx, int n_iters, const float* scales, float rescale_phi, int draw, long first_id,
                                    unsigned long long seed, float* x_prev, float* pred_x0, int B, int C, int H, int W, void* stream) {
  STEDM_CHECK_ARG(x && e_c && coefs && scales && x_prev, "ddim_step_rows: null pointer");
  STEDM_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0, "ddim_step_rows: bad shape B=%d C=%d H=%d W=%d", B, C, H, W);
  STEDM_CHECK_ARG((long)C * H * W <= 0x7FFFFFFFL, "ddim_step_rows: a sample of %d x %d x %d elements exceeds 2^31 - 1", C, H, W);
  STEDM_CHECK_ARG(!e_u || C * H > 1, "ddim_step_rows: std over (C,H) needs C*H > 1");
  STEDM_CHECK_ARG(!(draw && noise), "ddim_step_rows: a given noise tensor and the in-kernel draw exclude each other");
  STEDM_CHECK_ARG(!(draw && !step_idx), "ddim_step_rows: the in-kernel draw needs the device step index");
  STEDM_CHECK_ARG(!(draw && n_iters <= 0), "ddim_step_rows: the in-kernel draw needs n_iters > 0 (got %d)", n_iters);
  STEDM_CHECK_ARG(first_id >= 0 && first_id + B <= (1L << 32), "ddim_step_rows: sample ids %ld + %d outside [0, 2^32]", first_id, B);
  const int nchunk = (W + DdimRowsForm::kChunk - 1) / DdimRowsForm::kChunk;
  STEDM_CHECK_ARG((long)B * nchunk <= 0x7FFFFFFFL, "ddim_step_rows: %d samples of %d column chunks exceed one launch", B, nchunk);
  const DdimRowsForm form{scales, nchunk};
  const DdimEx ex{nullptr, nullptr, 1.0f, 1.0f, 0u, (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)first_id, n_iters, 0};
  const DdimOperands a{x, e_c, e_u, noise, coefs, step_idx, rescale_phi, x_prev, pred_x0, C, H, W};
  if (draw) launch_ddim_rows<true>(form, B, a, ex, as_stream(stream));
  else launch_ddim_rows<false>(form, B, a, ex, as_stream(stream));
  STEDM_LAUNCH_CHECK();
  return 0;
}

__global__ void step_advance_kernel(int32_t* p, int d) { *p += d; }
extern "C" int stedm_step_advance(int32_t* step_idx, int delta, void* stream) {
  STEDM_CHECK_ARG(step_idx, "step_advance: null pointer");
  step_advance_kernel<<<1, 1, 0, as_stream(stream)>>>(step_idx, delta);
  STEDM_LAUNCH_CHECK();
  return 0;
}

template <typename T>
__global__ void step_set_t_kernel(const T* __restrict__ ts, const int32_t* __restrict__ idx, T* __restrict__ t, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) t[i] = ts[*idx];
}
extern "C" int stedm_step_set_t(const int64_t* ts_table, const int32_t* step_idx, int64_t* t_buf, int B, void* stream) {
  STEDM_CHECK_ARG(ts_table && step_idx && t_buf && B > 0, "step_set_t: bad args");
  step_set_t_kernel<int64_t><<<(B + 255) / 256, 256, 0, as_stream(stream)>>>(ts_table, step_idx, t_buf, B);
  STEDM_LAUNCH_CHECK();
  return 0;
}
extern "C" int stedm_step_set_t_f32(const float* ts_table, const int32_t* step_idx, float* t_buf, int B, void* stream) {
  STEDM_CHECK_ARG(ts_table && step_idx && t_buf && B > 0, "step_set_t_f32: bad args");
  step_set_t_kernel<float><<<(B + 255) / 256, 256, 0, as_stream(stream)>>>(ts_table, step_idx, t_buf, B);
  STEDM_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// DPM-Solver++(2M) update (dpm_solver.py, predict_x0=True, solver_type 'dpm_solver'), elementwise over the flat [B*C*H*W] tensors:
//   eps = e_u + s (e_c - e_u)                              model_wrapper, classifier-free (dpm_solver.py:305-321); e_u NULL: eps = e_c
//   x0  = (x - sigma_i eps) / alpha_i                      data_prediction_fn (:361-368), thresholding off
//   x   = (r x - A x0) - (0.5 A) (inv_r0 (x0 - x0_prev))   multistep update: first order (:478-505) when the row's 0.5 A is 0,
//                                                          second order (:732-767) otherwise; x0_prev not read at first order
//   x0_prev = x0 (pred_x0 = x0 if given)
// The reference's operations in its order, each rounded once (contraction into FMAs is off): with equal inputs, torch's CPU arithmetic
// gives the same bits, in the float4 and the elementwise form alike. Row *step_idx of coefs [S][STEDM_DPM_NCOEF] = {alpha_i, sigma_i, r, A, inv_r0, 0.5 A (0: first order)}. One thread = four
// consecutive elements: float4 accesses when every pointer is 16-byte aligned, elementwise for the tail and otherwise. x, x0_prev and
// pred_x0 may alias one another element for element (each element is read before it is written).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float dpm_update1(float xv, float ec, float eu, float xp, bool cfg, float s, float alpha, float sigma, float r,
                                             float A, float inv_r0, float hA, float& x0) {
#pragma clang fp contract(off)       // every product and sum rounded on its own (HIP's default contracts them into FMAs across statements)
  const float eps = cfg ? eu + s * (ec - eu) : ec;
  x0 = (xv - sigma * eps) / alpha;     // IEEE division (HIP's default: correctly rounded fp32 divide)
  float o = r * xv - A * x0;
  if (hA != 0.0f) o = o - hA * (inv_r0 * (x0 - xp));
  return o;
}

template <bool VEC>
__global__ void __launch_bounds__(256) dpm_step_kernel(float* x, const float* __restrict__ e_c, const float* __restrict__ e_u, float* x0_prev,
                                                       float* pred_x0, const float* __restrict__ coefs, const int32_t* __restrict__ step_idx,
                                                       float s, long n) {
  const long e0 = 4 * ((long)blockIdx.x * 256 + threadIdx.x);
  if (e0 >= n) return;
  const float* row = coefs + (long)(step_idx ? *step_idx : 0) * STEDM_DPM_NCOEF;
  const float alpha = row[0], sigma = row[1], r = row[2], A = row[3], inv_r0 = row[4], hA = row[5];
  const bool cfg = e_u != nullptr;
  if (VEC && e0 + 4 <= n) {
    const float4 xv = *reinterpret_cast<const float4*>(x + e0), ec = *reinterpret_cast<const float4*>(e_c + e0);
    const float4 eu = cfg ? *reinterpret_cast<const float4*>(e_u + e0) : ec;
    const float4 xp = hA != 0.0f ? *reinterpret_cast<const float4*>(x0_prev + e0) : ec;
    float4 o, q;
    o.x = dpm_update1(xv.x, ec.x, eu.x, xp.x, cfg, s, alpha, sigma, r, A, inv_r0, hA, q.x);
    o.y = dpm_update1(xv.y, ec.y, eu.y, xp.y, cfg, s, alpha, sigma, r, A, inv_r0, hA, q.y);
    o.z = dpm_update1(xv.z, ec.z, eu.z, xp.z, cfg, s, alpha, sigma, r, A, inv_r0, hA, q.z);
    o.w = dpm_update1(xv.w, ec.w, eu.w, xp.w, cfg, s, alpha, sigma, r, A, inv_r0, hA, q.w);
    *reinterpret_cast<float4*>(x + e0) = o;
    *reinterpret_cast<float4*>(x0_prev + e0) = q;
    if (pred_x0) *reinterpret_cast<float4*>(pred_x0 + e0) = q;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long e = e0 + j;
      if (e < n) {
        const float ec = e_c[e];
        float q;
        const float o = dpm_update1(x[e], ec, cfg ? e_u[e] : ec, hA != 0.0f ? x0_prev[e] : ec, cfg, s, alpha, sigma, r, A, inv_r0, hA, q);
        x[e] = o;
        x0_prev[e] = q;
        if (pred_x0) pred_x0[e] = q;
      }
    }
  }
}

extern "C" int stedm_dpm_step(float* x, const float* e_c, const float* e_u, float* x0_prev, float* pred_x0, const float* coefs,
                              const int32_t* step_idx, float cfg_scale, long n, void* stream) {
  STEDM_CHECK_ARG(x && e_c && x0_prev && coefs, "dpm_step: null pointer");
  STEDM_CHECK_ARG(n > 0 && n <= (1L << 40), "dpm_step: bad element count %ld", n);
  const bool aligned = ((uintptr_t)x | (uintptr_t)e_c | (uintptr_t)e_u | (uintptr_t)x0_prev | (uintptr_t)pred_x0) % 16 == 0;
  const long groups = (n + 3) / 4;
  const long blocks = (groups + 255) / 256;
  STEDM_CHECK_ARG(blocks <= 0x7FFFFFFFL, "dpm_step: %ld elements exceed one launch", n);
  if (aligned)
    dpm_step_kernel<true><<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(x, e_c, e_u, x0_prev, pred_x0, coefs, step_idx, cfg_scale, n);
  else
    dpm_step_kernel<false><<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(x, e_c, e_u, x0_prev, pred_x0, coefs, step_idx, cfg_scale, n);
  STEDM_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------
// PLMS update (plms.py:173-239, ddim_eta = 0), elementwise over the flat [B*C*H*W] tensors:
//   e   = e_u + s (e_c - e_u)                              get_model_output (plms.py:178-192; no std rescale); e_u NULL: e = e_c
//   e'  = phase EULER: e (and ring[0] = e)                 pseudo improved Euler, first half (:219-221)
//         phase HEUN:  (ring[0] + e) / 2                   second half, e = the model at (x_tmp, t_next) (:222-223)
//         phase MULTISTEP, i = n_iters - 1 - *step_idx, order min(i, 3), e_{i-j} in ring slot (i - j) mod 4, ring[i mod 4] = e:
//           (3 e - e1) / 2,  (23 e - 16 e1 + 5 e2) / 12,  (55 e - 59 e1 + 37 e2 - 9 e3) / 24   (:224-232; order 0: e' = e)
//   x0  = (x - sqrt(1 - a_t) e') / sqrt(a_t);  x_prev = sqrt(a_prev) x0 + sqrt(1 - a_prev) e'   get_x_prev_and_pred_x0 (:199-216), sigma 0
// EULER writes x_prev to x_tmp and leaves x alone; HEUN and MULTISTEP write it to x (pred_x0 = x0 if given). The reference's operations
// in its order, each rounded once (no FMA contraction, true divisions), so with equal inputs torch's CPU arithmetic gives the same bits.
// Row *step_idx of the DDIM table coefs [n_iters][4] = {a_t, a_prev, sigma (0), sqrt(1 - a_t)}. One thread = four consecutive elements:
// float4 accesses when every pointer (the ring's slots included) is 16-byte aligned, elementwise for the tail and otherwise. pred_x0 and
// x_tmp may alias e_c / e_u element for element (each element is read before it is written).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float plms_update1(float xv, float ec, float eu, float r0, float r1, float r2, bool cfg, float s, int phase,
                                              int order, float sqrt_at, float sq1m, float sqrt_ap, float dir_c, float& e, float& x0) {
#pragma clang fp contract(off)       // every product and sum rounded on its own (HIP's default contracts them into FMAs across statements)
  e = cfg ? eu + s * (ec - eu) : ec;
  float ep = e;
  if (phase == STEDM_PLMS_HEUN) {
    ep = (r0 + e) / 2.0f;
  } else if (phase == STEDM_PLMS_MULTISTEP) {
    if (order == 1) ep = (3.0f * e - r0) / 2.0f;
    else if (order == 2) ep = (23.0f * e - 16.0f * r0 + 5.0f * r1) / 12.0f;
    else if (order >= 3) ep = (55.0f * e - 59.0f * r0 + 37.0f * r1 - 9.0f * r2) / 24.0f;
  }
  x0 = (xv - sq1m * ep) / sqrt_at;     // IEEE division (HIP's default: correctly rounded fp32 divide)
  return sqrt_ap * x0 + dir_c * ep;
}

template <bool VEC>
__global__ void __launch_bounds__(256) plms_step_kernel(float* x, const float* e_c, const float* e_u, float* ring, const float* __restrict__ coefs,
                                                        const int32_t* __restrict__ step_idx, int n_iters, int phase, float s, float* pred_x0,
                                                        float* x_tmp, long n) {
  const long e0 = 4 * ((long)blockIdx.x * 256 + threadIdx.x);
  if (e0 >= n) return;
  const int index = *step_idx;
  const float* row = coefs + (long)index * 4;
  const float a_t = row[0], a_prev = row[1], sq1m = row[3];
  const float sqrt_at = sqrtf(a_t), sqrt_ap = sqrtf(a_prev), dir_c = sqrtf(1.0f - a_prev);
  const int i = phase == STEDM_PLMS_MULTISTEP ? n_iters - 1 - index : 0;
  const int order = i < 0 ? 0 : (i > 3 ? 3 : i);
  // slots read: HEUN the e_t of EULER (slot 0); MULTISTEP e_{i-1}, e_{i-2}, e_{i-3}. Slot written: EULER 0, MULTISTEP i mod 4.
  const float* r0p = ring + (phase == STEDM_PLMS_HEUN ? 0L : (long)((i - 1) & 3) * n);
  const float* r1p = ring + (long)((i - 2) & 3) * n;
  const float* r2p = ring + (long)((i - 3) & 3) * n;
  float* wp = ring + (long)(i & 3) * n;
  const bool cfg = e_u != nullptr;
  const bool rd0 = phase == STEDM_PLMS_HEUN || (phase == STEDM_PLMS_MULTISTEP && order >= 1);
  const bool rd1 = phase == STEDM_PLMS_MULTISTEP && order >= 2, rd2 = phase == STEDM_PLMS_MULTISTEP && order >= 3;
  const bool wr = phase != STEDM_PLMS_HEUN;
  float* out = phase == STEDM_PLMS_EULER ? x_tmp : x;
  float* px = phase == STEDM_PLMS_EULER ? nullptr : pred_x0;
  float xv[4], ec[4], eu[4], r0[4], r1[4], r2[4], o[4], et[4], q[4];
  const bool full = VEC && e0 + 4 <= n;
  const int cnt = full ? 4 : (int)(n - e0 < 4 ? n - e0 : 4);
  auto ld = [&](const float* p, bool use, float (&v)[4]) {
    if (!use) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = 0.0f;
    } else if (full) {
      const float4 t = *reinterpret_cast<const float4*>(p + e0);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = j < cnt ? p[e0 + j] : 0.0f;
    }
  };
  auto st = [&](float* p, const float (&v)[4]) {
    if (full) {
      *reinterpret_cast<float4*>(p + e0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < cnt) p[e0 + j] = v[j];
    }
  };
  ld(x, true, xv);
  ld(e_c, true, ec);
  ld(e_u, cfg, eu);
  ld(r0p, rd0, r0);
  ld(r1p, rd1, r1);
  ld(r2p, rd2, r2);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    o[j] = plms_update1(xv[j], ec[j], eu[j], r0[j], r1[j], r2[j], cfg, s, phase, order, sqrt_at, sq1m, sqrt_ap, dir_c, et[j], q[j]);
  if (wr) st(wp, et);
  st(out, o);
  if (px) st(px, q);
}

extern "C" int stedm_plms_step(float* x, const float* e_c, const float* e_u, float* ring, const float* coefs, const int32_t* step_idx,
                               int n_iters, int phase, float cfg_scale, float* pred_x0, float* x_tmp, long n, void* stream) {
  STEDM_CHECK_ARG(x && e_c && ring && coefs && step_idx, "plms_step: null pointer");
  STEDM_CHECK_ARG(phase == STEDM_PLMS_EULER || phase == STEDM_PLMS_HEUN || phase == STEDM_PLMS_MULTISTEP, "plms_step: bad phase %d", phase);
  STEDM_CHECK_ARG(phase != STEDM_PLMS_EULER || x_tmp, "plms_step: the Euler phase needs x_tmp");
  STEDM_CHECK_ARG(n_iters > 0, "plms_step: bad iteration count %d", n_iters);
  STEDM_CHECK_ARG(n > 0 && n <= (1L << 40), "plms_step: bad element count %ld", n);
  const bool aligned = n % 4 == 0 &&
                       ((uintptr_t)x | (uintptr_t)e_c | (uintptr_t)e_u | (uintptr_t)ring | (uintptr_t)pred_x0 | (uintptr_t)x_tmp) % 16 == 0;
  const long groups = (n + 3) / 4;
  const long blocks = (groups + 255) / 256;
  STEDM_CHECK_ARG(blocks <= 0x7FFFFFFFL, "plms_step: %ld elements exceed one launch", n);
  if (aligned)
    plms_step_kernel<true><<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(x, e_c, e_u, ring, coefs, step_idx, n_iters, phase, cfg_scale,
                                                                            pred_x0, x_tmp, n);
  else
    plms_step_kernel<false><<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(x, e_c, e_u, ring, coefs, step_idx, n_iters, phase, cfg_scale,
                                                                             pred_x0, x_tmp, n);
  STEDM_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------ per-sample normal noise
// x_T (ddim.py:122) and the per-step noise of eta > 0 (ddim.py:206) for a rank's shard of a data-parallel prediction run: row i depends only
// on (seed, stream, global sample id), so a sample is the same under any world size (the reference draws batch-shaped from the global
// generator, which cannot give that). Definition (the parity tests restate it in numpy): group g of four consecutive elements of a
// row = Philox4x32-10(counter {g, stream, 0x4E524D4C, 0}, key {seed, sample id}); words (w0, w1) and (w2, w3) give two Box-Muller pairs with
// u = (w + 0.5) 2^-32: z0 = sqrt(-2 ln u0) cos(2 pi u1), z1 = sqrt(-2 ln u0) sin(2 pi u1). fp32 arithmetic with the hardware log / sin / cos.
__global__ void __launch_bounds__(256) philox_normal_kernel(float* __restrict__ out, const long* __restrict__ ids, int id0, int n, unsigned seed, unsigned stream) {
  const int row = blockIdx.y;
  const unsigned sid = ids ? (unsigned)ids[row] : (unsigned)(id0 + row);
  const int ngroups = (n + 3) >> 2;
  for (int g = blockIdx.x * 256 + threadIdx.x; g < ngroups; g += gridDim.x * 256) {
    float z[4];
    philox_normal4((unsigned)g, stream, seed, sid, z);
    float* o = out + (long)row * n + 4 * g;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * g + j < n) o[j] = z[j];
  }
}

extern "C" int stedm_philox_normal(float* out, int rows, int n, const long* sample_ids, int first_id, unsigned long long seed, unsigned stream, void* stream_) {
  STEDM_CHECK_ARG(out && rows > 0 && n > 0, "philox_normal: bad arguments");
  const int ngroups = (n + 3) / 4;
  dim3 grid((ngroups + 255) / 256 < 64 ? (ngroups + 255) / 256 : 64, rows);
  philox_normal_kernel<<<grid, 256, 0, as_stream(stream_)>>>(out, sample_ids, first_id, n, (unsigned)(seed & 0xFFFFFFFFull), stream);
  STEDM_LAUNCH_CHECK();
  return 0;
}


// ------------------------------------------------------------------------------------------------ row groups of a [B][C][HW] operand
// The thread mapping of the mask blend and the ancestral DDPM step: grid (ceil(C HW / 4 / 256), B), one thread = group g of four
// consecutive elements of sample b's row (the group of philox_normal4). VEC - HW % 4 == 0 and every operand 16-byte aligned
// (row_groups_check) - is the float4 form: a group lies in one channel plane. Otherwise the scalar tail form: any HW, a group may straddle
// planes or the row end; elements past the end load as 0 and are not stored. The mask is read through (batch, channel) strides, 0
// broadcasting.
template <bool VEC>
struct RowGroup {
  int b, g, n, HW;
  __device__ __forceinline__ RowGroup(int C, int HW_) : b(blockIdx.y), g(blockIdx.x * 256 + threadIdx.x), n(C * HW_), HW(HW_) {}
  __device__ __forceinline__ bool past_end() const { return 4 * g >= n; }
  __device__ __forceinline__ void load(const float* p, float (&v)[4]) const {
    p += (long)b * n + 4 * g;
    if (VEC) {
      const float4 q = *reinterpret_cast<const float4*>(p);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = 4 * g + j < n ? p[j] : 0.0f;
    }
  }
  __device__ __forceinline__ void load_mask(const float* mask, long mbs, long mcs, float (&m)[4]) const {
    if (VEC) {
      const int c = (4 * g) / HW, p = 4 * g - c * HW;
      const float4 w = *reinterpret_cast<const float4*>(mask + b * mbs + c * mcs + p);
      m[0] = w.x; m[1] = w.y; m[2] = w.z; m[3] = w.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = 4 * g + j;
        const bool in = e < n;
        const int c = in ? e / HW : 0, p = in ? e - c * HW : 0;
        m[j] = in ? mask[b * mbs + c * mcs + p] : 0.0f;
      }
    }
  }
  __device__ __forceinline__ void store(float* p, const float (&v)[4]) const {
    p += (long)b * n + 4 * g;
    if (VEC) {
      *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * g + j < n) p[j] = v[j];
    }
  }
};

// q_sample(x0) m + (1 - m) o (ddim.py:143-146, ddpm.py:1207-1209), one product of each sum rounded and the other fused into the sum:
// torch's unfused blend to an ulp, and o exactly where the mask is 0. These are the FMAs HIP's default contraction made of the float4
// form's two sums; they are spelled out because it fused the scalar form's sums element by element, some not at all, so that the bits
// of a blend depended on the operands' alignment.
__device__ __forceinline__ float ddpm_blend1(float o, float x0, float z, float m, float ca, float cn) {
#pragma clang fp contract(off)
  const float q = __builtin_fmaf(ca, x0, cn * z);
  return __builtin_fmaf(1.0f - m, o, q * m);
}

// The host checks of the entries that launch over row groups (`who` names the entry in the message; mask NULL: no strides to check),
// their grid, and the float4 form's condition on the addresses of every operand read or written in groups.
struct RowLaunch {
  dim3 grid;
  bool vec;
};
static int row_groups_check(const char* who, int B, int C, int HW, long first_id, const float* mask, long mbs, long mcs,
                            std::initializer_list<const void*> operands, RowLaunch* rl) {
  STEDM_CHECK_ARG(B > 0 && B <= 65535 && C > 0 && HW > 0 && (long)C * HW <= 0x7FFFFFFFL, "%s: bad shape B=%d C=%d HW=%d", who, B, C, HW);
  STEDM_CHECK_ARG(first_id >= 0 && first_id + B <= (1L << 32), "%s: sample ids %ld + %d outside [0, 2^32]", who, first_id, B);
  STEDM_CHECK_ARG(!mask || mcs == 0 || mcs == HW, "%s: mask channel stride %ld (0 or HW=%d)", who, mcs, HW);
  STEDM_CHECK_ARG(!mask || mbs == 0 || mbs == (mcs ? (long)C * HW : (long)HW), "%s: mask batch stride %ld (0 or the mask's per-sample size)",
                  who, mbs);
  uintptr_t bits = (uintptr_t)mask;
  for (const void* p : operands) bits |= (uintptr_t)p;
  rl->grid = dim3((unsigned)((((long)C * HW + 3) / 4 + 255) / 256), B);
  rl->vec = HW % 4 == 0 && bits % 16 == 0;
  return 0;
}

// ------------------------------------------------------------------------------------------------ masked DDIM: known region from x0
// ddim.py:143-146 before the U-Net call of every step: img = q_sample(x0, ts) * mask + (1 - mask) * img, q_sample = ddpm.py:277-280 with the
// fp32 schedule buffers gathered by t[b] (extract_into_tensor, util.py:96-99) and fresh noise each step. In place on img [B][C][HW], by row
// groups. noise: given ([B][C][HW]), or drawn here as stedm_philox_normal's row of sample first_id + b with stream 0x8000 + *step_idx -
// bit-identical to that kernel - so that a replayed graph draws new noise at every step.
template <bool VEC>
__global__ void __launch_bounds__(256) ddim_mask_blend_kernel(float* __restrict__ img, const float* __restrict__ x0, const float* __restrict__ mask,
                                                              long mbs, long mcs, const float* __restrict__ noise, const int64_t* __restrict__ t,
                                                              const float* __restrict__ sa, const float* __restrict__ s1, const int32_t* __restrict__ step_idx,
                                                              int C, int HW, unsigned id0, unsigned seed) {
  const RowGroup<VEC> r(C, HW);
  if (r.past_end()) return;
  const int64_t tb = t[r.b];
  const float ca = sa[tb], cn = s1[tb];
  float z[4], xi[4], x0v[4], m[4], o[4];
  if (noise) r.load(noise, z);
  else philox_normal4((unsigned)r.g, 0x8000u + (unsigned)*step_idx, seed, id0 + (unsigned)r.b, z);
  r.load(img, xi);
  r.load(x0, x0v);
  r.load_mask(mask, mbs, mcs, m);
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = ddpm_blend1(xi[j], x0v[j], z[j], m[j], ca, cn);
  r.store(img, o);
}

extern "C" int stedm_ddim_mask_blend(float* img, const float* x0, const float* mask, long mask_bstride, long mask_cstride, const float* noise,
                                     const int64_t* t, const float* sqrt_ac, const float* sqrt_1mac, const int32_t* step_idx, int B, int C, int HW,
                                     long first_id, unsigned long long seed, void* stream) {
  STEDM_CHECK_ARG(img && x0 && mask && t && sqrt_ac && sqrt_1mac, "ddim_mask_blend: null pointer");
  STEDM_CHECK_ARG(noise || step_idx, "ddim_mask_blend: the in-kernel noise draw needs the device step index");
  RowLaunch rl;
  if (const int rc = row_groups_check("ddim_mask_blend", B, C, HW, first_id, mask, mask_bstride, mask_cstride, {img, x0, noise}, &rl)) return rc;
  if (rl.vec)
    ddim_mask_blend_kernel<true><<<rl.grid, 256, 0, as_stream(stream)>>>(img, x0, mask, mask_bstride, mask_cstride, noise, t, sqrt_ac, sqrt_1mac,
                                                                           step_idx, C, HW, (unsigned)first_id, (unsigned)(seed & 0xFFFFFFFFull));
  else
    ddim_mask_blend_kernel<false><<<rl.grid, 256, 0, as_stream(stream)>>>(img, x0, mask, mask_bstride, mask_cstride, noise, t, sqrt_ac, sqrt_1mac,
                                                                            step_idx, C, HW, (unsigned)first_id, (unsigned)(seed & 0xFFFFFFFFull));
  STEDM_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------ ancestral DDPM step
// One iteration of the reference's p_sample_loop (ddpm.py:1169-1217) after the model call, with the options of p_sample / p_mean_variance
// (:1050-1110), on x [B][C][HW] by row groups; t = *step_idx, or tv[b] (one table row per sample):
//   x0   = sr[t] x - srm1[t] eps                          predict_start_from_noise (ddpm.py:219-223)
//   x0   = clamp(x0, -1, 1) when clip                     p_mean_variance (:1069-1070)
//          QUANT: read from x0_out, where the pre-pass (ddpm_quantize_x0_launch, vq.hip) left the nearest codebook rows
//   mean = c1[t] x0 + c2[t] x                             q_posterior (:225-232)
//   n    = ((z temperature[t]) keep) / (1 - p)            p_sample (:1099-1101)
//   x'   = mean + sigma[t] n                              (:1107-1110); sigma = nonzero(t) exp(0.5 logvar_clipped[t]), from the table
//   mask (optional): x' = (sqrt_ac[t] x0m + sqrt_1mac[t] z') m + (1 - m) x'    the blend after the step (:1207-1209)
// table: [T][5] rows {sr, srm1, c1, c2, sigma}. z: given ([B][C][HW]) or stedm_philox_normal's row of sample first_id + b with stream
// 0x10000 + t; z': given, or the row with stream 0x8000 + t and mask_seed - what stedm_ddim_mask_blend draws for that index. The keep bits
// of a thread's four elements 4 g .. 4 g + 3 are fields 4 (g & 1) + j of one Philox block (counter {g >> 1, 0x20000 + t, "DROP", 0}:
// ddim_drop_keep's rule with t for the iteration). The step (ddpm_math.hpp) rounds every product and sum on its own, so with equal inputs
// torch's CPU arithmetic gives the same bits - temperature 1 and keep 1 multiply exactly. The blend is ddim_mask_blend_kernel's function,
// so the fused blend equals the step followed by stedm_ddim_mask_blend bit for bit. Optional outputs: x0_out (after clamp and
// quantisation), mean_out, x_out (NULL: the sample is not written; may be x). A t outside [0, T) writes nothing. stedm_ddpm_step is this
// kernel with the options off and x_out = x.
struct DdpmEx {
  const int64_t* tv;
  const float* temperature;  // [T] indexed by t; NULL: 1
  float drop_scale;          // (float)(1 / (1 - p))
  uint32_t thr16;
  int drop;                  // p > 0 (thr16 may still be 0: every element kept, and scaled)
  float* x_out;
  float* x0_out;
  float* mean_out;
};

template <bool VEC, bool MASK, bool QUANT>
__global__ void __launch_bounds__(256) ddpm_step_kernel(const float* x, const float* __restrict__ eps, const float* __restrict__ table,
                                                        const int32_t* __restrict__ step_idx, int T, int clip, const float* __restrict__ noise,
                                                        const float* __restrict__ mask, long mbs, long mcs, const float* __restrict__ x0m,
                                                        const float* __restrict__ mnoise, const float* __restrict__ sa, const float* __restrict__ s1,
                                                        int C, int HW, unsigned id0, unsigned seed, unsigned mseed, DdpmEx ex) {
  const RowGroup<VEC> r(C, HW);
  if (r.past_end()) return;
  const int b = r.b, g = r.g;
  const long long tl = ex.tv ? (long long)ex.tv[b] : (long long)*step_idx;
  if (tl < 0 || tl >= T) return;
  const int t = (int)tl;
  const float* row = table + (long)t * 5;
  const float sr = row[0], srm1 = row[1], c1 = row[2], c2 = row[3], sig = row[4];
  const float temp = ex.temperature ? ex.temperature[t] : 1.0f;
  float xv[4], q[4], z[4], mean[4], o[4];
  r.load(x, xv);
  if (QUANT) {
    r.load(ex.x0_out, q);
  } else {
    float ev[4];
    r.load(eps, ev);
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = ddpm_predict_x0(xv[j], ev[j], sr, srm1, clip != 0);
    if (ex.x0_out) r.store(ex.x0_out, q);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) mean[j] = ddpm_posterior_mean(q[j], xv[j], c1, c2);
  if (ex.mean_out) r.store(ex.mean_out, mean);
  if (!ex.x_out) return;
  if (noise) r.load(noise, z);
  else philox_normal4((unsigned)g, 0x10000u + (unsigned)t, seed, id0 + (unsigned)b, z);
  float ks[4] = {1.0f, 1.0f, 1.0f, 1.0f};
  if (ex.drop) {
    const U4 kb = philox4x32_10(U4{(uint32_t)g >> 1, 0x20000u + (uint32_t)t, DDIM_DROP_WORD, 0u}, seed, id0 + (unsigned)b);
#pragma unroll
    for (int j = 0; j < 4; ++j) ks[j] = drop_u16(kb, 4 * (g & 1) + j) >= ex.thr16 ? ex.drop_scale : 0.0f;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = ddpm_add_noise(mean[j], sig, ddpm_shaped_noise(z[j], temp, ks[j]));
  if (MASK) {
    const float ca = sa[t], cn = s1[t];
    float xk[4], m[4], zb[4];
    r.load(x0m, xk);
    if (mnoise) r.load(mnoise, zb);
    else philox_normal4((unsigned)g, 0x8000u + (unsigned)t, mseed, id0 + (unsigned)b, zb);
    r.load_mask(mask, mbs, mcs, m);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = ddpm_blend1(o[j], xk[j], zb[j], m[j], ca, cn);
  }
  r.store(ex.x_out, o);
}

// Both entries' checks and launches (`who` names the entry in the messages).
static int ddpm_step_launch(const char* who, const float* x, const float* eps, const float* table, const int32_t* step_idx, const int64_t* t,
                            int T, int clip, const float* noise, const float* temperature, float noise_dropout, const float* codebook, int n_e,
                            const float* mask, long mask_bstride, long mask_cstride, const float* x0, const float* mask_noise,
                            const float* sqrt_ac, const float* sqrt_1mac, float* x_out, float* x0_out, float* mean_out, long long* idx_out,
                            int B, int C, int HW, long first_id, unsigned long long seed, unsigned long long mask_seed, void* stream) {
  STEDM_CHECK_ARG(x && eps && table, "%s: null pointer", who);
  STEDM_CHECK_ARG((step_idx != nullptr) != (t != nullptr), "%s: give the device step index or the per-sample t, not both", who);
  STEDM_CHECK_ARG(T > 0, "%s: bad table length %d", who, T);
  STEDM_CHECK_ARG(noise_dropout >= 0.0f && noise_dropout < 1.0f, "%s: noise_dropout %g outside [0, 1)", who, (double)noise_dropout);
  STEDM_CHECK_ARG(x_out || x0_out || mean_out || (codebook && idx_out), "%s: no output", who);
  const bool quant = codebook != nullptr;
  STEDM_CHECK_ARG(quant || !idx_out, "%s: idx_out without a codebook", who);
  STEDM_CHECK_ARG(!quant || (x0_out && x0_out != x && x0_out != eps),
                  "%s: with a codebook x0_out is required (the quantised x0 passes through it) and may alias neither x nor eps", who);
  const bool masked = mask != nullptr;
  STEDM_CHECK_ARG(!masked || (x0 && sqrt_ac && sqrt_1mac), "%s: the mask blend needs x0, sqrt_ac and sqrt_1mac", who);
  RowLaunch rl;
  if (const int rc = row_groups_check(who, B, C, HW, first_id, mask, mask_bstride, mask_cstride,
                                      {x, eps, noise, x0, mask_noise, x_out, x0_out, mean_out}, &rl))
    return rc;
  hipStream_t st = as_stream(stream);
  if (quant) {
    const int rc = ddpm_quantize_x0_launch(x, eps, table, step_idx, t, T, clip, codebook, n_e, C, B, (long)HW, x0_out, idx_out, st);
    if (rc) return rc;
  }
  const unsigned id0 = (unsigned)first_id, sd = (unsigned)(seed & 0xFFFFFFFFull), msd = (unsigned)(mask_seed & 0xFFFFFFFFull);
  const bool drop = noise_dropout > 0.0f;
  const DdpmEx ex{t, temperature, (float)(1.0 / (1.0 - (double)noise_dropout)), (uint32_t)lrint((double)noise_dropout * 65536.0), drop ? 1 : 0,
                  x_out, x0_out, mean_out};
#define STEDM_DDPM_LAUNCH(V, M, Q)                                                                                                       \
  ddpm_step_kernel<V, M, Q><<<rl.grid, 256, 0, st>>>(x, eps, table, step_idx, T, clip, noise, mask, mask_bstride, mask_cstride, x0,       \
                                                     mask_noise, sqrt_ac, sqrt_1mac, C, HW, id0, sd, msd, ex)
#define STEDM_DDPM_VM(Q)                                  \
  if (rl.vec && masked) STEDM_DDPM_LAUNCH(true, true, Q);   \
  else if (rl.vec) STEDM_DDPM_LAUNCH(true, false, Q);       \
  else if (masked) STEDM_DDPM_LAUNCH(false, true, Q);       \
  else STEDM_DDPM_LAUNCH(false, false, Q)
  if (quant) { STEDM_DDPM_VM(true); }
  else { STEDM_DDPM_VM(false); }
#undef STEDM_DDPM_VM
#undef STEDM_DDPM_LAUNCH
  STEDM_LAUNCH_CHECK();
  return 0;
}

extern "C" int stedm_ddpm_step(float* x, const float* eps, const float* table, const int32_t* step_idx, int T, int clip, const float* noise,
                               const float* mask, long mask_bstride, long mask_cstride, const float* x0, const float* mask_noise,
                               const float* sqrt_ac, const float* sqrt_1mac, int B, int C, int HW, long first_id, unsigned long long seed,
                               unsigned long long mask_seed, void* stream) {
  STEDM_CHECK_ARG(x && eps && table && step_idx, "ddpm_step: null pointer");
  return ddpm_step_launch("ddpm_step", x, eps, table, step_idx, nullptr, T, clip, noise, nullptr, 0.0f, nullptr, 0, mask, mask_bstride,
                          mask_cstride, x0, mask_noise, sqrt_ac, sqrt_1mac, x, nullptr, nullptr, nullptr, B, C, HW, first_id, seed, mask_seed,
                          stream);
}

extern "C" int stedm_ddpm_step_ex(const float* x, const float* eps, const float* table, const int32_t* step_idx, const int64_t* t, int T, int clip,
                                  const float* noise, const float* temperature, float noise_dropout, const float* codebook, int n_e,
                                  const float* mask, long mask_bstride, long mask_cstride, const float* x0, const float* mask_noise,
                                  const float* sqrt_ac, const float* sqrt_1mac, float* x_out, float* x0_out, float* mean_out, long long* idx_out,
                                  int B, int C, int HW, long first_id, unsigned long long seed, unsigned long long mask_seed, void* stream) {
  return ddpm_step_launch("ddpm_step_ex", x, eps, table, step_idx, t, T, clip, noise, temperature, noise_dropout, codebook, n_e, mask,
                          mask_bstride, mask_cstride, x0, mask_noise, sqrt_ac, sqrt_1mac, x_out, x0_out, mean_out, idx_out, B, C, HW, first_id,
                          seed, mask_seed, stream);
}
