// v3c: 3x3 implicit-GEMM convolution with the weights streamed to REGISTERS and a continuous fragment pipeline.
//
// Measured on v3b (conv_igemm_dma9.inc): with the weight tiles in LDS, fragment reads (32 KB per tap and CU at 8 waves of
// 64 x 64) plus the DMA writes saturate the 128 B/clk LDS, which caps the loop near 45 % of the MFMA peak. Here
//  * the weights never touch LDS: they are packed once in exact MFMA B-fragment order (stedm_pack_conv_weight_frag: one
//    wave-wide 16-B load = one fragment, 1 KiB contiguous, consecutive taps / chunks consecutive in memory) and every compute
//    wave streams its own fragments with global_load_dwordx4 three taps ahead. Read-only global memory needs no hand-off, so
//    the stream runs across chunk boundaries; waves that share a fragment hit the same lines in L1;
//  * LDS holds only the activation patch: 4 buffers of NP x 32 B, DMA'd by two loader waves up to three chunks ahead. The
//    single block barrier per chunk sits at tap 6, not at the chunk end: after it the next chunk's patch is known to have
//    landed, so the A-fragment reads of taps 7/8 already prefetch the next chunk and the MFMA pipe never drains;
//  * WM = 32-row fragments per compute wave: 2 -> 8 compute waves of 64 x 64; 4 -> 4 compute waves of 128 x 64 (one per SIMD),
//    which halves the weight traffic per MFMA: per tap and CU 16 KB of patch reads (LDS) and 8 KB of weight loads (vector
//    memory) against 256 MFMA cycles per SIMD;
//  * epilogue: the whole 256 x 128 fp32 tile is staged in LDS (the patch buffers are dead by then) and ALL waves, loaders
//    included, write it out as full 512-B rows, 16 B per lane, with bias / emb / residual applied in that phase.
#pragma once
#include <type_traits>

#include "conv_igemm_dma.inc"
#include "gn_fold.hpp"

// timing experiments only (STEDM_CONV_DBG & 1024): per-block phase stamps of the constant 100 MHz clock (tools/conv_phases.py)
static __device__ unsigned long long g_conv_stamps[2048 * 8];
#define STAMP(K) if (STEDM_DBG(p.dbg, 1024) && tid == 0 && blockIdx.x < 2048) g_conv_stamps[blockIdx.x * 8 + (K)] = wall_clock64()
// shader-clock stamp (s_memtime) beside a wall-clock one: (delta s_memtime) / (delta s_memrealtime) x 100 MHz is the clock the chip holds
// INSIDE the main loop (MI355X_MICROARCH.md, DVFS give-back item 6); slots 2 (loop start) and 7 (loop end)
#define STAMPC(K) if (STEDM_DBG(p.dbg, 1024) && tid == 0 && blockIdx.x < 2048) g_conv_stamps[blockIdx.x * 8 + (K)] = __builtin_amdgcn_s_memtime()

// Diagnostic builds only (-DSTEDM_CONV_DIAG=<bits>, tools/conv_diag.sh: extra libraries, never the shipped one): COMPILE-TIME removal of one
// ingredient of the 16x16x32 main loop at a time — 8: no A-fragment LDS reads, 16: no weight-fragment loads, 32: no chunk barrier (both sides) —
// to attribute the loop's non-MFMA cycles (in-loop stamps of tools/conv_phases.py). Results are garbage; the shipped build compiles none of it.
// (Run-time switches were tried first: the branches around the loads cost the compiler its exact vmcnt / lgkmcnt counts and the loop ran 6x slower.)
#ifdef STEDM_CONV_DIAG
#define RS_DIAG(BIT) ((STEDM_CONV_DIAG) & (BIT))
#else
#define RS_DIAG(BIT) 0
#endif

// value of lane ^ 1 (DPP quad_perm [1, 0, 3, 2]): pairs two lanes' 16-bit results into one dword store (N-persistent epilogue)
__device__ __forceinline__ float rs_lane_xor1(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
}
template <typename T>
__device__ __forceinline__ unsigned rs_pack2(float lo, float hi) {
  typedef T V2T __attribute__((ext_vector_type(2)));
  V2T v; v[0] = (T)lo; v[1] = (T)hi;
  return __builtin_bit_cast(unsigned, v);
}

constexpr int kStageStride = 136;   // floats per staged row: 16-B aligned, and 4 rows = 32 banks so both lane halves write conflict-free
constexpr int kStageStrideT = 260;  // floats per row of the transposed staging ([128 channels][256 tile rows]) of the qkv epilogue's v tiles
static_assert(128 * kStageStrideT <= 256 * kStageStride, "the transposed tile lives in the staging area");

// KIND: what one chunk (= one block barrier) holds and how its NS sub-steps (one 16-channel MFMA k-step each) address it.
// A chunk is NPL planes of BROW-byte rows, one row per patch position; sub-step s reads plane s / NTAB through gather-table
// row s % NTAB (table entry = row byte offset | 16-B piece key, the lane's k-half h is XORed into the key):
//   RS_3X3 (stride 1 / nearest-up): NS 9 = 9 taps of one haloed 16-channel plane (32-B rows)
//   RS_SUB (sub-pixel nearest-x2 + 3x3): NS 8 = 2 planes x 2x2 pre-summed taps per output parity; grid = 4 parities x tiles,
//          tiles cut on the low-res grid, rows scattered to output pixel (2y+py, 2x+px)
//          The same kind runs Downsample.op on space-to-depth planes (STEDM_CONV_S2D): one "parity", no scatter, 2x2 taps at
//          offsets (-1, 0) over 4*cin channels.
//   RS_1X1: NS 4 = the 4 16-channel slices of one 64-channel plane of the tile's own 256 pixels (128-B rows: a DMA lane group
//          of 8 fetches one full 128-B line; the table row of slice s carries the piece key 2s ^ swizzle)
//   RS_3X3M: the 3x3 kind on v_mfma_f32_16x16x32 (MI355X_MICROARCH.md "DVFS give-back" item 7: on random data the chip holds a higher
//          clock on the 16x16x32 shape than on 32x32x16 at equal cycles per FLOP). Same 128 x 64 slab per compute wave, as 8 x 4
//          accumulators of 16 x 16. A chunk is 32 channels = TWO 16-channel planes of the usual 32-B rows (the LDS image and the DMA
//          are those of RS_3X3, minus the XOR swizzle); sub-step = one tap x 32 channels, the MFMA's four 8-element k-groups
//          g = lane >> 4 are (plane g & 1, 16-B piece g >> 1). The second plane's image is skewed by 16 B: a ds_read_b128 group then
//          reads 8 rows of plane 0 (even 16-B slots) and 8 rows of plane 1 (odd slots) — conflict-free WITHOUT a swizzle, so a tap is
//          a wave-uniform byte offset ((dy * PW + dx) * 32, added to the chunk base in scalar registers) and a lane keeps 8 fragment
//          offsets instead of 9 x 8. Weights in the matching fragment order (stedm_pack_conv_weight_frag16, args.w_frag16).
// In all cases consecutive sub-steps are consecutive [cin/16][taps] blocks of the fragment-order weights.
//   RS_1X1N: the 1x1 kind in its N-persistent form (a flat short-K GEMM: one block per M-tile walks every N-tile; see the kernel)
//   RS_1X1M: a 1x1 on v_mfma_f32_16x16x32 for the 3-product modes (P3): a chunk is 32 channels of the tile's own 256 pixels as ONE plane of
//          64-B rows in natural piece order (a ds_read_b128 group reads 16 rows x 4 pieces = 1 KiB contiguous: conflict-free without
//          swizzle or skew), k-group g = lane >> 4 is piece g; one sub-step (one "tap") per chunk; weights from
//          stedm_pack_conv_weight_frag16_hl1 (hi stream, then lo stream)
//   RS_SUBM: the RS_SUB geometry (sub-pixel upsample: 4 output parities, scattered rows; space-to-depth downsample) on v_mfma_f32_16x16x32
//          (round 4: the 3-product modes; round 5: the single-product modes too, reading the hi stream of the same pack - the two
//          Upsample convolutions, the largest GEMMs of a step, ran the 32x32x16 RS_SUB form at 35 % MFMA-busy with 56 % of its LDS
//          cycles in bank conflicts): the LDS image of RS_3X3M (32 channels = two skewed 16-channel planes), 4 taps as uniform offsets
//          ((t >> 1) * PW + (t & 1)) * 32 from the tap-0 row (which carries the parity's (py, px) shift); weights from
//          stedm_pack_conv_weight_up_frag16_hl / stedm_pack_conv_weight_s2d_frag16_hl
enum { RS_3X3 = 0, RS_1X1 = 1, RS_SUB = 2, RS_3X3M = 4, RS_1X1N = 5, RS_1X1M = 6, RS_SUBM = 7 };

// One K-phase of a compute wave: `nchunks` chunks of NS sub-steps. A fragments come from the LDS chunk ring (4 buffers of a_buf
// bytes at A0, ring position `abuf`, one block barrier per chunk at sub-step NS-LA-1), B fragments stream from `wq` (sub-step g at
// wq + g*4096, second fragment +1024). Plain loads: the compiler counts vmcnt / lgkmcnt exactly, sched_barrier(0) pins each
// group where it is written (fragment loads LA / NSB sub-steps ahead of their MFMAs).
// NOBAR: every chunk of the phase is already resident in the ring (the N-persistent form below re-walks it): no chunk barriers.
// SWAP: the MFMA's operands trade places, so the accumulators hold the TRANSPOSED 32 x 32 blocks (rows = output channels, columns = tile rows).
template <typename T, int WM, int NS, int NTAB, bool FIRST, bool SPREAD = false, bool NOBAR = false, bool SWAP = false>
__device__ __forceinline__ void rs_phase(f32x16 (&acc)[WM][2], const unsigned (&aofs)[NTAB][WM], const unsigned A0, const int a_buf,
                                         const int a_plane, int& abuf, const int nchunks, const unsigned char* wq, const unsigned voff,
                                         const int dbg = 0) {
  using V8 = typename MM<T>::V8;
  constexpr int NSA = NS % 3 == 0 ? 3 : 4;               // A-fragment register stages
  constexpr int NSB = NS % 3 == 0 ? 3 : 4;               // weight-fragment register stages (look-ahead NSB sub-steps)
  constexpr int LA = 2;                                  // A-fragment look-ahead in sub-steps (< NSA)
  constexpr int NABUF = 4;
  static_assert(NS % NSA == 0 && NS % NSB == 0 && NS > LA + 1, "stage rotation must be chunk-periodic");
  const int gmax = nchunks * NS - 1;
  V8 af[NSA][WM], bf[NSB][2];
#define RS_MFMA(A, B, C) (SWAP ? MM<T>::mfma(B, A, C) : MM<T>::mfma(A, B, C))
#define LDSR(dst, addr) dst = *reinterpret_cast<const V8 __attribute__((address_space(3)))*>(addr)
#define GLDB(dst, sbase, off) dst = *reinterpret_cast<const V8*>((sbase) + voff + (off))
#define LOAD_B(G, ST)                                                          \
  {                                                                            \
    int g_ = (G);                                                              \
    g_ = g_ < gmax ? g_ : gmax;   /* keeps the load count uniform at the tail */ \
    if STEDM_DBG(dbg, 1) g_ &= 3;         /* timing ablation: weight stream from L1 */  \
    const unsigned char* sb_ = wq + ((size_t)(unsigned)g_ << 12);              \
    GLDB(bf[ST][0], sb_, 0); GLDB(bf[ST][1], sb_, 1024);                       \
  }
  // sub-step SUB of the chunk at BASE: plane SUB / NTAB, gather-table row SUB % NTAB
#define LOAD_A(BASE, SUB, ST)                                                  \
  {                                                                            \
    const unsigned pb_ = (BASE) + ((SUB) / NTAB) * a_plane;                    \
    _Pragma("unroll") for (int i_ = 0; i_ < WM; ++i_) { const unsigned a_ = pb_ + aofs[(SUB) % NTAB][i_]; LDSR(af[ST][i_], a_); } \
  }
  // Round 4: the fillers are spread over the MFMA gaps instead of sitting in two blocks per sub-step (tools/conv_phases.py in-loop stamps: the
  // blocked form ran the MFMA pipe 72 - 75 % of the loop's cycles; the 16x16x32 kind went 72 -> 90 % with one filler per gap, rs_phase16): the
  // A fragment of row block i for sub-step t + LA is read in the gap behind this sub-step's MFMA 2 i (its stage was consumed at least one
  // sub-step ago), the two weight fragments of sub-step (g - 1) + NSB go into the stage sub-step g - 1 used, in the gaps behind the first two
  // MFMAs of the second half (at the phase's first sub-step that re-reads what the prologue loaded into the same registers).
#define LOAD_A1(BASE, SUB, ST, I)                                              \
  {                                                                            \
    const unsigned a_ = (BASE) + ((SUB) / NTAB) * a_plane + aofs[(SUB) % NTAB][I]; \
    LDSR(af[ST][I], a_);                                                       \
  }
#pragma unroll
  for (int k = 0; k < NSB; ++k) LOAD_B(k, k)
  if (FIRST) __syncthreads();   // B_init: chunks 0 and 1 landed; start-up tables consumed by every wave
  {
    const unsigned Afirst = A0 + abuf * a_buf;
#pragma unroll
    for (int k = 0; k < LA; ++k) LOAD_A(Afirst, k, k)
  }
  // (SPREAD false: the blocked form — the 9-tap kinds carry 36 gather offsets per lane and sit at 247 - 249 registers; spreading the reads
  // lengthened enough live ranges to spill 48 - 52 bytes inside the loop, so they keep the blocked schedule)
  if constexpr (!SPREAD) {
  for (int step = 0; step < nchunks; ++step) {
    const unsigned Acur = A0 + abuf * a_buf;
    if (++abuf == NABUF) abuf = 0;
    const unsigned Anext = step + 1 < nchunks ? A0 + abuf * a_buf : Acur;
    const int g0 = step * NS;
#pragma unroll
    for (int t = 0; t < NS; ++t) {
      if (!NOBAR && t == NS - LA - 1) __builtin_amdgcn_s_barrier();   // chunk barrier: next chunk landed, previous buffer released
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[0][j] = RS_MFMA(af[t % NSA][0], bf[t % NSB][j], acc[0][j]);
      __builtin_amdgcn_sched_barrier(0);
      // fragments LA sub-steps ahead, issued under the first MFMAs; their stage was consumed at least one sub-step ago
      if (t + LA < NS) LOAD_A(Acur, t + LA, (t + LA) % NSA) else LOAD_A(Anext, t + LA - NS, (t + LA) % NSA)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int i = 1; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = RS_MFMA(af[t % NSA][i], bf[t % NSB][j], acc[i][j]);
      __builtin_amdgcn_sched_barrier(0);
      // the weight fragments of sub-step g+NSB go into the stage just consumed
      LOAD_B(g0 + t + NSB, t % NSB)
    }
  }
  } else
  for (int step = 0; step < nchunks; ++step) {
    const unsigned Acur = A0 + abuf * a_buf;
    if (++abuf == NABUF) abuf = 0;
    // on the phase's last chunk the look-ahead reads re-read the current buffer (values unused): keeps the counters uniform
    const unsigned Anext = step + 1 < nchunks ? A0 + abuf * a_buf : Acur;
    const int g0 = step * NS;
#pragma unroll
    for (int t = 0; t < NS; ++t) {
      if (!NOBAR && t == NS - LA - 1) __builtin_amdgcn_s_barrier();   // chunk barrier: next chunk landed, previous buffer released
      int gw_ = g0 + t - 1 + NSB;
      gw_ = gw_ < gmax ? gw_ : gmax;  /* keeps the load count uniform at the tail */
      if STEDM_DBG(dbg, 1) gw_ &= 3;          /* timing ablation: weight stream from L1 */
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          __builtin_amdgcn_sched_barrier(0);
          acc[i][j] = RS_MFMA(af[t % NSA][i], bf[t % NSB][j], acc[i][j]);
          __builtin_amdgcn_sched_barrier(0);
          const int m = 2 * i + j;          // MFMA index inside the sub-step (2 WM per sub-step)
          if (m < WM) {                     // row block m of the sub-step LA ahead
            if (t + LA < NS) LOAD_A1(Acur, t + LA, (t + LA) % NSA, m) else LOAD_A1(Anext, t + LA - NS, (t + LA) % NSA, m)
          } else if (m == WM) { const unsigned char* sbw = wq + ((size_t)(unsigned)gw_ << 12); GLDB(bf[(t + NSB - 1) % NSB][0], sbw, 0); }
          else if (m == WM + 1) { const unsigned char* sbw = wq + ((size_t)(unsigned)gw_ << 12); GLDB(bf[(t + NSB - 1) % NSB][1], sbw, 1024); }
        }
    }
  }
  __builtin_amdgcn_sched_barrier(0);
#undef LOAD_A1
#undef LOAD_A
#undef LOAD_B
#undef GLDB
#undef LDSR
#undef RS_MFMA
}


// K-phase of a compute wave on the 16x16x32 MFMA (RS_3X3M). Pipeline unit = half a sub-step: 4 of the wave's 8 row fragments x its 4
// column fragments = 16 MFMAs (256 cycles, the length of a 32x32x16 sub-step).
// A: ONE register stage of 4 fragments, refilled fragment by fragment: as soon as the 4 MFMAs that read af[i] are issued, the next
// unit's fragment i is loaded into it (12 MFMAs = 192 cycles ahead of its use). aofs[f]: the lane's byte offset of row fragment f at
// tap (0, 0) inside a chunk buffer (plane and 16-B piece of its k-group included); tapd[t]: the tap's uniform byte offset.
// B: three register stages of 4 fragments (NS % 3 == 0: the stage rotation is chunk-periodic), loaded two sub-steps ahead
// (sub-step g at wq + g * 8192, fragment c at + c * 1024).
// NSETS 1: one offset set, taps are uniform byte offsets (3x3). NSETS == NS: one offset set per sub-step, tapd unused (the fused 1x1
// phase: sub-step s reads the 16-B pieces 4 s + g of a swizzled 128-B row).
template <typename T, int NS, int NSETS, bool FIRST>
__device__ __forceinline__ void rs_phase16(f32x4 (&acc)[8][4], const unsigned (&aofs)[NSETS][8], const unsigned (&tapd)[NS], const unsigned A0,
                                           const int a_buf, int& abuf, const int nchunks, const unsigned char* wq, const unsigned voff, const int dbg = 0) {
  using V8 = typename MM<T>::V8;
  constexpr int NU = 2 * NS, NABUF = 4;
  constexpr int NSB = NS % 3 == 0 ? 3 : 2;      // weight-fragment stages: the rotation must be chunk-periodic
  static_assert(NS % NSB == 0 && (NSETS == 1 || NSETS == NS), "stage rotation / offset sets");
  const int gmax = nchunks * NS - 1;
  V8 af[4], bf[NSB][4];
#define LDSR(dst, addr) dst = *reinterpret_cast<const V8 __attribute__((address_space(3)))*>(addr)
  // Round 4: ONE filler per MFMA gap. In-loop stamps (tools/conv_phases.py; profiles/r04_conv_loop_attribution.md) put the loop's MFMA duty
  // at 72.5 % of its cycles, and compile-time removal of the ingredients attributes the rest: the A-fragment reads 13 points, the weight loads
  // 7, the chunk barrier 0 - a 16x16x32 MFMA holds the SIMD's issue port for 8 of its 16 cycles, so the three instructions that used to sit
  // between two groups of four MFMAs (address add, ds_read_b128, the next group's s_waitcnt) overran the 8 free cycles of ONE gap. Now the
  // fragment a group has consumed is reloaded inside the NEXT group - its address add in the gap behind that group's first MFMA, its
  // ds_read_b128 behind the second (10 MFMAs = 160 cycles ahead of its use) - and the four weight-fragment loads of a sub-step go, one per
  // gap, into the third / fourth gaps of the following sub-step's first groups (1.9 instead of 2.0 sub-steps ahead of their use).
  const unsigned char* wsb = wq + voff;           // per-lane base of the weight stream; advanced by the scalar sub-step offset below
  const unsigned char* wcur = wsb;
#define W_ADDR(G)                                                              \
  {                                                                            \
    int g_ = (G);                                                              \
    g_ = g_ < gmax ? g_ : gmax;   /* keeps the load count uniform at the tail */ \
    if STEDM_DBG(dbg, 1) g_ &= 3;         /* timing ablation: weight stream from L1 */  \
    wcur = wsb + ((size_t)(unsigned)g_ << 13);                                 \
  }
#define W_LOAD(ST, C) if constexpr (!RS_DIAG(16)) bf[ST][C] = *reinterpret_cast<const V8*>(wcur + (C) * 1024);
  // address of fragment I (0..3) of unit (TAP, HF) of the chunk at BASE (uniform): one VALU add, opaque so that it stays in its gap
#define A_ADDR(DST, BASE, TAP, HF, I)                                                                         \
  {                                                                                                           \
    if constexpr (NSETS == 1) asm volatile("v_add_u32 %0, %1, %2" : "=v"(DST) : "s"((BASE) + tapd[TAP]), "v"(aofs[0][(HF) * 4 + (I)])); \
    else asm volatile("v_add_u32 %0, %1, %2" : "=v"(DST) : "s"(BASE), "v"(aofs[NSETS == 1 ? 0 : (TAP)][(HF) * 4 + (I)]));           \
  }
#pragma unroll
  for (int k = 0; k < NSB; ++k) {
    W_ADDR(k)
#pragma unroll
    for (int c = 0; c < 4; ++c) W_LOAD(k, c)
  }
  if (FIRST) __syncthreads();   // B_init: chunks 0 and 1 landed; start-up tables consumed by every wave
  {
    const unsigned Afirst = A0 + abuf * a_buf;
#pragma unroll
    for (int i = 0; i < 4; ++i) { unsigned a_; A_ADDR(a_, Afirst, 0, 0, i) if constexpr (!RS_DIAG(8)) LDSR(af[i], a_); }
  }
  for (int step = 0; step < nchunks; ++step) {
    const unsigned Acur = A0 + abuf * a_buf;
    if (++abuf == NABUF) abuf = 0;
    // on the phase's last chunk the look-ahead reads re-read the current buffer (values unused): keeps the counters uniform
    const unsigned Anext = step + 1 < nchunks ? A0 + abuf * a_buf : Acur;
    const int g0 = step * NS;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int t = u >> 1, hf = u & 1;
      if (u == NU - 1 && !RS_DIAG(32)) __builtin_amdgcn_s_barrier();   // chunk barrier: the next chunk has landed (read from here on), the previous buffer is released
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        // the fragment this group reloads: the one the PREVIOUS group consumed (i - 1 of this unit, or 3 of the previous unit), for its next
        // use one unit on: unit u + 1 for fragments 0..2 (a unit of the next chunk behind the barrier), unit u itself for fragment 3
        const int pi = (i + 3) & 3;
        const int tu = i == 0 ? u : u + 1;
        unsigned a_ = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          __builtin_amdgcn_sched_barrier(0);
          acc[hf * 4 + i][j] = MM<T>::mfma16(af[i], bf[t % NSB][j], acc[hf * 4 + i][j]);
          __builtin_amdgcn_sched_barrier(0);
          if (j == 0) {
            if (tu < NU) A_ADDR(a_, Acur, tu >> 1, tu & 1, pi) else A_ADDR(a_, Anext, 0, 0, pi)
          } else if (j == 1) {
            if constexpr (!RS_DIAG(8)) LDSR(af[pi], a_);
          } else if (hf == 0) {
            // weight fragments of sub-step (g0 + t - 1) + NSB into the stage sub-step t - 1 used (free since that sub-step ended; at the
            // phase's first sub-step this re-reads what the prologue loaded into the same registers)
            const int st = (t + NSB - 1) % NSB;
            if (i == 0 && j == 2) W_ADDR(g0 + t - 1 + NSB)
            if (i == 0 && j == 3) W_LOAD(st, 0)
            if (i == 1 && j == 2) W_LOAD(st, 1)
            if (i == 1 && j == 3) W_LOAD(st, 2)
            if (i == 2 && j == 2) W_LOAD(st, 3)
          }
        }
      }
    }
  }
  __builtin_amdgcn_sched_barrier(0);
#undef A_ADDR
#undef W_LOAD
#undef W_ADDR
#undef LDSR
}

// K-phase of a compute wave in the 3-product (hi / lo split) mode on the 16x16x32 MFMA: every (row fragment, column fragment) pair takes
// lo.hi + hi.lo + hi.hi (the lo.lo term is below fp32 resolution), so a unit is 48 MFMAs against the same 8 LDS reads and a sub-step 96
// MFMAs against 8 weight-fragment loads: per MFMA a third fewer operand bytes than the single-product loop. The lo image of a chunk
// sits a_half bytes behind the hi image in the same ring buffer, the lo weight stream wlo bytes behind the hi stream.
// A: a ring of NAR = 2 (hi, lo) fragment pairs: the pair of row fragment i + 2 is loaded once the 12 MFMAs of fragment i are issued, 12 MFMAs
// (192 cycles) ahead of its use (the register budget of 2 waves per SIMD is 256; NAR = 4 measured the same, 2874 vs 2876 us over the nine
// layer shapes of the step). B: TWO stages of 4 (hi, lo) pairs, loaded
// one sub-step (96 MFMAs = 1536 cycles) ahead; NS is odd, so the stage of sub-step t alternates from chunk to chunk: the chunk body
// exists for both parities. The ring has 3 buffers (a chunk is twice the bytes and three times the MFMA time of the single-product one).
template <typename T, int NS, int NAR>
__device__ __forceinline__ void rs_phase16_p3(f32x4 (&acc)[8][4], const unsigned (&aofs)[8], const unsigned (&tapd)[NS], const unsigned A0,
                                              const int a_buf, const unsigned a_half, int& abuf, const int nchunks, const unsigned char* wq,
                                              const size_t wlo, const unsigned voff) {
  using V8 = typename MM<T>::V8;
  constexpr int NU = 2 * NS, NABUF = 3;
  const int gmax = nchunks * NS - 1;
  V8 ah[NAR], al[NAR], bh[2][4], bl[2][4];
#define LDSR(dst, addr) dst = *reinterpret_cast<const V8 __attribute__((address_space(3)))*>(addr)
#define LOAD_B3(G, ST)                                                         \
  {                                                                            \
    int g_ = (G);                                                              \
    g_ = g_ < gmax ? g_ : gmax;                                                \
    const unsigned char* sb_ = wq + ((size_t)(unsigned)g_ << 13) + voff;       \
    _Pragma("unroll") for (int c_ = 0; c_ < 4; ++c_) {                         \
      bh[ST][c_] = *reinterpret_cast<const V8*>(sb_ + c_ * 1024);              \
      bl[ST][c_] = *reinterpret_cast<const V8*>(sb_ + wlo + c_ * 1024);        \
    }                                                                          \
  }
  /* row fragment F (0..7) of tap TAP of the chunk at BASE into ring slot F & 1 */ \
  /* (the two adds are opaque: left to the compiler, the 72 tap + fragment sums are hoisted out of the loop and spilled) */ \
#define LOAD_A3(BASE, TAP, F)                                                  \
  {                                                                            \
    unsigned a_, a2_;                                                          \
    asm volatile("v_add_u32 %0, %1, %2" : "=v"(a_) : "s"((BASE) + tapd[TAP]), "v"(aofs[F]));             \
    asm volatile("v_add_u32 %0, %1, %2" : "=v"(a2_) : "s"((BASE) + tapd[TAP] + a_half), "v"(aofs[F]));   \
    LDSR(ah[(F) & (NAR - 1)], a_);                                             \
    LDSR(al[(F) & (NAR - 1)], a2_);                                            \
  }
  // one chunk; PAR = parity of its first sub-step's global index.
  // Round 4: one filler per MFMA gap (as rs_phase16; profiles/r04_conv_loop_attribution.md). A group is the 12 MFMAs of one row fragment R; the
  // ring slot the PREVIOUS group consumed is refilled with fragment R + 1 inside this group: its hi / lo reads sit behind MFMAs 0 and 1 (10 - 11
  // MFMAs ahead of their use), their two address adds behind MFMAs 10 and 11 of the group before; the eight weight-fragment loads of a sub-step
  // (stream index g + 1 into the stage sub-step g - 1 used) go one per gap behind MFMAs 4..11 of the sub-step's first group.
  // fragment the group AFTER group Q refills (= Q + 2 in the (tap, row fragment) order)
#define A3_AFTER(Q, WHAT)                                                                                          \
  {                                                                                                                \
    if ((Q) + 2 < 8) { WHAT(Acur, t, (Q) + 2) }                                                                    \
    else if (t + 1 < NS) { WHAT(Acur, t + 1, (Q) + 2 - 8) }                                                         \
    else { WHAT(Anext, 0, (Q) + 2 - 8) }                                                                           \
  }
#define A3_ADDR_HI(BASE, TAP, F) asm volatile("v_add_u32 %0, %1, %2" : "=v"(a_) : "s"((BASE) + tapd[TAP]), "v"(aofs[F]));
#define A3_ADDR_LO(BASE, TAP, F) asm volatile("v_add_u32 %0, %1, %2" : "=v"(a2_) : "s"((BASE) + tapd[TAP] + a_half), "v"(aofs[F]));
#define RS3_CHUNK(PAR)                                                                                             \
  _Pragma("unroll") for (int u = 0; u < NU; ++u) {                                                                 \
    const int t = u >> 1, hf = u & 1, sb = (t & 1) ^ (PAR);                                                        \
    if (u == NU - 1) __builtin_amdgcn_s_barrier();   /* the next chunk has landed, the previous buffer is released */ \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                \
      const int R = hf * 4 + i;                       /* row fragment of this group; its ring slot is R & 1 */      \
      _Pragma("unroll") for (int m = 0; m < 12; ++m) {                                                             \
        const int j = m & 3;                                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                                         \
        if (m < 4) acc[R][j] = MM<T>::mfma16(al[R & (NAR - 1)], bh[sb][j], acc[R][j]);                              \
        else if (m < 8) acc[R][j] = MM<T>::mfma16(ah[R & (NAR - 1)], bl[sb][j], acc[R][j]);                         \
        else acc[R][j] = MM<T>::mfma16(ah[R & (NAR - 1)], bh[sb][j], acc[R][j]);                                    \
        __builtin_amdgcn_sched_barrier(0);                                                                         \
        if (m == 0) { LDSR(ah[(R + 1) & (NAR - 1)], a_); }                                                          \
        else if (m == 1) { LDSR(al[(R + 1) & (NAR - 1)], a2_); }                                                    \
        if (R == 0 && m >= 4) {                                                                                    \
          /* weights of stream index g0 + t + 1 into the other stage (the one sub-step t - 1 used) */              \
          if (m == 4) { int g_ = g0 + t + 1; g_ = g_ < gmax ? g_ : gmax; wcur = wq + ((size_t)(unsigned)g_ << 13) + voff; } \
          if (m < 8) bh[sb ^ 1][m - 4] = *reinterpret_cast<const V8*>(wcur + (m - 4) * 1024);                        \
          else bl[sb ^ 1][m - 8] = *reinterpret_cast<const V8*>(wcur + wlo + (m - 8) * 1024);                        \
        }                                                                                                          \
        if (m == 10) A3_AFTER(R, A3_ADDR_HI)                                                                        \
        else if (m == 11) A3_AFTER(R, A3_ADDR_LO)                                                                   \
      }                                                                                                            \
    }                                                                                                              \
  }
  const unsigned char* wcur = wq + voff;
  unsigned a_ = 0, a2_ = 0;      // addresses of the fragment the next group refills (computed in the tail gaps of the group before)
  LOAD_B3(0, 0)
  LOAD_B3(1, 1)
  __syncthreads();   // B_init: chunks 0 and 1 landed; start-up tables consumed by every wave
  {
    const unsigned Afirst = A0 + abuf * a_buf;
#pragma unroll
    for (int f = 0; f < NAR; ++f) LOAD_A3(Afirst, 0, f)
    // the first group refills slot 1 with fragment 1 (what the line above just put there: a redundant read that keeps the loop uniform)
    A3_ADDR_HI(Afirst, 0, 1)
    A3_ADDR_LO(Afirst, 0, 1)
  }
  // two chunks per loop iteration (the stage parity is then the same at every loop header; the two bodies as the arms of a branch
  // inside the loop made the register allocator spill), an odd last chunk after the loop
#define RS3_STEP(STEP, PAR)                                                                                        \
  {                                                                                                                \
    const unsigned Acur = A0 + abuf * a_buf;                                                                       \
    if (++abuf == NABUF) abuf = 0;                                                                                 \
    /* last chunk: the look-ahead re-reads the current buffer (values unused) */                                   \
    const unsigned Anext = (STEP) + 1 < nchunks ? A0 + abuf * a_buf : Acur;                                        \
    const int g0 = (STEP) * NS;                                                                                    \
    RS3_CHUNK(PAR)                                                                                                 \
  }
  int step = 0;
  for (; step + 1 < nchunks; step += 2) {
    RS3_STEP(step, 0)
    RS3_STEP(step + 1, NS & 1)      // (an even NS keeps the stage parity of a chunk's first sub-step: RS_SUBM's four taps)
  }
  if (step < nchunks) RS3_STEP(step, 0)
#undef RS3_STEP
#undef RS3_CHUNK
#undef A3_AFTER
#undef A3_ADDR_HI
#undef A3_ADDR_LO
#undef LOAD_A3
#undef LOAD_B3
#undef LDSR
}

// FUSE (RS_3X3, stride 1 only): a second K-phase adds the ResBlock's 1x1 skip_connection (openaimodel.py:254, 288) over the raw
// 16-bit planes src16b [B][H][W][cb] of the block input: out = conv3x3(src16) + conv1x1(src16b) + bias + bias_b. The chunk ring
// simply continues with 64-channel 1x1 chunks (128-B rows of the tile's own pixels) and the weight stream switches to w_frag_b,
// so the skip's MACs run in the same MFMA loop and its output is never written and re-read as a residual.
// P3 (RS_3X3M only): the 3-product mode (npass = 3). The chunk ring holds the hi and the lo image of each chunk (3 buffers instead of 4),
// a.w_frag16 holds the hi fragment stream followed by the lo stream (stedm_pack_conv_weight_frag16_hl), the K-phase is rs_phase16_p3.
template <typename T, int WM, int KIND, bool FUSE = false, bool P3 = false>
__global__ void __launch_bounds__((16 / WM + 2) * 64) conv_rs_kernel(const ConvParams p) {
  static_assert(!FUSE || KIND == RS_3X3 || KIND == RS_3X3M, "the fused skip phase belongs to the 3x3 kinds");
  static_assert(!P3 || ((KIND == RS_3X3M || KIND == RS_1X1M || KIND == RS_SUBM) && !FUSE), "the 3-product form exists for the plain 16x16x32 kinds");
  static_assert(KIND != RS_1X1M || (P3 && !FUSE && WM == 4), "RS_1X1M is a 3-product kind");
  static_assert(KIND != RS_SUBM || (!FUSE && WM == 4), "RS_SUBM: plain epilogues, one compute wave per SIMD");
  constexpr int NCW = 16 / WM, NT = (NCW + 2) * 64, BMT = 256;
  constexpr bool NPERS = KIND == RS_1X1N, IS1X1 = KIND == RS_1X1 || NPERS, SUBM = KIND == RS_SUBM, SUBPIX = KIND == RS_SUB || SUBM;
  constexpr bool G1 = KIND == RS_1X1M;                   // 1x1 geometry on the 16x16x32 MFMA (3-product modes)
  constexpr bool M16 = KIND == RS_3X3M || G1 || SUBM;    // 16x16x32 MFMA forms: tap-0 gather row + uniform tap offsets, no XOR swizzle
  constexpr bool GEO1 = IS1X1 || G1;                     // the patch is the tile's own pixels
  constexpr bool IS3X3 = KIND == RS_3X3 || KIND == RS_3X3M;
  constexpr bool RES2 = IS3X3 && !FUSE && !P3;           // stedm_conv_args.res2 (host: the kinds that take res_bmod); every other instantiation compiles none of it
  constexpr int NS = IS3X3 ? 9 : (SUBM ? 4 : (SUBPIX ? 8 : (G1 ? 1 : 4)));   // sub-steps per chunk
  constexpr int NPL = (SUBPIX || KIND == RS_3X3M) ? 2 : 1;      // planes per chunk
  constexpr int NTAB = IS3X3 ? 9 : 4;                    // gather-table rows (taps, or k-slices of the 1x1 row)
  constexpr int BROW = IS1X1 ? 128 : (G1 ? 64 : 32);     // bytes per LDS row
  constexpr int CPP = BROW / 16, RPB = 16 / CPP, PPI = 64 / CPP;   // 16-B pieces per row, rows per 256 B, rows per DMA instruction
  constexpr int BKC = M16 ? 32 : NS * 16 / (IS3X3 ? 9 : (SUBPIX ? 4 : 1));   // channels per chunk: 16 (64 wide), 32, 64
  constexpr int TAPS = NTAB, NABUF = P3 ? 3 : 4;
  constexpr int SST = kStageStride;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nai = (p.NP + PPI - 1) / PPI;
  const int a_plane = nai * 1024;
  // ring buffer size. Fused skip phase: a 1x1 chunk is 256 pixels x 128 B
  const int a_half = NPL * a_plane + (M16 ? 32 : 0);          // one image of a chunk (P3: the lo image follows the hi image)
  const int a_buf = P3 ? 2 * a_half : ((FUSE && NPL * a_plane < 32768) ? 32768 : a_half);
  const int pl_skew = (KIND == RS_3X3M || SUBM) ? 16 : 0;     // two-plane 16x16x32 kinds: byte skew of plane 1 (bank-slot parity), no XOR swizzle
  int* sM = reinterpret_cast<int*>(smem);                    // [BMT] output pixel of each tile row (-1: beyond M)
  int* sMb = sM + BMT;                                       // [BMT] its sample
  unsigned char* sA = reinterpret_cast<unsigned char*>(sMb + BMT);   // [NABUF][nai*1024]; epilogue: fp32 tile [BMT][SST]
  float* sStage = reinterpret_cast<float*>(sA);
  const int ring_bytes = NABUF * a_buf;
  int* sIdx = reinterpret_cast<int*>(sA + ring_bytes);       // start-up: [TAPS][BMT] gather table

  const stedm_conv_args& a = p.a;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool is_loader = wave >= NCW;
  const int ntile = p.tiles_m * p.tiles_n;
  const bool s2d = SUBPIX && a.mode == STEDM_CONV_S2D;       // stride-2 conv on space-to-depth planes: taps of "parity 0", plain rows
  const int parity = (SUBPIX && !s2d) ? (blockIdx.x / ntile) & 3 : 0;   // output parity class py*2+px
  // K split (3x3 without the fused phase, small grids): ksplit blocks per tile, each an equal share of the chunks, each writes its
  // raw partial tile to the workspace a.ws[kz][M][cout]; conv_splitk_reduce_kernel adds them in a fixed order with bias / emb / residual
  const bool split = (IS3X3 || SUBPIX || GEO1) && p.ksplit >= 2;      // (FUSE: every K share also takes its share of the skip's 64-channel chunks)
  // (sub-pixel upsample with a K split: blockIdx.x = (kz * 4 + parity) * ntile + tile)
  const int kz = split ? ((SUBPIX && !s2d) ? blockIdx.x / (4 * ntile) : blockIdx.x / ntile) : 0;
  const int bid = (SUBPIX || split) ? blockIdx.x % ntile : blockIdx.x;
  const int py = parity >> 1, px = parity & 1;
  int tile_n = bid % p.tiles_n, tile_m = bid / p.tiles_n;
  // XCD-aware order: the hardware deals block ids round-robin over the 8 XCDs, each with its own L2. Plain order puts the N-tiles of one
  // M-tile on min(8, tiles_n) different XCDs: every one of them fetches the same patch through the fabric, and each weight slice crosses
  // it once. With gm = p.xcd_m the XCDs form a gm x (8 / gm) grid: XCD x = L & 7 owns the M-tiles = x % gm (mod gm) and the N-tiles
  // = x / gm (mod 8 / gm) and walks the N-tiles of an M-tile back to back; the patch then crosses the fabric 8 / gm times and the weights
  // gm times. The host picks the cheapest of the four orders for the problem (conv_rs_try).
  if (p.xcd_m) {
    const int gm = p.xcd_m, gn = 8 / gm, x = bid & 7, j = bid >> 3, tn_x = p.tiles_n / gn;
    const int jm = j / tn_x;
    tile_n = (j - jm * tn_x) * gn + x / gm;
    tile_m = jm * gm + x % gm;
  }
  // N-persistent form (1x1 kind, flat GEMM with its whole K in the ring: conv_rs_try): one block per M-tile walks every N-tile
  constexpr bool npers = NPERS;
  // (p.npers = blocks per M-tile, each an equal share of the N-tiles: 2 when one block per tile would leave a mostly empty last round)
  if (npers) { tile_m = bid / p.npers; tile_n = (bid % p.npers) * (p.tiles_n / p.npers); }
  if STEDM_DBG(p.dbg, 256) { tile_n = 0; tile_m = 0; }
  const int m0 = tile_m * BMT, n0 = tile_n * BN;
  const int nchunks_all = p.Cin / BKC;
  // K window (stedm_conv_args.k_chan0 / w_cin, the plain 3x3 kinds): the host moved src16_hi and the fragment stream to the window's first
  // chunk, so only two things differ from the plain form: the pixel rows are p.cstride elements apart and an N-tile of the pack holds
  // nchunks_w chunks. The chunk walk itself (and the K split's share of it) runs over the window's p.Cin channels as ever.
  const int nchunks_w = p.w_cin / BKC;
  const int nsteps = split ? nchunks_all / p.ksplit : nchunks_all;   // chunks of this block
  const int cbeg = kz * nsteps;                               // its first chunk
  const int nsteps2_all = FUSE ? a.cb / 64 : 0;      // chunks of the fused 1x1 phase
  const int nsteps2 = split ? nsteps2_all / p.ksplit : nsteps2_all;      // ... of this block (the host checked divisibility)
  const int c2beg = split ? kz * nsteps2 : 0;
  STAMP(0);

  int b0, yo0;
  if (p.whole) { b0 = tile_m * p.nsamp; yo0 = 0; }
  else { b0 = m0 / p.HWout; yo0 = (m0 - b0 * p.HWout) / p.Wout; }
  const int br = s2d ? a.pad_br : 0;                          // bottom/right-padded stride-2 conv: the 2x2 taps sit at (0, +1)
  const int x0 = p.wsplit ? (m0 - b0 * p.HWout) - yo0 * p.Wout : 0;   // rows wider than the tile: its first column (the patch columns are tile-local)
  const int srow0 = ((a.mode == STEDM_CONV_S1 || SUBPIX) ? yo0 - 1 : (yo0 - 1) >> 1) + br;
  static_assert(RS_3X3 == 0, "");

  // tile-geometry tables; every numerator below is < 2^16, so n / d = umulhi(n, ceil(2^32 / d)) exactly (magics from the host)
  auto div_hw = [&](int n) { return (int)__umulhi((unsigned)n, p.mg_hw); };
  auto div_w = [&](int n) { return (int)__umulhi((unsigned)n, p.mg_w); };
  auto div_pw = [&](int n) { return (int)__umulhi((unsigned)n, p.mg_pw); };
  auto div_prpw = [&](int n) { return (int)__umulhi((unsigned)n, p.mg_prpw); };
  const int rem0 = GEO1 ? m0 - (m0 / p.HWout) * p.HWout : 0;   // 1x1: offset of the tile's first pixel inside its sample
  // source pixel of patch position `pos` (-1: halo / padding / beyond the batch -> zero page)
  auto patch_pixel = [&](int pos) {
    int off = -1;
    if (pos < p.NP) {
      if (GEO1) { if (m0 + pos < p.M) off = m0 + pos; }
      else {
        const int s_ = div_prpw(pos), rem = pos - s_ * (p.PRs * p.PW);
        const int prow = div_pw(rem), pcol = rem - prow * p.PW;
        const int b = b0 + s_, sy = srow0 + prow, sx = x0 + pcol - 1 + br;
        if (b < a.B && sy >= 0 && sy < a.Hin && sx >= 0 && sx < a.Win) off = (b * a.Hin + sy) * a.Win + sx;
      }
    }
    return off;
  };
  // The compute waves build the gather / row tables while the loader waves already stream the first chunks (their per-lane
  // source offsets need no table): the first patch's memory latency overlaps the table arithmetic.
  constexpr int NTC = NCW * 64;
  if (!is_loader) {
  for (int ml = tid; ml < BMT; ml += NTC) {      // one thread per tile row: the divisions happen once, the taps are offsets
    int s_ = 0, yl = 0, x = 0, y = 0;
    if (!GEO1) {
      if (p.whole) { s_ = div_hw(ml); const int rem = ml - s_ * p.HWout; yl = div_w(rem); x = rem - yl * p.Wout; y = yl; }
      else { yl = div_w(ml); x = ml - yl * p.Wout; y = yo0 + yl; }      // (wsplit: ml < tile <= Wout, so yl = 0 and x is the tile-local column)
    }
    // (the 16x16x32 kind reads the (0, 0) row only: its taps are wave-uniform offsets from it)
#pragma unroll
    for (int tap = 0; tap < (M16 ? 1 : TAPS); ++tap) {
      int pos;
      if (GEO1) pos = ml;
      else {
        const int dy = SUBPIX ? (tap >> 1) + py : tap / 3, dx = SUBPIX ? (tap & 1) + px : tap - (tap / 3) * 3;
        int prow, pcol;
        if (a.mode == STEDM_CONV_S1 || SUBPIX) { prow = yl + dy; pcol = x + dx; }
        else { prow = ((y + dy - 1) >> 1) - srow0; pcol = ((x + dx - 1) >> 1) + 1; }
        pos = (s_ * p.PRs + prow) * p.PW + pcol;
      }
      sIdx[tap * BMT + ml] = (pos * BROW) | (M16 ? 0 : ((((pos / RPB) % CPP) ^ (IS1X1 ? 2 * tap : 0)) << 24));
    }
  }
  for (int ml = tid; ml < BMT; ml += NTC) {
    int m, b;
    if (GEO1) { m = m0 + ml; b = (IS1X1 && a.qkv_q) ? m / a.qkv_T : m0 / p.HWout + div_hw(rem0 + ml); }   // (qkv epilogue: the sample of a flat GEMM row)
    else if (!p.whole) { m = m0 + ml; b = b0; }     // a 256-row tile lies inside one image
    else { const int s_ = div_hw(ml); b = b0 + s_; m = b * p.HWout + (ml - s_ * p.HWout); }
    const bool okm = m < p.M;
    if (SUBPIX && !s2d && okm) {   // low-res pixel (b, y, x) -> output pixel (b, 2y+py, 2x+px) of the [B][2H][2W] tensor
      const int rem = m - b * p.HWout, y = div_w(rem), x = rem - y * p.Wout;
      m = (b * 2 * p.Hout + 2 * y + py) * (2 * p.Wout) + 2 * x + px;
    }
    sM[ml] = okm ? m : -1;
    sMb[ml] = b;
  }
  }
  if (is_loader) {
    // ---------------------------------------------------------------- patch stream (2 waves), up to three chunks ahead
    bool early[3] = {false, false, false};   // prologue chunks issued before the table barrier
#define WAIT_VM(N) asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory")
    const int aw = wave - NCW;
    const uint16_t* a_hi = reinterpret_cast<const uint16_t*>(a.src16_hi);
    const uint16_t* zero16 = reinterpret_cast<const uint16_t*>(g_zero_page);
    const int nslots = (nai + 1 - aw) / 2;
    constexpr int MAXS = IS1X1 ? 16 : 13;   // DMA instructions per plane and loader wave (128-B rows: 8 positions each)
    // per-lane source of every DMA slot: a full pointer (patch pixel, or the zero page for halo / padding lanes), so that issuing
    // a chunk is one 64-bit add per instruction; chunk 0 of a slot is issued the moment its pointer exists
    const uint16_t* asrc[MAXS];
    const int lpos = lane / CPP, lphys = lane % CPP;
    // P3: the lo plane of a lane's pixel lies lo_delta elements behind its hi plane; halo lanes (bit k of zmask) read the zero page twice
    const long lo_delta = P3 ? reinterpret_cast<const uint16_t*>(a.src16_lo) - a_hi : 0;
    unsigned zmask = 0;
#define LO_SRC(K) (asrc[K] + (((zmask >> (K)) & 1u) ? 0 : lo_delta))
#pragma unroll
    for (int k = 0; k < MAXS; ++k) {
      asrc[k] = zero16;
      if (k < nslots) {
        const int pos = (aw + 2 * k) * PPI + lpos;
        const int logical = M16 ? lphys : lphys ^ ((pos / RPB) % CPP);
        const int pix = patch_pixel(pos);
        asrc[k] = (pix >= 0 ? a_hi + (long)pix * p.cstride : zero16) + logical * 8;
        if (P3 && pix < 0) zmask |= 1u << k;
        if (!STEDM_DBG(p.dbg, 2)) {
#pragma unroll
          for (int pl = 0; pl < NPL; ++pl) {
            GLDS16(asrc[k] + (cbeg * NPL + pl) * (BROW / 2), sA + pl * (a_plane + pl_skew) + (aw + 2 * k) * 1024);
            if (P3) GLDS16(LO_SRC(k) + (cbeg * NPL + pl) * (BROW / 2), sA + a_half + pl * (a_plane + pl_skew) + (aw + 2 * k) * 1024);
          }
        }
      }
    }
    auto issue_a = [&](int chunk) {
      if STEDM_DBG(p.dbg, 2) return;
      unsigned char* dsta = sA + (chunk % NABUF) * a_buf;
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) {
        const int c0 = ((cbeg + chunk) * NPL + pl) * (BROW / 2);
#pragma unroll
        for (int k = 0; k < MAXS; ++k) {
          if (k < nslots) {
            GLDS16(asrc[k] + c0, dsta + pl * (a_plane + pl_skew) + (aw + 2 * k) * 1024);
            if (P3) GLDS16(LO_SRC(k) + c0, dsta + a_half + pl * (a_plane + pl_skew) + (aw + 2 * k) * 1024);
          }
        }
      }
    };
    if constexpr (P3) {
      // 3-buffer ring, one chunk in flight: chunk s+2 goes out once every compute wave is past chunk s-1 (its buffer), i.e. after barrier s,
      // and has a whole chunk (864 MFMAs per wave) to land
      if (nsteps > 1) issue_a(1);
      __syncthreads();   // tables built (pairs with the compute waves)
      WAIT_VM(0);
      __syncthreads();   // B_init: chunks 0 and 1 landed
      for (int s = 0; s < nsteps; ++s) {
        WAIT_VM(0);      // chunk s+1 landed
        __builtin_amdgcn_s_barrier();
        if (s + 2 < nsteps) issue_a(s + 2);
      }
    } else {
    early[0] = true;                      // issued slot by slot above
#pragma unroll
    for (int c = 1; c < 3; ++c)
      if (c < nsteps) { issue_a(c); early[c] = true; }
    __syncthreads();   // tables built (pairs with the compute waves)
    // fused skip phase: chunk c >= nsteps is 64 channels of the tile's own pixels (8 pixels x 128 B per DMA instruction)
    int aoff2[FUSE ? 16 : 1];
    if (FUSE) {
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int ml = (aw + 2 * k) * 8 + (lane >> 3);
        const int logical = (lane & 7) ^ ((ml >> 1) & 7);
        const int m = sM[ml];
        aoff2[k] = m >= 0 ? m * a.cb + logical * 8 : -(logical * 8) - 1;
      }
    }
    auto issue2 = [&](int c2, int ringpos) {   // chunk c2 of the fused 1x1 phase into ring slot `ringpos` (slots of a_buf bytes)
      if STEDM_DBG(p.dbg, 2) return;
      const uint16_t* b_hi = reinterpret_cast<const uint16_t*>(a.src16b_hi);
      unsigned char* dsta = sA + ringpos * a_buf;
      const int c0 = (c2beg + c2) * 64;
#pragma unroll
      for (int k = 0; k < (FUSE ? 16 : 0); ++k) {
        const int o = aoff2[k];
        const uint16_t* sh = o >= 0 ? b_hi + o + c0 : zero16 + (-o - 1) + c0;
        GLDS16(sh, dsta + (aw + 2 * k) * 1024);
      }
    };
    auto issue_any = [&](int chunk) {
      if (!FUSE || chunk < nsteps) issue_a(chunk); else issue2(chunk - nsteps, chunk % NABUF);
    };
    const int ntot = nsteps + nsteps2;
    auto wait_keep = [&](int cnt) {   // everything but the newest `cnt` DMA instructions of this wave has landed
      switch (cnt) {
        case 1: WAIT_VM(1); break; case 2: WAIT_VM(2); break; case 3: WAIT_VM(3); break; case 4: WAIT_VM(4); break;
        case 5: WAIT_VM(5); break; case 6: WAIT_VM(6); break; case 7: WAIT_VM(7); break; case 8: WAIT_VM(8); break;
        case 9: WAIT_VM(9); break; case 10: WAIT_VM(10); break; case 11: WAIT_VM(11); break; case 12: WAIT_VM(12); break;
        case 13: WAIT_VM(13); break; case 14: WAIT_VM(14); break; case 15: WAIT_VM(15); break; case 16: WAIT_VM(16); break;
        case 18: WAIT_VM(18); break; case 20: WAIT_VM(20); break; case 22: WAIT_VM(22); break; case 24: WAIT_VM(24); break;
        default: WAIT_VM(0); break;
      }
    };
    auto wait_all_but = [&](int chunk) { wait_keep((FUSE && chunk >= nsteps) ? 16 : nslots * NPL); };   // all older than `chunk` landed
    {
      if (!early[0]) issue_any(0);
      if (ntot > 1 && !early[1]) issue_any(1);
      if (ntot > 2 && !early[2]) issue_any(2);
      if (ntot > 2 && !STEDM_DBG(p.dbg, 2)) wait_all_but(2); else WAIT_VM(0);
      __syncthreads();   // B_init (pairs with the compute waves): chunks 0 and 1 landed, start-up tables consumed
      for (int s = 0; s < ntot; ++s) {
        // chunk s+1 must have landed when the compute waves pass barrier s (they read it from then on); chunk s+2 may still fly
        if STEDM_DBG(p.dbg, 4) { if (s + 1 >= ntot) WAIT_VM(0); }   // timing ablation: never wait for the patch DMA inside the loop
        else if (s + 2 < ntot && !STEDM_DBG(p.dbg, 2)) wait_all_but(s + 2); else WAIT_VM(0);
        if (!(M16 && RS_DIAG(32))) __builtin_amdgcn_s_barrier();
        // every compute wave is past chunk s-1: its buffer (= that of chunk s+3) is free
        if (s + 3 < ntot) issue_any(s + 3);
      }
    }
    }
    if (npers) return;   // the whole K is in the ring; the compute waves take it from here without another block barrier
#undef LO_SRC
#undef WAIT_VM
  } else {
    // ================================================================================= COMPUTE WAVES
    __syncthreads();   // tables built
    STAMP(1);
    STAMPC(2);
    const int wm = wave >> 1, wn = wave & 1;
    const int r = lane & 31, h = lane >> 5;
    const unsigned voff = lane * 16;
    int abuf = 0;
    const unsigned A0 = (unsigned)(uintptr_t)sA;
    if constexpr (M16) {
      // ---- 16x16x32 MFMA form: 8 row fragments of 16 pixels x 4 column fragments of 16 channels per wave
      const int r16 = lane & 15;
      unsigned aofs[1][8];
#pragma unroll
      for (int f = 0; f < 8; ++f) {
        const int e = sIdx[wm * 128 + f * 16 + r16];            // tap (0, 0) of the fragment's row: its patch position * BROW
        if (G1) aofs[0][f] = (unsigned)(e & 0xFFFFFF) + (unsigned)(lane >> 4) * 16u;      // 64-B rows: k-group g is piece g
        else aofs[0][f] = (unsigned)(e & 0xFFFFFF) + (unsigned)h * 16u + (unsigned)((lane >> 4) & 1) * (unsigned)(a_plane + pl_skew);
      }
      unsigned tapd[NS];
#pragma unroll
      for (int t = 0; t < NS; ++t)         // stride 1: pos(tap) = pos(0,0) + dy * PW + dx (3x3: 3 x 3 taps; sub-pixel / space-to-depth: 2 x 2)
        tapd[t] = G1 ? 0u : (SUBM ? (unsigned)((t >> 1) * p.PW + (t & 1)) * 32u : (unsigned)((t / 3) * p.PW + (t % 3)) * 32u);
      // weight fragment stream: sub-step g = chunk * 9 + tap at wq + g * 8192, this wave's 4 column fragments at + wn * 4096
      const unsigned char* wq = reinterpret_cast<const unsigned char*>(a.w_frag16) +
                                (((((size_t)parity * p.tiles_n + tile_n) * nchunks_w + cbeg) * NS) * 8 + wn * 4) * 1024;
      f32x4 acc[8][4];
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[i][j][e] = 0.f;
      if constexpr (P3) {
        const size_t wlo = (size_t)((SUBPIX && !s2d) ? 4 : 1) * p.tiles_n * nchunks_all * NS * 8 * 1024;    // bytes of the hi fragment stream: the lo stream follows it
        rs_phase16_p3<T, NS, 2>(acc, aofs[0], tapd, A0, a_buf, (unsigned)a_half, abuf, nsteps, wq, wlo, voff);
      } else
      rs_phase16<T, NS, 1, true>(acc, aofs, tapd, A0, a_buf, abuf, nsteps, wq, voff, p.dbg);
      if (FUSE) {
        // 1x1 phase on the same MFMA shape: row ml of a chunk is pixel ml of the tile (128 B = 64 channels, 16-B pieces XOR-swizzled by
        // (ml >> 1) & 7); sub-step s = channels 32 s .. 32 s + 31, k-group g = piece 4 s + g (natural order: the 8 rows a ds_read_b128
        // group takes from k-group 2q and the 8 it takes from 2q + 1 then sit on disjoint 16-B slots)
        unsigned aofs2[2][8];
#pragma unroll
        for (int sl = 0; sl < 2; ++sl)
#pragma unroll
          for (int f = 0; f < 8; ++f) {
            const unsigned ml = wm * 128 + f * 16 + r16;
            aofs2[sl][f] = ml * 128 + ((((unsigned)(4 * sl) + (unsigned)(lane >> 4)) ^ ((ml >> 1) & 7)) << 4);
          }
        const unsigned tapd2[2] = {0u, 0u};
        const unsigned char* wq2 = reinterpret_cast<const unsigned char*>(a.w_frag_b16) + ((((size_t)tile_n * nsteps2_all + c2beg) * 2) * 8 + wn * 4) * 1024;
        rs_phase16<T, 2, 2, false>(acc, aofs2, tapd2, A0, a_buf, abuf, nsteps2, wq2, voff);
      }
      __syncthreads();   // #3: every wave is past the main loop, the patch buffers become the fp32 staging tile
      STAMP(3);
      STAMPC(7);
      if (!STEDM_DBG(p.dbg, 64)) {
        const int g4 = lane >> 4;
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float* dst = sStage + (wm * 128 + i * 16 + g4 * 4) * SST + wn * 64 + j * 16 + r16;   // C/D: col = lane & 15, row = 4 (lane >> 4) + e
#pragma unroll
            for (int e = 0; e < 4; ++e) dst[e * SST] = acc[i][j][e];
          }
      }
    } else {
    unsigned aofs[TAPS][WM];
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
      for (int i = 0; i < WM; ++i) {
        const int e = sIdx[t * BMT + wm * (WM * 32) + i * 32 + r];
        aofs[t][i] = (unsigned)(e & 0xFFFFFF) + ((((unsigned)e >> 24) ^ (unsigned)h) << 4);
      }
    // weight fragment stream: sub-step g = chunk*NS + s lives at wq + g*4096 B (+1024 for the second fragment)
    const unsigned char* wq = reinterpret_cast<const unsigned char*>(a.w_frag) +
                              ((((size_t)parity * p.tiles_n + tile_n) * nchunks_w + cbeg) * NS * 4 + wn * 2) * 1024;

    f32x16 acc[WM][2];
    if constexpr (NPERS) {
      {
        // ---- N-persistent form. A short-K GEMM (K <= 256: the set-ViT's to_qkv / FeedForward Linears, vit_set.py:23-31, 52) is all prologue
        // and epilogue per 256 x 128 tile (measured: tables 4.6 us + loop 4.3 us + staging / stores 5 - 12 us, one block per CU, nothing
        // overlapped). Here the block keeps its 256 rows x K in the ring and the compute waves walk the N-tiles on their own: the first
        // tile runs the usual chunk protocol with the loader waves, every later one re-reads the resident chunks without barriers, and each
        // wave stores its 128 x 64 block straight from the accumulators (fp32: 128-B runs; 16-bit: 64-B runs that the next column block
        // completes) while the other waves are in their MFMA loops. v tiles of the qkv epilogue are computed transposed (SWAP): a lane then
        // holds one token's column and consecutive lanes write consecutive tokens of a v^T row.
        // Stores and residual loads go through buffer descriptors: 32-bit per-lane byte offsets, and the hardware range check drops the rows
        // of the last M-tile that lie beyond M (their offsets are >= the tensor's size: row-major outputs by m >= M, the attention planes by
        // sample index = nb) — no predicate, no branch per element (cdna_hip_programming.md T8; sizes < 2^32 bytes are a host-side condition).
        const unsigned N = (unsigned)a.cout;
        const int HD = a.qkv_heads * 64, Tn = a.qkv_T;
        const unsigned Tp = (unsigned)a.qkv_Tp;
        const unsigned esz = a.out ? 4u : 2u;
        // (timing ablation STEDM_CONV_DBG & 2048: zero-record descriptors, the range check drops every store / residual load of the epilogue)
        const unsigned out_bytes = STEDM_DBG(p.dbg, 2048) ? 0u : (unsigned)p.M * N * esz;
        const unsigned pl_bytes = (a.qkv_q && !STEDM_DBG(p.dbg, 2048)) ? (unsigned)(p.M / Tn) * (unsigned)HD * Tp * 2u : 0u;
        const auto rs_out = __builtin_amdgcn_make_buffer_rsrc(a.out ? (void*)a.out : a.out16_hi, 0, out_bytes, 0x00020000);
        const auto rs_res = __builtin_amdgcn_make_buffer_rsrc((void*)a.res, 0, a.res ? out_bytes : 0u, 0x00020000);
        const auto rs_q = __builtin_amdgcn_make_buffer_rsrc(a.qkv_q, 0, pl_bytes, 0x00020000);
        const auto rs_k = __builtin_amdgcn_make_buffer_rsrc(a.qkv_k, 0, pl_bytes, 0x00020000);
        const auto rs_v = __builtin_amdgcn_make_buffer_rsrc(a.qkv_vt, 0, pl_bytes, 0x00020000);
        const bool has_res = a.res != nullptr, gelu = a.act_out == 2;
        const float* __restrict__ bp = a.bias ? a.bias : reinterpret_cast<const float*>(g_zero_page);   // (no bias: zeros, no branch per element)
        static_assert(STEDM_ZERO_PAGE_BYTES >= 4 * 8192, "the zero page stands in for a missing bias of up to 8192 channels");
        unsigned bad16 = 0u;
        const int rl0 = wm * 128 + 4 * h;            // first tile row of this lane's accumulator rows (block i adds 32 i, element e adds 8 (e >> 2) + (e & 3))
        const int tn_first = tile_n, tn_end = tile_n + p.tiles_n / p.npers;
        for (int tn = tn_first; tn < tn_end; ++tn) {
          const int n0t = tn * BN;
#pragma unroll
          for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
              for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
          const unsigned char* wqt = reinterpret_cast<const unsigned char*>(a.w_frag) + (((size_t)tn * nchunks_all) * NS * 4 + wn * 2) * 1024;
          const int sec = a.qkv_q ? n0t / HD : 0;
          abuf = 0;
          if (tn == tn_first) rs_phase<T, WM, NS, NTAB, true, true>(acc, aofs, A0, a_buf, a_plane, abuf, nsteps, wqt, voff, p.dbg);   // (never a v tile: host)
          else if (sec == 2) rs_phase<T, WM, NS, NTAB, false, true, true, true>(acc, aofs, A0, a_buf, a_plane, abuf, nsteps, wqt, voff, p.dbg);
          else rs_phase<T, WM, NS, NTAB, false, true, true, false>(acc, aofs, A0, a_buf, a_plane, abuf, nsteps, wqt, voff, p.dbg);
          if (a.qkv_q) {
            if (sec == 2) {
              // acc[i][j][e] = v[token wm * 128 + 32 i + r][channel n0t + wn * 64 + 32 j + 4 h + 8 (e >> 2) + (e & 3)]
              // 16-bit stores go out as dwords: lanes 2k / 2k + 1 (tokens 2k, 2k + 1: same sample, t even) trade one of every two channels, the
              // even lane then holds both tokens of channel c, the odd lane both of c + 1 (2-byte stores ran the epilogue at a third of the rate)
              const int cb = n0t - 2 * HD + wn * 64 + 4 * h + (lane & 1);
              const bool odd = lane & 1;
#pragma unroll
              for (int i = 0; i < WM; ++i) {
                __builtin_amdgcn_sched_barrier(0);
                const int rl = wm * 128 + i * 32 + (r & ~1), m = m0 + rl;
                const int b = sMb[rl], t = m - b * Tn;
                const unsigned o0 = (((unsigned)b * (unsigned)HD + (unsigned)cb) * Tp + (unsigned)t) * 2u;
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                  for (int e = 0; e < 16; e += 2) {
                    const int c = j * 32 + 8 * (e >> 2) + (e & 3);
                    const float a0 = acc[i][j][e] + bp[n0t + wn * 64 + 4 * h + c], a1 = acc[i][j][e + 1] + bp[n0t + wn * 64 + 4 * h + c + 1];
                    const float recv = rs_lane_xor1(odd ? a0 : a1);
                    const unsigned pk = rs_pack2<T>(odd ? recv : a0, odd ? a1 : recv);
                    __builtin_amdgcn_raw_buffer_store_b32(pk, rs_v, o0 + (unsigned)c * Tp * 2u, 0, 0);
                    bad16 |= f16_over2<T>(pk);
                  }
              }
            } else {
              const float sc = sec == 0 ? a.qkv_qscale : 1.0f;
              const auto rs_qk = sec == 0 ? rs_q : rs_k;
              // dword stores: lanes 2k / 2k + 1 trade their column-block values, the even lane then holds columns 2k, 2k + 1 of block 0, the odd
              // lane those of block 1 (32 + 2k, 33 + 2k): 32 lanes write the 128 contiguous bytes of one head's row
              const bool odd = lane & 1;
              const int cl = n0t - sec * HD + wn * 64 + (odd ? 32 : 0) + (r & ~1);          // first of the lane's two columns inside the q / k block
              const float b0 = bp[n0t + wn * 64 + (odd ? 32 : 0) + (r & ~1)], b1 = bp[n0t + wn * 64 + (odd ? 32 : 0) + (r & ~1) + 1];
              const unsigned ocol = (unsigned)(cl >> 6) * Tp * 128u + (unsigned)(cl & 63) * 2u;
#pragma unroll
              for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                  __builtin_amdgcn_sched_barrier(0);
                  const int rl = rl0 + i * 32 + 8 * q4;
                  const int4 b4 = *reinterpret_cast<const int4*>(sMb + rl);
                  const int bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                  for (int u = 0; u < 4; ++u) {
                    const int t = m0 + rl + u - bb[u] * Tn;
                    const unsigned orow = ((unsigned)bb[u] * (unsigned)a.qkv_heads * Tp + (unsigned)t) * 128u;      // row t of head 0 of sample b
                    const float a0 = acc[i][0][4 * q4 + u], a1 = acc[i][1][4 * q4 + u];
                    const float recv = rs_lane_xor1(odd ? a0 : a1);
                    const unsigned pk = rs_pack2<T>(((odd ? recv : a0) + b0) * sc, ((odd ? a1 : recv) + b1) * sc);
                    __builtin_amdgcn_raw_buffer_store_b32(pk, rs_qk, orow + ocol, 0, 0);
                    bad16 |= f16_over2<T>(pk);
                  }
                }
            }
          } else if (a.out) {
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
              for (int j = 0; j < 2; ++j) {
                __builtin_amdgcn_sched_barrier(0);      // one 32 x 32 block at a time: its 16 residual loads, then its 16 stores
                const unsigned col = (unsigned)(n0t + wn * 64 + j * 32 + r);
                const bool cv = col < N;                  // (a ragged last N-tile: offsets from 2^31 on are beyond every admitted tensor -> dropped)
                const float bsv = bp[cv ? col : 0u];
                const unsigned o0 = cv ? ((unsigned)(m0 + rl0 + i * 32) * N + col) * 4u : 0x80000000u;
                float rv[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) rv[e] = 0.f;
                if (has_res) {
#pragma unroll
                  for (int e = 0; e < 16; ++e)
                    rv[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_res, o0 + (unsigned)(8 * (e >> 2) + (e & 3)) * N * 4u, 0, 0));
                }
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                  float v = acc[i][j][e] + bsv;
                  if (has_res) v += rv[e];
                  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rs_out, o0 + (unsigned)(8 * (e >> 2) + (e & 3)) * N * 4u, 0, 0);
                }
              }
          } else {
            auto store16 = [&](auto with_gelu) {
              const bool odd = lane & 1;
              const unsigned col = (unsigned)(n0t + wn * 64 + (odd ? 32 : 0) + (r & ~1));      // (dword stores: see the q / k planes above)
              const bool cv = col < N;                    // (ragged last N-tile; N is even, so a lane's two columns are in or out together)
              const float b0 = bp[cv ? col : 0u], b1 = bp[cv ? col + 1 : 0u];
#pragma unroll
              for (int i = 0; i < WM; ++i) {
                __builtin_amdgcn_sched_barrier(0);
                const unsigned o0 = cv ? ((unsigned)(m0 + rl0 + i * 32) * N + col) * 2u : 0x80000000u;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                  const float a0 = acc[i][0][e], a1 = acc[i][1][e];
                  const float recv = rs_lane_xor1(odd ? a0 : a1);
                  const float v0 = (odd ? recv : a0) + b0, v1 = (odd ? a1 : recv) + b1;
                  const unsigned pk = decltype(with_gelu)::value ? rs_pack2<T>(gelu_erf_f(v0), gelu_erf_f(v1)) : rs_pack2<T>(v0, v1);
                  __builtin_amdgcn_raw_buffer_store_b32(pk, rs_out, o0 + (unsigned)(8 * (e >> 2) + (e & 3)) * N * 2u, 0, 0);
                  bad16 |= f16_over2<T>(pk);
                }
              }
            };
            if (gelu) store16(std::true_type{}); else store16(std::false_type{});
          }
        }
        f16_guard_commit(p.ovf, bad16, STEDM_F16G_CONV_OUT16);
        return;
      }
    }
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    rs_phase<T, WM, NS, NTAB, true, !IS3X3>(acc, aofs, A0, a_buf, a_plane, abuf, nsteps, wq, voff, p.dbg);
    if (FUSE) {
      // 1x1 phase: row ml of the chunk is pixel ml of the tile, 128 B; slice s of lane half h is piece (2s ^ swizzle) ^ h
      unsigned aofs2[4][WM];
#pragma unroll
      for (int sl = 0; sl < 4; ++sl)
#pragma unroll
        for (int i = 0; i < WM; ++i) {
          const unsigned ml = wm * (WM * 32) + i * 32 + r;
          aofs2[sl][i] = ml * 128 + ((((2 * sl) ^ ((ml >> 1) & 7)) ^ (unsigned)h) << 4);
        }
      const unsigned char* wq2 = reinterpret_cast<const unsigned char*>(a.w_frag_b) + ((((size_t)tile_n * nsteps2_all + c2beg) * 4) * 4 + wn * 2) * 1024;
      rs_phase<T, WM, 4, 4, false>(acc, aofs2, A0, a_buf, 0, abuf, nsteps2, wq2, voff);
    }
    __syncthreads();   // #3: every wave is past the main loop, the patch buffers become the fp32 staging tile
    STAMP(3);
    STAMPC(7);
    if (IS1X1 && a.qkv_q && n0 >= 2 * a.qkv_heads * 64) {
      // qkv epilogue, a tile of v columns: staged TRANSPOSED, [128 channels][kStageStrideT] with the tile's 256 tokens along a row (an
      // accumulator's four consecutive rows are one 16-B write; pitch 260 floats: 8 lanes = 8 channels cover the 32 banks)
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          float* dst = sStage + (wn * 64 + j * 32 + r) * kStageStrideT + wm * (WM * 32) + i * 32 + 4 * h;
#pragma unroll
          for (int q4 = 0; q4 < 4; ++q4)
            *reinterpret_cast<float4*>(dst + 8 * q4) = make_float4(acc[i][j][4 * q4], acc[i][j][4 * q4 + 1], acc[i][j][4 * q4 + 2], acc[i][j][4 * q4 + 3]);
        }
    } else
    if (!STEDM_DBG(p.dbg, 64)) {
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          float* dst = sStage + (wm * (WM * 32) + i * 32 + 4 * h) * SST + wn * 64 + j * 32 + r;
#pragma unroll
          for (int e = 0; e < 16; ++e) dst[((e & 3) + 8 * (e >> 2)) * SST] = acc[i][j][e];
        }
    }
    }
  }
  if (is_loader) __syncthreads();   // #3 (loader side)
  if STEDM_DBG(p.dbg, 64) return;
  __syncthreads();   // #4: tile staged
  STAMP(5);

  // ---- store phase, all waves: one 512-B row per 32 lanes; optional per-channel statistics of the stored values
  const bool vec_ok = (a.cout & 3) == 0;
  const int c4 = tid & 31, rg = tid >> 5;
  const int n = n0 + c4 * 4;
  const bool active = n < a.cout;
  const int nv = !active ? 0 : (vec_ok ? 4 : (a.cout - n < 4 ? a.cout - n : 4));
  float bv[4] = {0.f, 0.f, 0.f, 0.f};
  if (a.bias && !split) for (int u = 0; u < nv; ++u) bv[u] = a.bias[n + u];
  if (FUSE && a.bias_b && !split) for (int u = 0; u < nv; ++u) bv[u] += a.bias_b[n + u];     // (split: both biases are the reduce pass's)
  // LayerNorm epilogue (stedm_conv_args.ln_*): the tile holds whole output rows (cout <= 128, one N-tile), 32 lanes x 4 channels own a row:
  // mean and centred variance by butterflies inside the half-wave, then (v - mean) * rstd * gamma + beta (+ ln_res), fp32 and / or 16-bit
  if constexpr (IS1X1 && !NPERS) {
    if (a.ln_gamma) {
      typedef T V4T __attribute__((ext_vector_type(4)));
      const int c4l = tid & 31, nl = c4l * 4;
      const bool act = nl < a.cout;
      float4 gm = make_float4(0.f, 0.f, 0.f, 0.f), bt = gm, bs = gm;
      if (act) {
        gm = *reinterpret_cast<const float4*>(a.ln_gamma + nl); bt = *reinterpret_cast<const float4*>(a.ln_beta + nl);
        if (a.bias) bs = *reinterpret_cast<const float4*>(a.bias + nl);
      }
      const float inv_dim = 1.0f / (float)a.cout;
      const float* __restrict__ lres = a.ln_res;
      float* __restrict__ outp = a.out;
      T* __restrict__ o16 = reinterpret_cast<T*>(a.out16_hi);
      unsigned bad16 = 0u;
      // four rows per pass: their residual loads and the four pairs of butterflies are independent chains the scheduler interleaves
      constexpr int RB = 4;
      for (int row0 = tid >> 5; row0 < BMT; row0 += RB * (NT / 32)) {
        int mm[RB];
        float4 r4[RB], v[RB];
        float s1[RB], s2[RB];
#pragma unroll
        for (int k = 0; k < RB; ++k) {
          const int row = row0 + k * (NT / 32);
          mm[k] = row < BMT ? sM[row] : -1;             // (the same for the 32 lanes of a row)
          r4[k] = make_float4(0.f, 0.f, 0.f, 0.f); v[k] = r4[k];
          if (mm[k] >= 0 && act) {
            if (lres) r4[k] = *reinterpret_cast<const float4*>(lres + (long)mm[k] * a.cout + nl);
            v[k] = *reinterpret_cast<const float4*>(sStage + row * SST + nl);
            v[k].x += bs.x; v[k].y += bs.y; v[k].z += bs.z; v[k].w += bs.w;
          }
          s1[k] = (v[k].x + v[k].y) + (v[k].z + v[k].w);
        }
#pragma unroll
        for (int ofs = 16; ofs > 0; ofs >>= 1)
#pragma unroll
          for (int k = 0; k < RB; ++k) s1[k] += __shfl_xor(s1[k], ofs, 64);
#pragma unroll
        for (int k = 0; k < RB; ++k) {
          const float mean = s1[k] * inv_dim;
          v[k].x = act ? v[k].x - mean : 0.f; v[k].y = act ? v[k].y - mean : 0.f; v[k].z = act ? v[k].z - mean : 0.f; v[k].w = act ? v[k].w - mean : 0.f;
          s2[k] = (v[k].x * v[k].x + v[k].y * v[k].y) + (v[k].z * v[k].z + v[k].w * v[k].w);
        }
#pragma unroll
        for (int ofs = 16; ofs > 0; ofs >>= 1)
#pragma unroll
          for (int k = 0; k < RB; ++k) s2[k] += __shfl_xor(s2[k], ofs, 64);
#pragma unroll
        for (int k = 0; k < RB; ++k) {
          if (mm[k] < 0 || !act) continue;
          const float rstd = 1.0f / sqrtf(s2[k] * inv_dim + a.ln_eps);
          const long o = (long)mm[k] * a.cout + nl;
          const float w0 = v[k].x * rstd * gm.x + bt.x + r4[k].x, w1 = v[k].y * rstd * gm.y + bt.y + r4[k].y;
          const float w2 = v[k].z * rstd * gm.z + bt.z + r4[k].z, w3 = v[k].w * rstd * gm.w + bt.w + r4[k].w;
          if (outp) *reinterpret_cast<float4*>(outp + o) = make_float4(w0, w1, w2, w3);
          if (o16) {
            V4T h4; h4[0] = (T)w0; h4[1] = (T)w1; h4[2] = (T)w2; h4[3] = (T)w3;
            *reinterpret_cast<V4T*>(o16 + o) = h4;
            bad16 |= f16_over_v4<T>(h4);
          }
        }
      }
      f16_guard_commit(p.ovf, bad16, STEDM_F16G_NORM);
      return;
    }
  }
  // qkv epilogue (stedm_conv_args.qkv_*; vit_set.py:52-57): the tile's 128 columns are two heads of q, k or v (heads * 64 is a multiple of 128).
  // q (scaled) and k: the lean row loop below with the rows scattered to [sample * heads + head][t][64] (a row's 64 channels of a head are
  // 128 contiguous bytes); v: from the transposed staging, a lane takes two consecutive tokens of one channel -> one 4-B store, a wave 256
  // contiguous bytes of a [sample * heads + head][channel][Tp] row (T even: a row pair never straddles two samples and t is even).
  if constexpr (IS1X1) {
    if (a.qkv_q) {
      typedef T V8T __attribute__((ext_vector_type(8)));
      typedef T V2T __attribute__((ext_vector_type(2)));
      const int H = a.qkv_heads, HD = H * 64, sec = n0 / HD, Tn = a.qkv_T;
      const long Tp = a.qkv_Tp;
      unsigned bad16 = 0u;
      if (sec < 2) {
        const int c8 = tid & 15, nl = n0 - sec * HD + c8 * 8, hd = nl >> 6, d0 = nl & 63;
        const float sc = sec == 0 ? a.qkv_qscale : 1.0f;
        float b8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) b8[u] = a.bias ? a.bias[n0 + c8 * 8 + u] : 0.f;
        T* __restrict__ dstp = reinterpret_cast<T*>(sec == 0 ? a.qkv_q : a.qkv_k);
#pragma unroll 2
        for (int row = tid >> 4; row < BMT; row += NT / 16) {
          const int m = sM[row];
          if (m < 0) continue;
          const int b = sMb[row], t = m - b * Tn;
          const float4 x0 = *reinterpret_cast<const float4*>(sStage + row * SST + c8 * 8);
          const float4 x1 = *reinterpret_cast<const float4*>(sStage + row * SST + c8 * 8 + 4);
          const float v[8] = {x0.x + b8[0], x0.y + b8[1], x0.z + b8[2], x0.w + b8[3], x1.x + b8[4], x1.y + b8[5], x1.z + b8[6], x1.w + b8[7]};
          V8T h8;
#pragma unroll
          for (int u = 0; u < 8; ++u) h8[u] = (T)(v[u] * sc);
          *reinterpret_cast<V8T*>(dstp + (((long)b * H + hd) * Tp + t) * 64 + d0) = h8;
          const uint4 hb = __builtin_bit_cast(uint4, h8);
          bad16 |= f16_over2<T>(hb.x) | f16_over2<T>(hb.y) | f16_over2<T>(hb.z) | f16_over2<T>(hb.w);
        }
      } else {
        long o[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          const int row = 2 * (hf * 64 + lane), m = sM[row];
          o[hf] = m < 0 ? -1 : (long)sMb[row] * HD * Tp + (m - sMb[row] * Tn);
        }
        T* __restrict__ vt = reinterpret_cast<T*>(a.qkv_vt);
        for (int d = tid >> 6; d < 128; d += NT / 64) {
          const int nl = n0 - 2 * HD + d;               // (head, channel) = (nl >> 6, nl & 63): row nl of the sample's [heads * 64][Tp] block
          const float bs = a.bias ? a.bias[n0 + d] : 0.f;
#pragma unroll
          for (int hf = 0; hf < 2; ++hf) {
            if (o[hf] < 0) continue;
            const float2 x = *reinterpret_cast<const float2*>(sStage + d * kStageStrideT + 2 * (hf * 64 + lane));
            V2T h2; h2[0] = (T)(x.x + bs); h2[1] = (T)(x.y + bs);
            *reinterpret_cast<V2T*>(vt + o[hf] + (long)nl * Tp) = h2;
            bad16 |= f16_over2<T>(__builtin_bit_cast(unsigned, h2));
          }
        }
      }
      f16_guard_commit(p.ovf, bad16, STEDM_F16G_CONV_OUT16);
      return;
    }
  }
  // 16-bit-only output (a GEMM whose consumer reads operand planes: qkv / fc1 of the transformer blocks): lean loop, 8 channels and one
  // 16-B store per lane, bias and the optional GELU applied on the way
  if (!split && !a.out && a.out16_hi && !a.out16_lo && !a.res && !a.emb && !a.chan_stats && (a.cout & 7) == 0) {
    typedef T V8T __attribute__((ext_vector_type(8)));
    const int c8 = tid & 15, n8 = n0 + c8 * 8;
    if (n8 < a.cout) {
      float b8[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) b8[u] = (a.bias ? a.bias[n8 + u] : 0.f) + ((FUSE && a.bias_b) ? a.bias_b[n8 + u] : 0.f);
      const bool gelu = a.act_out == 2;
      T* __restrict__ o16 = reinterpret_cast<T*>(a.out16_hi);
      unsigned bad16 = 0u;      // fp16 range guard (common.hpp)
#pragma unroll 2
      for (int row = tid >> 4; row < BMT; row += NT / 16) {
        const int m = sM[row];
        if (m < 0) continue;
        const float4 x0 = *reinterpret_cast<const float4*>(sStage + row * SST + c8 * 8);
        const float4 x1 = *reinterpret_cast<const float4*>(sStage + row * SST + c8 * 8 + 4);
        float v[8] = {x0.x + b8[0], x0.y + b8[1], x0.z + b8[2], x0.w + b8[3], x1.x + b8[4], x1.y + b8[5], x1.z + b8[6], x1.w + b8[7]};
        V8T h8;
#pragma unroll
        for (int u = 0; u < 8; ++u) h8[u] = (T)(gelu ? gelu_erf_f(v[u]) : v[u]);
        *reinterpret_cast<V8T*>(o16 + (long)m * (a.out16_stride ? a.out16_stride : a.cout) + n8) = h8;
        const uint4 hb = __builtin_bit_cast(uint4, h8);
        bad16 |= f16_over2<T>(hb.x) | f16_over2<T>(hb.y) | f16_over2<T>(hb.z) | f16_over2<T>(hb.w);
      }
      f16_guard_commit(p.ovf, bad16, STEDM_F16G_CONV_OUT16);
    }
    return;
  }
  float* sPart = sStage + BMT * SST;                 // [NT/32 row groups][128 channels][2]
  float* sCh = sPart + (NT / 32) * 128 * 2;          // gn_tile: [128 channels][2] totals of the current sample, then [32 groups][2] mean / rstd
  float* sGm = sCh + 128 * 2;
  const int coop = p.gn_coop;                        // 2 .. 4: this tile is one of `coop` tiles of a sample that exchange their channel sums (below)
  const bool gn_t = p.gn_tile != 0 || coop != 0;     // block-uniform: whole samples x whole groups in this tile, fast path (host-checked)
  float* sAll = sGm + 32 * 2;                        // coop: [4 tiles][128 channels][2] sums of the sample
  const bool keep_out = !(gn_t && a.gn_only);        // gn_only: the planes below are the only consumer of these values
  // rows of one sample in this tile. The 3x3 geometries guarantee that samples and tiles align (conv_geometry); a 1x1 takes any H * W:
  // when neither divides the other (`ragged`: 10 x 10 = 100 pixels: 2.56 samples per tile) the tile is ONE run of 256 rows whose samples
  // change inside it - no per-sample statistics (the host routes them to the dispatcher's pass), the embedding row is looked up per row.
  // (Round 4 cut the tile into floor(256 / HW) samples and never stored the rows behind them: found by the round-5 test of ADVICE r04's case.)
  const bool ragged = p.HWout % BMT != 0 && BMT % p.HWout != 0;
  const int rows_per = (p.HWout < BMT && !ragged) ? p.HWout : BMT;
  const int nsub = BMT / rows_per;
  unsigned bad16 = 0u, badn = 0u;      // fp16 range guard: 16-bit side output / GroupNorm planes (common.hpp)
  for (int sub = 0; sub < nsub; ++sub) {
    float cs[4] = {0.f, 0.f, 0.f, 0.f}, cq[4] = {0.f, 0.f, 0.f, 0.f};
    // fast path (the common case: fp32 output, cout % 4 == 0, no split, no 16-bit side output): a lean row loop; the embedding row is
    // the same for every row of this `sub` (one sample) and is fetched once; same operation order as the generic loop below
    // (round 5: also the 16-bit-only form - out == NULL, out16_hi [+ out16_stride] - of a tensor whose only readers take 16-bit values: the
    //  generic loop below ran that form 2.4x slower per tile than this one runs the fp32 store, with half the bytes)
    const bool only16 = !a.out && a.out16_hi && !a.out16_lo;
    const bool fast = vec_ok && !split && (a.out ? !a.out16_hi : only16) && !a.act_out && !(ragged && a.emb);
    if (active && fast) {
      float ev[4] = {0.f, 0.f, 0.f, 0.f};
      const int rfirst = sub * rows_per;
      if (a.emb && sM[rfirst] >= 0) {   // a masked first row means the whole sample lies beyond the batch
        const float* ep = a.emb + (long)sMb[rfirst] * a.emb_bstride + n;
#pragma unroll
        for (int u = 0; u < 4; ++u) ev[u] = ep[u];
      }
      const bool has_emb = a.emb != nullptr;
      // (res_bmod: the sample of this `sub` reads the residual rows of sample b % res_bmod - one block-uniform pointer shift)
      const int rb_ = a.res_bmod ? __builtin_amdgcn_readfirstlane(sMb[rfirst]) : 0;
      const float* __restrict__ resp = a.res_bmod ? a.res - (long)(rb_ - rb_ % a.res_bmod) * p.HWout * a.cout : a.res;
      // (res2, the plain 3x3 kinds: a second residual behind the same shift; the row's residual is res + res2, added as one value)
      const float* __restrict__ resp2 = (RES2 && a.res2) ? a.res2 + (resp - a.res) : nullptr;
      float* __restrict__ outp = a.out;
      typedef T V4T16 __attribute__((ext_vector_type(4)));
      T* __restrict__ o16p = only16 ? reinterpret_cast<T*>(a.out16_hi) : nullptr;
      const long ostr16 = a.out16_stride ? a.out16_stride : a.cout;
      // (the residual rows of RB consecutive iterations are fetched before the first is used: with two in flight per thread the phase was
      // bound by the load latency, 21 us per tile of 256 KB on the set-ViT's residual GEMMs; same operation order per element)
      constexpr int RB = 8;
      for (int row0 = rfirst + rg; row0 < rfirst + rows_per; row0 += RB * (NT / 32)) {
        int mm[RB];
        float4 r4[RB];
#pragma unroll
        for (int k = 0; k < RB; ++k) {
          const int row = row0 + k * (NT / 32);
          mm[k] = row < rfirst + rows_per ? sM[row] : -1;
          r4[k] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (resp && mm[k] >= 0) r4[k] = *reinterpret_cast<const float4*>(resp + (long)mm[k] * a.cout + n);
        }
        if (RES2 && resp2) {
#pragma unroll
          for (int k = 0; k < RB; ++k)
            if (mm[k] >= 0) {
              const float4 s4 = *reinterpret_cast<const float4*>(resp2 + (long)mm[k] * a.cout + n);
              r4[k].x += s4.x; r4[k].y += s4.y; r4[k].z += s4.z; r4[k].w += s4.w;
            }
        }
#pragma unroll
        for (int k = 0; k < RB; ++k) {
          const int row = row0 + k * (NT / 32), m = mm[k];
          if (m < 0) continue;
          const float4 v4 = *reinterpret_cast<const float4*>(sStage + row * SST + c4 * 4);
          const long o = (long)m * a.cout + n;
          float v[4] = {v4.x + bv[0], v4.y + bv[1], v4.z + bv[2], v4.w + bv[3]};
          if (has_emb) { v[0] += ev[0]; v[1] += ev[1]; v[2] += ev[2]; v[3] += ev[3]; }
          if (resp) { v[0] += r4[k].x; v[1] += r4[k].y; v[2] += r4[k].z; v[3] += r4[k].w; }
          if (keep_out && outp) *reinterpret_cast<float4*>(outp + o) = make_float4(v[0], v[1], v[2], v[3]);
          if (o16p) {
            V4T16 h4;
#pragma unroll
            for (int u = 0; u < 4; ++u) h4[u] = (T)v[u];
            *reinterpret_cast<V4T16*>(o16p + (long)m * ostr16 + n) = h4;
            bad16 |= f16_over_v4<T>(h4);
          }
          if (gn_t) *reinterpret_cast<float4*>(sStage + row * SST + c4 * 4) = make_float4(v[0], v[1], v[2], v[3]);   // final values: read again below
#pragma unroll
          for (int u = 0; u < 4; ++u) { cs[u] += v[u]; cq[u] += v[u] * v[u]; }
        }
      }
    } else
    if (active) {
      for (int row = sub * rows_per + rg; row < (sub + 1) * rows_per; row += NT / 32) {
        const int m = sM[row];
        if (m < 0) continue;
        const float4 v4 = *reinterpret_cast<const float4*>(sStage + row * SST + c4 * 4);
        float v[4] = {v4.x + bv[0], v4.y + bv[1], v4.z + bv[2], v4.w + bv[3]};
        const long o = (long)m * a.cout + n;
        if (split) {   // raw partial tile; cout % 4 == 0 is a condition of the split
          // (sub-pixel form: `o` is a pixel of the full-resolution output, a partial plane holds 4 M rows)
          *reinterpret_cast<float4*>(a.ws + (long)kz * p.M * ((SUBPIX && !s2d) ? 4 : 1) * a.cout + o) = v4;
          continue;
        }
        if (a.emb) {
          const float* ep = a.emb + (long)sMb[row] * a.emb_bstride + n;
          for (int u = 0; u < nv; ++u) v[u] += ep[u];
        }
        if (a.res) {
          const long ro = a.res_bmod ? o - (long)(sMb[row] - sMb[row] % a.res_bmod) * p.HWout * a.cout : o;     // (the rows of sample b % res_bmod)
          if (RES2 && a.res2) {      // (t = res + res2, then v += t; the host admits res2 with cout % 4 == 0 only)
            const float4 r4 = *reinterpret_cast<const float4*>(a.res + ro), s4 = *reinterpret_cast<const float4*>(a.res2 + ro);
            v[0] += r4.x + s4.x; v[1] += r4.y + s4.y; v[2] += r4.z + s4.z; v[3] += r4.w + s4.w;
          } else
          if (vec_ok) { const float4 r4 = *reinterpret_cast<const float4*>(a.res + ro); v[0] += r4.x; v[1] += r4.y; v[2] += r4.z; v[3] += r4.w; }
          else for (int u = 0; u < nv; ++u) v[u] += a.res[ro + u];
        }
        if (a.act_out == 2) {   // exact GELU (nn.GELU default), as the LDS kernels' epilogue
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = gelu_erf_f(v[u]);
        }
        if (a.out) {
          if (vec_ok) *reinterpret_cast<float4*>(a.out + o) = make_float4(v[0], v[1], v[2], v[3]);
          else for (int u = 0; u < nv; ++u) a.out[o + u] = v[u];
        }
        if (a.out16_hi) {
          typedef T V4T __attribute__((ext_vector_type(4)));
          if (vec_ok) {   // 8-B stores (out16_stride: into channels [0, cout) of a wider plane; the host admits it with cout % 4 == 0 only)
            V4T h4, l4;
#pragma unroll
            for (int u = 0; u < 4; ++u) { h4[u] = (T)v[u]; l4[u] = (T)(v[u] - (float)h4[u]); }
            *reinterpret_cast<V4T*>(reinterpret_cast<T*>(a.out16_hi) + (a.out16_stride ? (long)m * a.out16_stride + n : o)) = h4;
            bad16 |= f16_over_v4<T>(h4);
            if (a.out16_lo) *reinterpret_cast<V4T*>(reinterpret_cast<T*>(a.out16_lo) + o) = l4;
          } else {
            for (int u = 0; u < nv; ++u) {
              const T hv = (T)v[u];
              bad16 |= f16_over2<T>((unsigned)__builtin_bit_cast(unsigned short, hv));
              reinterpret_cast<T*>(a.out16_hi)[o + u] = hv;
              if (a.out16_lo) reinterpret_cast<T*>(a.out16_lo)[o + u] = (T)(v[u] - (float)hv);
            }
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) { cs[u] += v[u]; cq[u] += v[u] * v[u]; }
      }
    }
    if (a.chan_stats) {   // block-uniform
#pragma unroll
      for (int u = 0; u < 4; ++u) { sPart[(rg * 128 + c4 * 4 + u) * 2] = cs[u]; sPart[(rg * 128 + c4 * 4 + u) * 2 + 1] = cq[u]; }
      __syncthreads();
      const int row0 = sub * rows_per;
      if (tid < 128 && n0 + tid < a.cout && sM[row0] >= 0) {
        float su = 0.f, sq = 0.f;
        for (int g = 0; g < NT / 32; ++g) { su += sPart[(g * 128 + tid) * 2]; sq += sPart[(g * 128 + tid) * 2 + 1]; }   // fixed order
        const int b = sMb[row0];
        // slot: 256-pixel run of the sample; sub-pixel upsample: (low-res run, output parity)
        const int mlow = (p.whole && !GEO1) ? b * p.HWout : m0 + row0;    // first pixel of these rows on the tile grid
        const int run = (mlow - b * p.HWout) / BMT;
        const int nrun = (p.HWout + 255) / 256;
        const int nslab = (SUBPIX && !s2d) ? 4 * nrun : nrun;
        const int slab = (SUBPIX && !s2d) ? run * 4 + parity : run;
        float* d = a.chan_stats + (((long)b * nslab + slab) * a.cout + n0 + tid) * 2;
        d[0] = su; d[1] = sq;
        if (gn_t) { sCh[tid * 2] = su; sCh[tid * 2 + 1] = sq; }
        if (coop) {
          // Publish this tile's sums to the sample's other tiles: 8-byte words {epoch, fp32 bits}, each ONE aligned write-through store
          // (relaxed agent-scope atomic = global_store_dwordx2 sc1) - the data is its own flag, no fence on either side
          // (cdna_hip_programming.md Guideline 16, form R2). The epoch is a device word the host advances before every forward: words of
          // an earlier forward (or the zeros of a fresh buffer) never match it.
          typedef __attribute__((address_space(1))) unsigned long long gu64;
          const unsigned ep = *a.gn_coop_epoch;
          gu64* G = (gu64*)(reinterpret_cast<unsigned long long*>(a.gn_coop) + (((long)b * 4 + run) * 128 + tid) * 2);
          __hip_atomic_store(G, ((unsigned long long)ep << 32) | __float_as_uint(su), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(G + 1, ((unsigned long long)ep << 32) | __float_as_uint(sq), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          sAll[(run * 128 + tid) * 2] = su; sAll[(run * 128 + tid) * 2 + 1] = sq;
        }
      }
      if (coop && wave == 0 && sM[sub * rows_per] >= 0) {
        // ONE wave collects the partner tiles' words: lane l owns channels l and l + 64 of every partner, re-reads all of them each pass until
        // every tag is this forward's epoch, sleeps in between. The partners are this block's neighbours in launch order (block = M-tile,
        // a sample = `coop` consecutive blocks), resident together or started as soon as an earlier block exits; the spin is bounded all the
        // same: on giving up the block flags *gn_coop_tmo (checked by the host like the fp16 guard) and normalises with what it has.
        typedef __attribute__((address_space(1))) unsigned long long gu64;
        const unsigned ep = *a.gn_coop_epoch;
        const int row0c = sub * rows_per;
        const int bb = sMb[row0c];
        const int runc = ((m0 + row0c) - bb * p.HWout) / BMT;
        const gu64* Gb = (const gu64*)(reinterpret_cast<const unsigned long long*>(a.gn_coop) + (long)bb * 4 * 128 * 2);
        bool done = false;
        for (unsigned spins = 0; !done; ++spins) {
          bool ok = true;
          unsigned v[3][4];
#pragma unroll
          for (int pi = 0; pi < 3; ++pi) {
            const int k = (runc + 1 + pi) % coop;
            if (pi < coop - 1) {
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const unsigned long long x = __hip_atomic_load(Gb + (k * 128 + lane + 64 * (j >> 1)) * 2 + (j & 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                v[pi][j] = (unsigned)x;
                ok &= (unsigned)(x >> 32) == ep;
              }
            }
          }
          done = __all(ok);
          if (!done && spins >= (1u << 18)) {       // ~0.25 s of 1-us sleeps: not a scheduling delay any more
            if (lane == 0) atomicOr(a.gn_coop_tmo, 1u);
            done = true;
          }
          if (done) {
#pragma unroll
            for (int pi = 0; pi < 3; ++pi) {
              const int k = (runc + 1 + pi) % coop;
              if (pi < coop - 1) {
#pragma unroll
                for (int j = 0; j < 4; ++j) sAll[(k * 128 + lane + 64 * (j >> 1)) * 2 + (j & 1)] = __uint_as_float(v[pi][j]);
              }
            }
          } else __builtin_amdgcn_s_sleep(32);
        }
      }
      __syncthreads();
      if (gn_t) {
        // The consumer's GroupNorm (+ SiLU) of this sample's 128 channels (a.gn_*): the channel totals just written are complete (the tile
        // holds every pixel of the sample), a group is cpg of them, folded in double like stedm_gn_apply16c; the final values are still
        // in the staged tile.
        const int cpg = a.cout / a.gn_groups, ng = 128 / cpg;
        if (tid < ng) {
          double s_ = 0.0, q_ = 0.0;
          if (coop) {
            // the sample's `coop` x cpg partial sums of this group in the order gn_fold_block (gn_fold.hpp) states for the apply kernels, which
            // fold the same statistics with L = 256 / groups lanes per group: same mean / rstd bits
            const int L = 256 / a.gn_groups, n_e = cpg * coop;
            for (int l = 0; l < L; ++l) {
              double su = 0.0, sq = 0.0;
              for (int e = l; e < n_e; e += L) {
                const int k = e / cpg, c = tid * cpg + (e - k * cpg);
                su += (double)sAll[(k * 128 + c) * 2]; sq += (double)sAll[(k * 128 + c) * 2 + 1];
              }
              s_ += su; q_ += sq;
            }
          } else
          for (int c = tid * cpg; c < (tid + 1) * cpg; ++c) { s_ += (double)sCh[c * 2]; q_ += (double)sCh[c * 2 + 1]; }
          gn_mean_rstd(s_, q_, 1.0 / ((double)cpg * (coop ? p.HWout : rows_per)), a.gn_eps, sGm[tid * 2], sGm[tid * 2 + 1]);
          if (a.gn_mr && sM[row0] >= 0) { float* d = a.gn_mr + ((long)sMb[row0] * a.gn_groups + n0 / cpg + tid) * 2; d[0] = sGm[tid * 2]; d[1] = sGm[tid * 2 + 1]; }
        }
        __syncthreads();
        if (active) {
          const int g = (c4 * 4) / cpg;
          const float mean = sGm[g * 2], rstd = sGm[g * 2 + 1];
          const float4 gm = *reinterpret_cast<const float4*>(a.gn_gamma + n), bt = *reinterpret_cast<const float4*>(a.gn_beta + n);
          const float4 sc = make_float4(rstd * gm.x, rstd * gm.y, rstd * gm.z, rstd * gm.w);
          typedef T V4T __attribute__((ext_vector_type(4)));
          T* __restrict__ g16 = reinterpret_cast<T*>(a.gn_out16);
          const bool silu = a.gn_act == 1;
#pragma unroll 2
          for (int row = row0 + rg; row < row0 + rows_per; row += NT / 32) {
            const int m = sM[row];
            if (m < 0) continue;
            float4 w = *reinterpret_cast<const float4*>(sStage + row * SST + c4 * 4);
            w.x = (w.x - mean) * sc.x + bt.x; w.y = (w.y - mean) * sc.y + bt.y; w.z = (w.z - mean) * sc.z + bt.z; w.w = (w.w - mean) * sc.w + bt.w;
            if (silu) { w.x = silu_f(w.x); w.y = silu_f(w.y); w.z = silu_f(w.z); w.w = silu_f(w.w); }
            V4T h4; h4[0] = (T)w.x; h4[1] = (T)w.y; h4[2] = (T)w.z; h4[3] = (T)w.w;
            *reinterpret_cast<V4T*>(g16 + (long)m * a.cout + n) = h4;
            badn |= f16_over_v4<T>(h4);
            if (a.gn_out16_lo) {     // 3-product modes: the lo planes of the same values
              V4T l4; l4[0] = (T)(w.x - (float)h4[0]); l4[1] = (T)(w.y - (float)h4[1]); l4[2] = (T)(w.z - (float)h4[2]); l4[3] = (T)(w.w - (float)h4[3]);
              *reinterpret_cast<V4T*>(reinterpret_cast<T*>(a.gn_out16_lo) + (long)m * a.cout + n) = l4;
            }
          }
        }
        __syncthreads();
      }
    }
  }
  f16_guard_commit(p.ovf, bad16, STEDM_F16G_CONV_OUT16);
  f16_guard_commit(p.ovf, badn, STEDM_F16G_NORM);
  STAMP(6);
  if STEDM_DBG(p.dbg, 1024) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); STAMP(4); }
}
#undef STAMP
#undef STAMPC

// out = ws[0] + ws[1] + bias + emb + res (fixed order), optional per-(sample, slab, channel) statistics.
// grid (B, slabs of 256 pixels, blocks of 64 channel quads): 256 threads = QB quads x (256 / QB) pixel lanes
// GN: the block also writes the consumer's GroupNorm (+ SiLU) of what it just produced as 16-bit planes (a.gn_out16). The host launches that
// form with one 256-pixel slab per sample (HW <= 256) and qbs = 8: the block's 32 channels are whole groups of its sample, so the group
// statistics are complete inside the block (the same per-channel sums chan_stats receives, folded in double like stedm_gn_apply16c);
// a thread then reads back the pixels it stored itself and writes (v - mean) * (rstd * gamma) + beta, SiLU, 8 bytes per quad.
template <int KSMAX, bool GN = false>   // 2: the two-way split of the batch-64 layers (no register array); 16: any split up to 16
static __global__ void __launch_bounds__(256) conv_splitk_reduce_kernel(const stedm_conv_args a, const int HW, const long plane, const int ksplit,
                                                                        const int qbs /* channel quads per block: 64, 32, 16 or 8 */,
                                                                        unsigned* const ovf /* fp16 range guard flag or nullptr */,
                                                                        const int slab_px = 256 /* pixels per block = per statistics slot */) {
  __shared__ float rpart[256 * 8];   // [npl][QB][8]
  __shared__ float gsum[GN ? 8 * 8 : 1], gmr[GN ? 16 : 1];
  const int b = blockIdx.x, slab = blockIdx.y, nslab = gridDim.y;
  const int C = a.cout, Q = C >> 2, t = threadIdx.x;
  const int qb0 = blockIdx.z * qbs, QB = min(qbs, Q - qb0);
  const int npl = 256 / QB, tq = t % QB, tp = t / QB;
  const int px0 = slab * slab_px, px1 = min(HW, px0 + slab_px);
  const int n = (qb0 + tq) * 4;
  float s[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
  unsigned bad16 = 0u, badn = 0u;
  if (tp < npl) {
    float4 add = a.bias ? *reinterpret_cast<const float4*>(a.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.src16b_hi && a.bias_b) {      // a fused skip_connection: its bias too
      const float4 b4 = *reinterpret_cast<const float4*>(a.bias_b + n);
      add.x += b4.x; add.y += b4.y; add.z += b4.z; add.w += b4.w;
    }
    if (a.emb) {
      const float4 e4 = *reinterpret_cast<const float4*>(a.emb + (long)b * a.emb_bstride + n);
      add.x += e4.x; add.y += e4.y; add.z += e4.z; add.w += e4.w;
    }
    // (ws_bmod: the partials were written at batch ws_bmod - the rows of sample b % ws_bmod; `plane` is one partial of THAT batch)
    const long wshift = a.ws_bmod ? (long)(b - b % a.ws_bmod) * HW * C : 0;
    const long rshift = a.res_bmod ? (long)(b - b % a.res_bmod) * HW * C : 0;
#pragma unroll 2
    for (int pix = px0 + tp; pix < px1; pix += npl) {
      const long o = ((long)b * HW + pix) * C + n;
      float4 pz[KSMAX];                           // all partial tiles of this quad are loaded before they are added (fixed order)
#pragma unroll
      for (int z = 0; z < KSMAX; ++z)
        if (KSMAX == 2 || z < ksplit) pz[z] = *reinterpret_cast<const float4*>(a.ws + z * plane + (o - wshift));
      float4 v = pz[0];
#pragma unroll
      for (int z = 1; z < KSMAX; ++z)
        if (KSMAX == 2 || z < ksplit) { v.x += pz[z].x; v.y += pz[z].y; v.z += pz[z].z; v.w += pz[z].w; }
      v.x += add.x; v.y += add.y; v.z += add.z; v.w += add.w;
      if (a.res) {
        float4 r4 = *reinterpret_cast<const float4*>(a.res + (o - rshift));
        if (a.res2) { const float4 s4 = *reinterpret_cast<const float4*>(a.res2 + (o - rshift)); r4.x += s4.x; r4.y += s4.y; r4.z += s4.z; r4.w += s4.w; }     // t = res + res2
        v.x += r4.x; v.y += r4.y; v.z += r4.z; v.w += r4.w;
      }
      if (GN || a.out) *reinterpret_cast<float4*>(a.out + o) = v;      // (16-bit-only form: no fp32 tensor; the GN form always has one: host)
      if (a.out16_hi) {      // 16-bit side output (operand planes of the consumer), single-product modes; out16_stride: into a wider plane
        const long o16 = a.out16_stride ? ((long)b * HW + pix) * a.out16_stride + n : o;
        if (a.mm_dtype == STEDM_F16) {
          f16x4 h4; h4[0] = (_Float16)v.x; h4[1] = (_Float16)v.y; h4[2] = (_Float16)v.z; h4[3] = (_Float16)v.w;
          *reinterpret_cast<f16x4*>(reinterpret_cast<_Float16*>(a.out16_hi) + o16) = h4;
          bad16 |= f16_over_v4<_Float16>(h4);
        } else {
          bf16x4 h4; h4[0] = (__bf16)v.x; h4[1] = (__bf16)v.y; h4[2] = (__bf16)v.z; h4[3] = (__bf16)v.w;
          *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(a.out16_hi) + o16) = h4;
        }
      }
      s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
      q[0] += v.x * v.x; q[1] += v.y * v.y; q[2] += v.z * v.z; q[3] += v.w * v.w;
    }
    float* d = rpart + (tp * QB + tq) * 8;
#pragma unroll
    for (int j = 0; j < 4; ++j) { d[j] = s[j]; d[4 + j] = q[j]; }
  }
  f16_guard_commit(ovf, bad16, STEDM_F16G_CONV_OUT16);
  if (!a.chan_stats) return;   // block-uniform
  __syncthreads();
  if (t < QB) {
    float su[4] = {0.f, 0.f, 0.f, 0.f}, sq[4] = {0.f, 0.f, 0.f, 0.f};
    for (int l = 0; l < npl; ++l) {   // fixed order
      const float* d = rpart + (l * QB + t) * 8;
#pragma unroll
      for (int j = 0; j < 4; ++j) { su[j] += d[j]; sq[j] += d[4 + j]; }
    }
    float* dst = a.chan_stats + (((long)b * nslab + slab) * C + (qb0 + t) * 4) * 2;
#pragma unroll
    for (int j = 0; j < 4; ++j) { dst[j * 2] = su[j]; dst[j * 2 + 1] = sq[j]; }
    if (GN) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { gsum[t * 8 + j] = su[j]; gsum[t * 8 + 4 + j] = sq[j]; }
    }
  }
  if (GN) {
    const int cpg = C / a.gn_groups, ng = (QB * 4) / cpg;       // whole groups of this block (host-checked: cpg % 4 == 0, 32 % cpg == 0)
    __syncthreads();
    if (t < ng) {
      double s_ = 0.0, q_ = 0.0;
      for (int c = t * cpg; c < (t + 1) * cpg; ++c) { s_ += (double)gsum[(c >> 2) * 8 + (c & 3)]; q_ += (double)gsum[(c >> 2) * 8 + 4 + (c & 3)]; }
      gn_mean_rstd(s_, q_, 1.0 / ((double)cpg * HW), a.gn_eps, gmr[t * 2], gmr[t * 2 + 1]);
      if (a.gn_mr) { float* d = a.gn_mr + ((long)b * a.gn_groups + (qb0 * 4) / cpg + t) * 2; d[0] = gmr[t * 2]; d[1] = gmr[t * 2 + 1]; }
    }
    __syncthreads();
    if (tp < npl) {
      const int g = (tq * 4) / cpg;
      const float mean = gmr[g * 2], rstd = gmr[g * 2 + 1];
      const float4 gm = *reinterpret_cast<const float4*>(a.gn_gamma + n), bt = *reinterpret_cast<const float4*>(a.gn_beta + n);
      const float4 sc = make_float4(rstd * gm.x, rstd * gm.y, rstd * gm.z, rstd * gm.w);
      for (int pix = px0 + tp; pix < px1; pix += npl) {
        const long o = ((long)b * HW + pix) * C + n;
        float4 w = *reinterpret_cast<const float4*>(a.out + o);         // this thread's own store of the loop above
        w.x = (w.x - mean) * sc.x + bt.x; w.y = (w.y - mean) * sc.y + bt.y; w.z = (w.z - mean) * sc.z + bt.z; w.w = (w.w - mean) * sc.w + bt.w;
        if (a.gn_act == 1) { w.x = silu_f(w.x); w.y = silu_f(w.y); w.z = silu_f(w.z); w.w = silu_f(w.w); }
        if (a.mm_dtype == STEDM_F16) {
          f16x4 h4; h4[0] = (_Float16)w.x; h4[1] = (_Float16)w.y; h4[2] = (_Float16)w.z; h4[3] = (_Float16)w.w;
          *reinterpret_cast<f16x4*>(reinterpret_cast<_Float16*>(a.gn_out16) + o) = h4;
          badn |= f16_over_v4<_Float16>(h4);
          if (a.gn_out16_lo) {
            f16x4 l4; l4[0] = (_Float16)(w.x - (float)h4[0]); l4[1] = (_Float16)(w.y - (float)h4[1]); l4[2] = (_Float16)(w.z - (float)h4[2]); l4[3] = (_Float16)(w.w - (float)h4[3]);
            *reinterpret_cast<f16x4*>(reinterpret_cast<_Float16*>(a.gn_out16_lo) + o) = l4;
          }
        } else {
          bf16x4 h4; h4[0] = (__bf16)w.x; h4[1] = (__bf16)w.y; h4[2] = (__bf16)w.z; h4[3] = (__bf16)w.w;
          *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(a.gn_out16) + o) = h4;
          if (a.gn_out16_lo) {
            bf16x4 l4; l4[0] = (__bf16)(w.x - (float)h4[0]); l4[1] = (__bf16)(w.y - (float)h4[1]); l4[2] = (__bf16)(w.z - (float)h4[2]); l4[3] = (__bf16)(w.w - (float)h4[3]);
            *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(a.gn_out16_lo) + o) = l4;
          }
        }
      }
      f16_guard_commit(ovf, badn, STEDM_F16G_NORM);
    }
  }
}

// Launches the reduce pass over `ksplit` partial planes of `plane` floats each (a.ws) for the output of p.a (HWo pixels per sample): the
// second half of a split-K call (conv_rs_try) or a call of its own (conv_splitk_finish, where the planes may hold fewer samples than the
// output: a.ws_bmod, and ksplit may be 1). stats: this pass may write a.chan_stats in the caller's slot layout (fine_ok: ... a partition of
// its own into equal runs of 8 .. 256 pixels). gn_ok: the consumer's GroupNorm may ride in it. Returns whether the statistics were written;
// sets p.gn_done.
static bool splitk_reduce_launch(ConvParams& p, const int HWo, const long plane, const int ksplit, bool stats, const bool fine_ok, const bool gn_ok, hipStream_t st) {
  int qbs = 64;     // small tensors: fewer channel quads per block, so that the partial tiles are read by many CUs
  while (qbs > 8 && (long)p.a.B * ((HWo + 255) / 256) * ((p.a.cout / 4 + qbs - 1) / qbs) < 256) qbs >>= 1;
  // the consumer's GroupNorm in the same pass: a block of 8 channel quads x all pixels of a sample owns whole groups
  const int cpg = (p.a.gn_out16 && p.a.gn_groups > 0) ? p.a.cout / p.a.gn_groups : 0;
  const bool gn = cpg > 0 && p.a.out && HWo <= 256 && gn_ok && p.a.chan_stats && stats && (p.a.chan_nslab == 0 || p.a.chan_nslab == 1) && p.a.cout % 32 == 0 &&
                  cpg % 4 == 0 && 32 % cpg == 0;
  if (gn) qbs = 8;
  // pixels per block (= per statistics slot). With statistics: the caller's partition (fine_ok above; the default is 256-pixel runs).
  // Without: free - short runs when the 256-pixel grid would leave most of the chip idle (batch <= 8: a reduce of 32 - 64 blocks walking
  // 8 pixel iterations x up to 16 partials each took 10 - 13 us, 27 % of a batch-1 denoising step)
  int slab_px = 256;
  if (!gn) {
    if (p.a.chan_stats && stats && fine_ok) slab_px = HWo / p.a.chan_nslab;
    else if (!p.a.chan_stats || !stats)
      while (slab_px > 16 && HWo % (slab_px / 2) == 0 && (long)p.a.B * ((HWo + slab_px - 1) / slab_px) * ((p.a.cout / 4 + 7) / 8) < 512) slab_px >>= 1;
    if (slab_px < 256) {   // a block is (pixel lanes) x (channel quads) = 256 threads: as many pixel lanes as the run has pixels, at most 32
      qbs = 256 / (slab_px < 32 ? slab_px : 32);
      if (qbs > 64) qbs = 64;
    }
  }
  dim3 grid(p.a.B, (HWo + slab_px - 1) / slab_px, (p.a.cout / 4 + qbs - 1) / qbs);
  stedm_conv_args ra = p.a;
  if (!stats) ra.chan_stats = nullptr;     // another slot layout than this pass fills: the dispatcher's statistics pass writes the caller's
  if (gn) {
    if (ksplit == 2) conv_splitk_reduce_kernel<2, true><<<grid, 256, 0, st>>>(ra, HWo, plane, 2, qbs, p.ovf);
    else conv_splitk_reduce_kernel<16, true><<<grid, 256, 0, st>>>(ra, HWo, plane, ksplit, qbs, p.ovf);
    p.gn_done = 1;
  } else if (ksplit == 2) conv_splitk_reduce_kernel<2><<<grid, 256, 0, st>>>(ra, HWo, plane, 2, qbs, p.ovf, slab_px);
  else conv_splitk_reduce_kernel<16><<<grid, 256, 0, st>>>(ra, HWo, plane, ksplit, qbs, p.ovf, slab_px);
  return ra.chan_stats != nullptr;      // only what the reduce pass really wrote in the caller's layout counts as done
}

// stedm_conv_finish (conv_common.hpp): the pass above on its own. The caller (conv_igemm.hip) has checked the arguments.
static int splitk_finish_impl(ConvParams& p, const int nshare, hipStream_t st) {
  const stedm_conv_args& a = p.a;
  const int HW = a.Hin * a.Win, nrun = (HW + 255) / 256;
  const bool fine_ok = a.chan_nslab > 0 && HW % a.chan_nslab == 0 && HW / a.chan_nslab >= 8 && HW / a.chan_nslab <= 256;
  const bool stats = a.chan_stats && (a.chan_nslab == 0 || a.chan_nslab == nrun || fine_ok);
  const long plane = (long)(a.ws_bmod ? a.ws_bmod : a.B) * HW * a.cout;
  p.gn_done = 0;
  const bool wrote = splitk_reduce_launch(p, HW, plane, nshare, stats, fine_ok, true, st);
  STEDM_LAUNCH_CHECK();
  p.stats_done = wrote ? 1 : 0;
  return 0;
}

template <typename T, int WM, int KIND, bool FUSE = false, bool P3 = false>
static int conv_rs_try(ConvParams& p, const ConvParams& q, hipStream_t st, bool dry = false) {
  constexpr size_t LDS_MAX = 160 * 1024;
  constexpr int BMT = 256;
  constexpr bool G1 = KIND == RS_1X1M;                       // the 3-product 1x1 (16x16x32 MFMA, 64-B rows)
  constexpr bool SUBK = KIND == RS_SUB || KIND == RS_SUBM;   // sub-pixel upsample / space-to-depth geometry
  constexpr bool M16 = KIND == RS_3X3M || G1 || KIND == RS_SUBM;
  constexpr bool K1 = KIND == RS_1X1 || KIND == RS_1X1N;
  constexpr int PPI = K1 ? 8 : (G1 ? 16 : 32), NPL = (SUBK || KIND == RS_3X3M) ? 2 : 1, NTAB = (KIND == RS_3X3 || KIND == RS_3X3M) ? 9 : 4;
  if ((KIND == RS_3X3M || G1) && q.a.mode != STEDM_CONV_S1) return -1;   // a tap is the uniform offset (dy * PW + dx) * 32: stride-1 geometry
  const size_t nai = (q.NP + PPI - 1) / PPI;
  if ((nai + 1) / 2 > (K1 ? 16 : 13)) return -1;
  bool stats = q.a.chan_stats != nullptr;
  if (stats && (K1 || G1) && !(BMT % q.HWout == 0 || q.HWout % BMT == 0)) stats = false;   // tile rows do not split by sample: dispatcher pass
  const bool s2d = SUBK && q.a.mode == STEDM_CONV_S2D;
  const int nrun = (q.HWout + 255) / 256;
  // the epilogue fills 256-pixel runs (sub-pixel upsample: run x output parity); another slot count is left to the extra pass
  // (a split-K launch leaves the statistics to its reduce pass, which fills whatever partition of a sample's pixels into equal runs of 8..256 the
  // caller laid out: small batches ask for short runs so that the reduce has blocks for the whole chip - reduce_slab_px below)
  const int HWo = (SUBK && !s2d) ? 4 * q.HWout : q.HWout;     // pixels of a sample in the OUTPUT (what a split-K reduce pass walks)
  const bool fine_ok = q.ksplit >= 2 && q.a.chan_nslab > 0 && HWo % q.a.chan_nslab == 0 && HWo / q.a.chan_nslab >= 8 && HWo / q.a.chan_nslab <= 256;
  if (stats && q.a.chan_nslab != 0 && q.a.chan_nslab != ((SUBK && !s2d) ? 4 * nrun : nrun) && !fine_ok) stats = false;
  if (stats && SUBK && !s2d && q.a.chan_nslab == 0) stats = false;
  // a split-K reduce pass without the caller's fine partition walks 256-pixel runs of the OUTPUT: its slot count must be the caller's
  // (sub-pixel upsample from 40 x 40: 4 * nrun = 28 slots at the caller, 25 runs of the 80 x 80 output)
  if (stats && q.ksplit >= 2 && !fine_ok && q.a.chan_nslab != 0 && (HWo + 255) / 256 != q.a.chan_nslab) stats = false;
  size_t a_buf = NPL * nai * 1024 + (M16 ? 32 : 0);
  if (FUSE && a_buf < 32768) a_buf = 32768;
  if (P3) a_buf *= 2;                                  // hi and lo image of a chunk
  const size_t ring = (P3 ? 3 : 4) * a_buf;
  const size_t loop = ring + (size_t)(M16 ? 1 : NTAB) * BMT * sizeof(int);    // (the 16x16x32 kind builds the tap-0 gather row only)
  const size_t staging = (size_t)BMT * kStageStride * sizeof(float) + (stats ? (size_t)((16 / WM + 2) * 2) * 128 * 2 * sizeof(float) + (128 + 32) * 2 * sizeof(float) : 0);
  const size_t lds = (size_t)2 * BMT * sizeof(int) + (loop > staging ? loop : staging);
  if (lds > LDS_MAX) return -1;
  auto magic = [](int d) { return (unsigned)((0x100000000ull + (unsigned)d - 1) / (unsigned)d); };
  const bool flat = (K1 || G1) && q.a.B == 1;    // a GEMM viewed as one long "image": every row belongs to sample 0
  // keeps every numerator * divisor of the magic divisions below 2^32: div_hw sees tile-local or sample-local rows (1x1 / whole-sample
  // tiles), div_w sees a row index of the tile or, for the sub-pixel scatter, a pixel index of the sample
  // (the 1x1 kind never divides by Wout: a long flat GEMM, Wout = M, stays admissible)
  if (((K1 || G1) && q.HWout >= 65536 && !flat) || q.PRs * q.PW >= 65536 || (!(K1 || G1) && (long)q.HWout * q.Wout >= (1l << 32))) return -1;
  // N-persistent form (see the kernel): a flat GEMM whose K fits the ring, enough M-tiles for the chip, one of the three plain epilogues
  if (KIND == RS_1X1N &&
      !(WM == 4 && !FUSE && flat && q.ksplit < 2 && q.Cin <= 256 && q.tiles_n >= 2 && q.a.cout % 8 == 0 && (long)q.tiles_m * 4 >= (long)stedm_device_cus() * 3 &&
        !q.a.chan_stats && !q.a.emb && !q.a.gn_out16 && !q.a.out16_lo && !q.a.ln_gamma &&
        // 32-bit offsets (ragged N: + the 2^31 sentinel). Bounded on the PADDED row count: the last M-tile addresses up to 255 rows beyond M and
        // relies on the descriptor's range check, which only works while those offsets do not wrap
        (q.a.qkv_q || (long)q.tiles_m * 256 * q.a.cout * (q.a.out ? 4 : 2) < (q.a.cout % 128 ? (1l << 31) : (1l << 32))) &&
        (!q.a.qkv_q || ((long)q.tiles_m * 256 / q.a.qkv_T + 2) * q.a.qkv_heads * 64 * q.a.qkv_Tp * 2 < (1l << 32)) &&
        ((q.a.qkv_q && q.tiles_n >= 3) || (q.a.out && !q.a.out16_hi && !q.a.act_out) || (!q.a.out && q.a.out16_hi && !q.a.res && !q.a.qkv_q)) &&
        !getenv("STEDM_CONV_NO_NPERS")))
    return -1;
  if (q.a.ln_gamma && (KIND != RS_1X1 || q.tiles_n != 1 || q.ksplit >= 2)) return -1;     // the LayerNorm epilogue: the tiled 1x1 kind, one N-tile, no K split
  // the 16-bit-only form with statistics (out == NULL, out16_hi [+ out16_stride], chan_stats): this launch's own epilogue / reduce pass must
  // write them - there is no fp32 tensor for the dispatcher's extra pass; a strided out16 plane belongs to the generic row loop / reduce pass
  if (!q.a.out && q.a.chan_stats && !stats) return -1;
  if (q.a.out16_stride && (KIND == RS_1X1N || P3)) return -1;
  // a K window / res_bmod / res2 / the partials-only form: the plain 3x3 kinds alone (conv_setup has checked the arguments; this keeps every other instantiation out)
  const bool kwin = q.a.src16_cstride || q.a.k_chan0 || q.a.w_cin;
  if ((kwin || q.a.res_bmod || q.a.res2 || q.partials) && !((KIND == RS_3X3 || KIND == RS_3X3M) && !FUSE && !P3)) return -1;
  if (q.a.res2 && q.a.cout % 4 != 0) return -1;     // (both row loops read it as float4)
  if (dry) { p.nshare = q.ksplit >= 2 ? q.ksplit : 1; return 0; }
  p = q;
  p.mg_hw = flat ? 0u : magic(p.HWout); p.mg_w = magic(p.Wout); p.mg_pw = magic(p.PW); p.mg_prpw = magic(p.PRs * p.PW);
  {
    // block -> tile order by fabric bytes: plain order fetches the patch min(8, tiles_n) times and each weight slice once; a gm x (8 / gm)
    // XCD grid fetches the patch 8 / gm times and the weights gm times
    const double abytes = (double)p.M * (p.Cin + (FUSE ? p.a.cb : 0)) * 2.0 * (P3 ? 2 : 1);
    const double wbytes = (double)p.a.cout * (p.Cin * p.taps + (FUSE ? p.a.cb : 0)) * 2.0 * (P3 ? 2 : 1);
    double best = abytes * (p.tiles_n < 8 ? p.tiles_n : 8) + wbytes;
    p.xcd_m = 0;
    if (p.tiles_n > 1)
      for (int gm = 8; gm >= 2; gm >>= 1) {
        const int gn = 8 / gm;
        if (p.tiles_m % gm != 0 || p.tiles_n % gn != 0) continue;
        const double cost = abytes * gn + wbytes * gm;
        if (cost < best * 0.97) { best = cost; p.xcd_m = gm; }
      }
  }
  // the consumer's GroupNorm in the epilogue: a tile of whole samples (HWout divides 256) and 128 channels of whole groups, fast store path
  {
    const stedm_conv_args& a_ = p.a;
    const int cpg = (a_.gn_out16 && a_.gn_groups > 0) ? a_.cout / a_.gn_groups : 0;
    // (round 5: also behind a fused skip_connection phase - the epilogue is the same - for the NEXT block's in_layers GroupNorm riding on a tail convolution)
    p.gn_tile = (cpg > 0 && stats && q.ksplit < 2 && (KIND == RS_3X3 || KIND == RS_3X3M) && (!P3 || a_.gn_out16_lo) && p.HWout <= BMT && BMT % p.HWout == 0 &&
                 a_.cout % 128 == 0 && cpg % 4 == 0 && 128 % cpg == 0 && a_.out && !a_.out16_hi && !a_.act_out) ? 1 : 0;
  }
  // ... or, where a sample spans 2 .. 4 tiles (the 32 x 32 level at 128 channels), with the tiles of a sample exchanging their channel sums inside
  // the launch (a.gn_coop; the kernel's comment has the protocol). One N-tile only: block id = M-tile, so the tiles of a sample are
  // consecutive blocks of one dispatch round
  p.gn_coop = 0;
  {
    const stedm_conv_args& a_ = p.a;
    const int cpg = (a_.gn_out16 && a_.gn_groups > 0) ? a_.cout / a_.gn_groups : 0;
    const int nt = p.HWout / BMT;
    static const bool off = getenv("STEDM_NO_GN_COOP") != nullptr;      // A/B timing and the tests' reference run
    if (!p.gn_tile && !off && cpg > 0 && stats && q.ksplit < 2 && (KIND == RS_3X3 || KIND == RS_3X3M) && !FUSE && !P3 && p.HWout % BMT == 0 && nt >= 2 && nt <= 4 &&
        a_.cout == 128 && p.tiles_n == 1 && p.xcd_m == 0 && !p.whole && cpg % 4 == 0 && 128 % cpg == 0 && 256 % a_.gn_groups == 0 && a_.out && !a_.out16_hi && !a_.act_out &&
        a_.gn_coop && a_.gn_coop_epoch && a_.gn_coop_tmo && (size_t)lds + 4 * 128 * 2 * sizeof(float) <= LDS_MAX)
      p.gn_coop = nt;
  }
  p.npers = 0;
  if (KIND == RS_1X1N) {
    // one block per M-tile, or two (each half of the N-tiles) when that shortens the schedule: rounds x (fixed cost + N-tiles per block), the
    // fixed cost (tables, the A panel) priced at two N-tiles; the second block starts at tiles_n / 2, before the v tiles (from 2 tiles_n / 3) of a qkv epilogue
    const long cus = stedm_device_cus() > 0 ? stedm_device_cus() : 256;
    auto cost = [&](int s_) { return ((long)p.tiles_m * s_ + cus - 1) / cus * (2 + p.tiles_n / s_); };
    p.npers = (p.tiles_n % 2 == 0 && p.tiles_n >= 4 && cost(2) < cost(1)) ? 2 : 1;
  }
  ConvParams kp = p;
  if (!stats) kp.a.chan_stats = nullptr;
  if (q.a.k_chan0) {
    // the window's first chunk: a channel is 2 bytes of a pixel row and 9 taps x 256 bytes of an N-tile's fragment stream in both
    // fragment orders (16 channels x 9 x 4 KiB, 32 channels x 9 x 8 KiB)
    kp.a.src16_hi = reinterpret_cast<const unsigned char*>(q.a.src16_hi) + (size_t)q.a.k_chan0 * 2;
    if (q.a.w_frag) kp.a.w_frag = reinterpret_cast<const unsigned char*>(q.a.w_frag) + (size_t)q.a.k_chan0 * 9 * 256;
    if (q.a.w_frag16) kp.a.w_frag16 = reinterpret_cast<const unsigned char*>(q.a.w_frag16) + (size_t)q.a.k_chan0 * 9 * 256;
  }
  auto k = conv_rs_kernel<T, WM, KIND, FUSE, P3>;
  const size_t lds_launch = lds + (p.gn_coop ? (size_t)4 * 128 * 2 * sizeof(float) : 0);     // + the partner tiles' channel sums
  static size_t lds_set = 0;     // per instantiation: the attribute only ever grows (one driver call per new maximum)
  if (lds_launch > lds_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_launch);
    if (e != hipSuccess) { set_error("conv_igemm(rs): hipFuncSetAttribute(%zu) failed: %s", lds_launch, hipGetErrorString(e)); return 2; }
    lds_set = lds_launch;
  }
  if (kp.ksplit >= 2) kp.a.chan_stats = nullptr;   // the reduce kernel below writes them
  k<<<p.npers ? p.tiles_m * p.npers : p.tiles_m * p.tiles_n * ((SUBK && !s2d) ? 4 : 1) * (kp.ksplit >= 2 ? kp.ksplit : 1), (16 / WM + 2) * 64, lds_launch, st>>>(kp);
  STEDM_LAUNCH_CHECK();
  p.nshare = kp.ksplit >= 2 ? kp.ksplit : 1;
  if (kp.ksplit >= 2 && !p.partials) {
    stats = splitk_reduce_launch(p, HWo, (long)p.a.B * HWo * p.a.cout, kp.ksplit, stats, fine_ok, !(SUBK && !s2d), st);
    STEDM_LAUNCH_CHECK();
  }
  if (p.partials) return 0;     // (stedm_conv_partials: the partial planes are the result)
  if (stats) p.stats_done = 1;
  if (p.gn_tile || p.gn_coop) p.gn_done = 1;
  return 0;
}

// single-product 3x3 (stride 1 / nearest-up) and 1x1 convolutions with fragment-order weights, 256 x 128 tiles; -1 when it does not apply
// `dry`: only report whether the kernel would run (0) or not (-1); used for the fused-skip capability query
template <typename T>
static int conv_rs_pick(ConvParams& p, hipStream_t st, bool dry = false) {
  const stedm_conv_args& a = p.a;
  const bool fuse = a.src16b_hi != nullptr;
  if (fuse && (a.ks != 3 || a.mode != STEDM_CONV_S1 || !a.w_frag_b || a.cb <= 0 || a.cb % 64 != 0 || a.res)) return -1;
  if ((!a.w_frag && !a.w_frag16) || (a.act_out != 0 && a.act_out != 2) || a.npass != 1 || a.mode == STEDM_CONV_DOWN) return -1;
  const bool s2d = a.mode == STEDM_CONV_S2D;
  const bool sp = (a.mode == STEDM_CONV_UP_SUBPIXEL || s2d) && p.taps == 4 && p.Cin % 32 == 0;
  if (s2d && !sp) return -1;
  const bool k3 = a.ks == 3 && p.taps == 9 && p.Cin % 16 == 0, k1 = a.ks == 1 && p.Cin % 64 == 0;
  if (!k3 && !k1 && !sp) return -1;
  if (a.qkv_q && (!k1 || fuse || !a.w_frag)) return -1;     // the qkv epilogue lives in the 1x1 kind (no K split: it has no fp32 output)
  if (a.ln_gamma && (!k1 || fuse || !a.w_frag || a.cout > 128)) return -1;   // ... and so does the LayerNorm epilogue (whole rows in one tile)
  static int cus = 0;
  if (cus == 0) { cus = stedm_device_cus(); if (cus <= 0) cus = 256; }
  ConvParams q = p;
  if (!conv_geometry(q, 256, /*allow_wsplit=*/true)) return -1;
  q.ksplit = 0;
  // K split: the smallest power of two (<= 16) that brings the grid to 3/4 of the chip (or the largest admissible one), if the chunk
  // count divides and every share keeps at least 4 chunks; needs the caller's workspace (ksplit partial tiles) and the plain fp32 epilogue.
  // Very small grids (the batch-1 CFG step: 8 tiles) may go down to 2 or 1 chunks per share: a workgroup's fixed cost (tables, first patch,
  // partial-tile store: ~10 us) is paid either way, its K walk (~3 us per 32-channel chunk at one tile per CU) is what the idle CUs can take
  auto pick_split = [&](long tiles, int nchunks, int planes = 1, int nchunks2 = 0) {   // planes: partial rows per tile row (4: the sub-pixel form's output); nchunks2: the fused skip's chunks
    if (!a.ws || (!a.out && !a.out16_hi) || a.out16_lo || a.act_out || a.cout % 4 != 0 || (a.emb && a.emb_bstride % 4 != 0) || a.ln_gamma || a.qkv_q) return 0;
    const int minc = tiles * 16 <= cus ? 1 : (tiles * 8 <= cus ? 2 : 4);
    int best = 0;   // tiny problems never fill the chip: the largest admissible split still shortens the serial K walk the most
    for (int ks = 2; ks <= 16; ks *= 2) {
      if (nchunks % ks != 0 || nchunks / ks < minc || a.ws_floats < (long)ks * planes * p.M * a.cout || nchunks2 % ks != 0) break;
      best = ks;
      if (tiles * ks * 4 >= (long)cus * 3) break;
    }
    return best;
  };
  // sub-pixel / space-to-depth forms on the 16x16x32 MFMA (RS_SUBM) when the caller packed ONLY that fragment order (hi stream of the _hl
  // packs). Measured on the headline step (round 5, same box): 154.4 steps/s with the two Upsamples on RS_SUBM against 156.3 on the
  // 32x32x16 RS_SUB form - four taps per 32-channel chunk make the chunk barrier and the patch DMA 2.25x as frequent per MFMA as in the
  // 3x3, and that, not the MFMA shape, is what holds this kind at 35 % MFMA-busy. RS_SUB stays the form of choice.
  const bool subm = sp && a.w_frag16 && !a.w_frag;
  if (s2d) {
    // Downsample: small grids by nature (encoder batch, half resolution); there is no other kernel for this form
    q.ksplit = (long)q.tiles_m * q.tiles_n * 4 < (long)cus * 3 ? pick_split((long)q.tiles_m * q.tiles_n, p.Cin / 32) : 0;
    if (subm) { const int rc = conv_rs_try<T, 4, RS_SUBM>(p, q, st, dry); if (rc >= 0 || !a.w_frag) return rc; }
    return a.w_frag ? conv_rs_try<T, 4, RS_SUB>(p, q, st, dry) : -1;
  }
  // 16x16x32 MFMA kind: plain 3x3 with its fragment-order weights at hand
  // (short K: the per-tile fixed costs dominate and the 32x32x16 form is 3 % faster at Cin 128, equal at 256: measured, tools/ab_m16.py)
  // (round 4, with the spread loop: the 16x16x32 form from 128 channels on measured 160.3 vs 159.7 steps/s - inside the noise; the threshold stays)
  const bool m16 = k3 && a.mode == STEDM_CONV_S1 && a.w_frag16 && p.Cin % 32 == 0 && p.Cin >= 256 && (!fuse || a.w_frag_b16);
  if (!a.w_frag && !m16 && !subm) return -1;          // only the 16x16x32 order was packed and this problem cannot use it
  if (fuse && !m16 && !a.w_frag_b) return -1;
  if ((long)q.tiles_m * q.tiles_n * (sp ? 4 : 1) * 4 < (long)cus * 3) {
    // too few 256-row tiles to fill the chip: split K over several blocks per tile when that does (deterministic, see the kernel)
    const int ks = k3 ? pick_split((long)q.tiles_m * q.tiles_n, p.Cin / (m16 ? 32 : 16), 1, fuse ? a.cb / 64 : 0)
                 : (k1 && !fuse)      ? pick_split((long)q.tiles_m * q.tiles_n, p.Cin / 64)
                 : sp                 ? pick_split((long)q.tiles_m * q.tiles_n * 4, p.Cin / 32, 4) : 0;     // (sub-pixel upsample; s2d returned above)
    // a 1x1 on half the chip still beats the LDS kernels (its bound is the L1 / L2 traffic per CU, not the CU count)
    const bool half_ok = k1 && (long)q.tiles_m * q.tiles_n * 2 >= cus;
    if (ks == 0 && !half_ok) return -1;   // the 128-row kernels fill the chip better
    q.ksplit = ks;
  }
  if (fuse) {
    if (!k3) return -1;
    int rc = m16 ? conv_rs_try<T, 4, RS_3X3M, true>(p, q, st, dry) : -1;
    if (rc >= 0 || !a.w_frag || !a.w_frag_b) return rc;
    if (m16) q.ksplit = 0;        // (the split was sized for 32-channel chunks)
    return conv_rs_try<T, 4, RS_3X3, true>(p, q, st, dry);
  }
  if (sp) {
    if (subm) { const int rc = conv_rs_try<T, 4, RS_SUBM>(p, q, st, dry); if (rc >= 0 || !a.w_frag) return rc; }
    return a.w_frag ? conv_rs_try<T, 4, RS_SUB>(p, q, st, dry) : -1;
  }
  if (k1) {
    const int rc = conv_rs_try<T, 4, RS_1X1N>(p, q, st, dry);     // short-K flat GEMMs that fill the chip with M-tiles alone
    return rc >= 0 ? rc : conv_rs_try<T, 4, RS_1X1>(p, q, st, dry);
  }
  if (m16) { const int rc = conv_rs_try<T, 4, RS_3X3M>(p, q, st, dry); if (rc >= 0 || !a.w_frag) return rc; q.ksplit = 0; }
  return conv_rs_try<T, 4, RS_3X3>(p, q, st, dry);
}

// 3-product mode (npass = 3) on the register-streamed kernel: plain 3x3, stride 1, from 128 input channels (a multiple of 32), hi / lo
// activation planes and the hi + lo fragment streams of stedm_pack_conv_weight_frag16_hl in a.w_frag16. -1 when it does not apply (the
// LDS-operand 3-product kernel then runs the problem from w_hi / w_lo).
template <typename T>
static int conv_rs3_pick(ConvParams& p, hipStream_t st, bool dry = false) {
  const stedm_conv_args& a = p.a;
  const bool k1 = a.ks == 1 && p.taps == 1;          // 1x1 (skip_connection, qkv, proj_out): RS_1X1M, w_frag16 from stedm_pack_conv_weight_frag16_hl1
  const bool s2d = a.mode == STEDM_CONV_S2D;
  const bool sp = (a.mode == STEDM_CONV_UP_SUBPIXEL || s2d) && a.ks == 3 && p.taps == 4;      // RS_SUBM, w_frag16 from the _up_ / _s2d_frag16_hl packers
  if (a.npass != 3 || !a.w_frag16 || !a.src16_lo || a.src16b_hi || !(sp || ((k1 || (a.ks == 3 && p.taps == 9)) && a.mode == STEDM_CONV_S1)) ||
      p.Cin % 32 != 0 || p.Cin < (k1 ? 64 : 128) || (a.act_out != 0 && a.act_out != 2))
    return -1;
  static int cus = 0;
  if (cus == 0) { cus = stedm_device_cus(); if (cus <= 0) cus = 256; }
  ConvParams q = p;
  if (!conv_geometry(q, 256, /*allow_wsplit=*/true)) return -1;
  q.ksplit = 0;
  const long tiles = (long)q.tiles_m * q.tiles_n * ((sp && !s2d) ? 4 : 1);      // (the sub-pixel form launches every tile for its 4 output parities)
  if (tiles * 4 < (long)cus * 3) {   // too few tiles for the chip: K split as in conv_rs_pick (same workspace contract, same reduce kernel)
    const int nchunks = p.Cin / 32;
    int best = 0;
    if (a.ws && a.out && !a.out16_hi && !a.act_out && a.cout % 4 == 0 && !(a.emb && a.emb_bstride % 4 != 0) && !(sp && !s2d))
      for (int ks = 2; ks <= 16; ks *= 2) {
        if (nchunks % ks != 0 || nchunks / ks < 4 || a.ws_floats < (long)ks * p.M * a.cout) break;
        best = ks;
        if (tiles * ks * 4 >= (long)cus * 3) break;
      }
    if (best == 0 && tiles * 2 < cus) return -1;     // under half the chip and no split: the 128-row LDS-operand tiles fill it better
    q.ksplit = best;
  }
  if (k1) return conv_rs_try<T, 4, RS_1X1M, false, true>(p, q, st, dry);
  if (sp) return conv_rs_try<T, 4, RS_SUBM, false, true>(p, q, st, dry);
  return conv_rs_try<T, 4, RS_3X3M, false, true>(p, q, st, dry);
}
