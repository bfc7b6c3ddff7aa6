// head_kernels.hip — the PPO actor / critic MLP heads over the learner's tall
// activation matrices (builders.py:86-175: Linear-ReLU-Linear-ReLU-Linear
// [-Tanh], PPO_ActorNetwork / PPO_CriticNetwork; ppo_net.py:143-152,277-315
// feed them the LSTM outputs), the forward and the input-gradient chain each
// as ONE launch instead of three GEMM launches (+ split-K reduces at small
// batches).
//
// A workgroup owns 16 rows (one MFMA row tile) and runs every layer of the
// chain over them; the activations between layers stay in LDS, the weights
// stream from L2 straight into MFMA registers.  Layer Y = X W^T with W [N][K]
// row-major (k contiguous):
//   * output features in 16-column tiles, tile nt on wave nt % 4; in the
//     two-row-tile forms a wave runs exactly the tiles it owns: the k loop
//     exists unrolled for NT, NT - 1 and NT - 2 tiles and one wave-uniform
//     branch per layer picks the body (hc_run), so no matrix-pipe time goes to
//     tiles past the layer's last;
//   * k in chunks of 16: lane (li, lk) reads X[li][16c + 4lk .. +3] from LDS
//     and W[16 nt + li][16c + 4lk .. +3] from global memory (16-byte reads),
//     and MFMA j of the chunk (v_mfma_f32_16x16x4_f32) takes element j of
//     both: the k order inside a chunk is permuted identically on the two
//     operands, so every chunk adds its exact 16-term dot product (an fmaf
//     chain, like every f32 MFMA);
//   * the weight reads of the next two chunks are in flight behind the MFMAs
//     of the current one (register ring, sched_barrier pins the refills), each
//     addressed by the matrix's scalar base and one 32-bit offset register;
//   * the epilogue (bias + ReLU, or the ReLU mask of the backward) writes the
//     tile to LDS for the next layer and the workgroup copies the rows out to
//     HBM as 16-byte stores (HA1 / HA2 for the backward, dH2 / dH1 for the
//     weight gradients).
// The narrow last layer (<= 16 outputs: the 8 action means, the value) splits
// its k chunks over the four waves and sums the four partials in a fixed order.
//
// The backward chain dH2 = (dZ W3) * [HA2 > 0], dH1 = (dH2 W2) * [HA1 > 0],
// dX = dH1 W1[:, cols] reads W2 and W1 TRANSPOSED (k contiguous again): the
// forward of the same phase writes W1^T and W2^T as a side job (the weights do
// not change between a phase's forward and backward), so the backward's
// weight reads are 16-byte reads too.  dZ W3 has K = out <= 16 (8 actions or
// the value): a VALU pass in the order of the streaming small-K kernel; in the
// two-row-tile forms its W3 rows and HA2 masks are loaded with dZ, ahead of the
// first barrier, and only the row groups that exist.
//
// Rows are the learner's [step][segment] rows; the weight gradients of the
// three layers stay in the phase's grouped dW launch (linear_dw.hip).
#include "smi_device.hpp"
#include "smi_internal.hpp"
#include "pol_rows.hpp"
#include <type_traits>

namespace smi {

// (HC_R, rows per workgroup, and the LDS carve, head_plan: smi_shapes.hpp)
constexpr int HC_MAXK = 512;             // widest layer input / output handled here

struct HeadFwdArgs {
  const float* X; int64_t ldx; int K0;   // input rows [rows][ldx], K0 features
  const float* W1; const float* b1;      // [h1][K0]
  const float* W2; const float* b2;      // [h2][h1]
  const float* W3; const float* b3;      // [out][h2]
  int h1, h2, out, tanh_out;
  float* HA1; float* HA2;                // [rows][h1], [rows][h2] (post-ReLU)
  float* Y; int64_t ldy;                 // [rows][ldy]
  float* W1T; float* W2T;                // optional: [K0][h1], [h1][h2] for the backward
  int64_t rows; const int* skip;
  int ld0, ld1, ld2;                     // LDS leading dims (floats)
  // the carve (head_plan): the HA1 tile and the partials / transpose tile in
  // floats from the start of LDS (X and HA2 at 0); shared: o1 == 0, every tile
  // takes its turn in the one region
  int o1, oR, shared;
  // optional value-loss epilogue (out == 1, ppo.py:311-331): vgrad[r] =
  // vscale * (Y[r] - vret[r]), the MSE gradient the learner's value_rows pass
  // would compute from Y (same fp32 ops), written by the forward itself
  const float* vret; float* vgrad; float vscale;
  // with vgrad: the value statistics of the last value epoch (ppo.py:324-331,
  // value_rows_kernel's sums {sum (V-R)^2, sum (R-V), sum (R-V)^2, sum R,
  // sum R^2}), five fp64 per workgroup at vpart[blockIdx.x * 5 ..] (nullable)
  double* vpart;
};

struct HeadBwdArgs {
  const float* dZ; int out;              // [rows][out]: gradient at the last pre-activation
  const float* W3;                       // [out][h2]
  const float* W2T;                      // [h1][h2] (forward's transpose)
  const float* W1T;                      // [in][h1] (forward's transpose)
  int h1, h2, dx0, dxn;                  // dX columns [dx0, dx0 + dxn) of the head input
  const float* HA1; const float* HA2;    // forward activations (ReLU masks)
  float* dH2; float* dH1;                // [rows][h2], [rows][h1]
  float* dX; int64_t lddx;               // [rows][lddx]
  const float* mask; int64_t ldm;        // optional: dX zero where mask <= 0
  int64_t rows; const int* skip;
  int ld2, ld1;                          // LDS leading dims
  // policy-gradient prologue (head_bwd_kernel<..., PG>): dZ of the workgroup's
  // rows computed here from the policy rows (policy_rows_grad_kernel's pass)
  // instead of read; written to pg.dz for the layer-3 weight gradient, the
  // rows' d/dstd sums to pg.lvpart[blockIdx.x]
  PolRowArgs pg;
};

// Developer phase timer (build variant 'prof', -DSMI_PROF): thread 0 of every
// workgroup adds its wall-clock ticks (100 MHz) per phase into g_head_ticks
// (vector atomics), [8] counts the workgroups; forward and backward each own
// 10 slots (smi_head_phase_ticks, tools/head_ticks.py)
#ifdef SMI_PROF
__device__ unsigned long long g_head_ticks[2][10];
#define HEAD_T0() unsigned long long h_t0_ = wall_clock64(), h_prev_ = h_t0_
#define HEAD_TICK(k, id)                                                   \
  do {                                                                      \
    if (threadIdx.x == 0) {                                                 \
      const unsigned long long n_ = wall_clock64();                         \
      atomicAdd(&g_head_ticks[k][id], n_ - h_prev_);                        \
      h_prev_ = n_;                                                         \
    }                                                                       \
  } while (0)
#define HEAD_END(k)                                                        \
  do {                                                                      \
    if (threadIdx.x == 0) {                                                 \
      atomicAdd(&g_head_ticks[k][8], 1ull);                                 \
      atomicAdd(&g_head_ticks[k][9], wall_clock64() - h_t0_);               \
    }                                                                       \
  } while (0)
#else
#define HEAD_T0() (void)0
#define HEAD_TICK(k, id) (void)0
#define HEAD_END(k) (void)0
#endif

// A barrier for LDS hand-offs between the waves only: the fences are limited
// to the LDS address space, so global loads in flight (the next layer's weight
// prefetch) stay in flight across it instead of being drained (a plain
// __syncthreads() waits vmcnt(0))
__device__ __forceinline__ void hc_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// The weight stream of one layer: output tiles nt = nt0 + ntst * t (t < NT,
// nt < ceil(N / 16)) over the k chunks c0, c0 + cst, ... (< ceil(K / 16)),
// through a ring of HC_D chunk slots.  init() issues the weight reads of the
// first two chunks, which need nothing from the layer's input: a layer's init
// runs before the previous layer's epilogue and barrier, so those reads are
// in flight meanwhile; hc_run issues the rest of the ring.
// chunks in flight per wave; measured (C3 bench, one MI355X, interleaved
// trials): 2 -> 8.45 ms, 3 -> 8.59, 4 -> 8.67 per learn: the deeper rings cost
// occupancy (124 -> 184 VGPRs) and gain nothing
constexpr int HC_D = 2;
// 16-byte X loads per thread in flight while staging the forward's input rows
constexpr int HC_XB = 4;
static_assert(HC_D >= 2, "ring of at least two chunks");
template <int NT>
struct HcStream {
  // tile slot t's weight row as a byte offset from the (wave-uniform) matrix:
  // a scalar base and one 32-bit address register per slot, not a 64-bit pair
  const float* W;
  unsigned wo[NT];
  float4 b[HC_D][NT];
  int K, nch, c0, cst, ntv;
  // k past K (the last chunk of a K % 16 != 0 layer) reads the row's last
  // float4 instead (clamped address: no branch, no select after the load) and
  // meets A = 0 there: the LDS tiles are zero-padded up to the chunk.  Loads
  // are issued unconditionally (chunk indices clamped): a load issued on one
  // path only made the waitcnt pass assume the shorter queue everywhere and
  // wait for nearly every load in flight.
  // (NV: the first NV tile slots only, hc_run's body for a wave of NV tiles)
  template <int NV = NT>
  __device__ __forceinline__ void ldb(int c, float4 (&bb)[NT]) {
    const int lk = (threadIdx.x & 63) >> 4;
    const unsigned kb = 4u * (unsigned)min(16 * c + 4 * lk, K - 4);     // K % 4 == 0
#pragma unroll
    for (int t = 0; t < NV; ++t)
      bb[t] = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(W) + (size_t)(wo[t] + kb));
  }
  __device__ __forceinline__ void init(const float* __restrict__ W_, int ldw, int K_, int N,
                                       int nt0, int ntst, int c0_, int cst_) {
    const int li = threadIdx.x & 15;
    const int CT = (N + 15) >> 4;
    W = W_; K = K_; nch = (K + 15) >> 4; c0 = c0_; cst = cst_;
    // tiles of this wave that exist (wave-uniform)
    ntv = __builtin_amdgcn_readfirstlane(nt0 < CT ? (CT - 1 - nt0) / ntst + 1 : 0);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int n = min(16 * (nt0 + ntst * t) + li, N - 1);
      wo[t] = 4u * (unsigned)(n * ldw);          // < 4 HC_MAXK^2 bytes
    }
    ldb(min(c0, nch - 1), b[0]);
    ldb(min(c0 + cst, nch - 1), b[1]);
  }
};

// acc[rt][t] = A[16 rt .. 16 rt + 15][K] (LDS, lda) x W^T over the stream's
// tiles and chunks: RT row tiles share every weight chunk (RT = 2 halves the
// weight traffic per flop at large batches).  hc_body is the k loop over the
// first NV of the stream's NT tile slots, fully unrolled for that count.
template <int NT, int NV, int RT, bool CM>
__device__ __forceinline__ void hc_body(HcStream<NT>& S, const float* ap, int lda,
                                        f32x4 (&acc)[RT][NT]) {
  static_assert(NV >= 1 && NV <= NT, "a body for 1 .. NT tiles");
  // tile major (CM false): each tile's four k components back to back, the
  // row tiles interleaved; k-component major (CM): consecutive MFMAs go to
  // different accumulators.  Each accumulator takes x, y, z, w in order either
  // way (bit-identical sums).  Measured at C3 (interleaved trials): the forward
  // 67.5 (tile major) vs 70.1 us, the input-gradient chain 64.0 vs 62.4 us
  auto mm = [&](const float4 (&a)[RT], const float4 (&bb)[NT]) {
    if constexpr (!CM) {
#pragma unroll
      for (int t = 0; t < NV; ++t) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt][t] = mfma4(a[rt].x, bb[t].x, acc[rt][t]);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt][t] = mfma4(a[rt].y, bb[t].y, acc[rt][t]);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt][t] = mfma4(a[rt].z, bb[t].z, acc[rt][t]);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt][t] = mfma4(a[rt].w, bb[t].w, acc[rt][t]);
      }
    } else {
#pragma unroll
      for (int t = 0; t < NV; ++t)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt][t] = mfma4(a[rt].x, bb[t].x, acc[rt][t]);
#pragma unroll
      for (int t = 0; t < NV; ++t)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt][t] = mfma4(a[rt].y, bb[t].y, acc[rt][t]);
#pragma unroll
      for (int t = 0; t < NV; ++t)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt][t] = mfma4(a[rt].z, bb[t].z, acc[rt][t]);
#pragma unroll
      for (int t = 0; t < NV; ++t)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt][t] = mfma4(a[rt].w, bb[t].w, acc[rt][t]);
    }
  };
  auto lda_ = [&](int c, float4 (&o)[RT]) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
      o[rt] = *reinterpret_cast<const float4*>(ap + rt * 16 * lda + 16 * c);
  };
  const int nch = S.nch, cst = S.cst, cl = nch - 1;
  int c = S.c0;
  float4 a[HC_D][RT];
#pragma unroll
  for (int d = 2; d < HC_D; ++d) S.template ldb<NV>(min(c + d * cst, cl), S.b[d]);
#pragma unroll
  for (int d = 0; d < HC_D; ++d) lda_(min(c + d * cst, cl), a[d]);
  // steady state without conditionals (HC_D chunks per trip, every refill
  // issued): the waitcnt pass then sees the ring's loads in flight and waits
  // for exactly the slot it consumes
  for (; c + (2 * HC_D - 1) * cst < nch; c += HC_D * cst) {
#pragma unroll
    for (int d = 0; d < HC_D; ++d) {
      mm(a[d], S.b[d]);
      lda_(c + (d + HC_D) * cst, a[d]);
      S.template ldb<NV>(c + (d + HC_D) * cst, S.b[d]);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // the last < 2 HC_D chunks
#pragma unroll
  for (int d = 0; d < HC_D; ++d) {
    if (c + d * cst < nch) mm(a[d], S.b[d]);
    lda_(min(c + (d + HC_D) * cst, cl), a[d]);
    S.template ldb<NV>(min(c + (d + HC_D) * cst, cl), S.b[d]);
  }
#pragma unroll
  for (int d = 0; d < HC_D; ++d)
    if (c + (d + HC_D) * cst < nch) mm(a[d], S.b[d]);
}

// A wave runs exactly the tiles it owns: S.ntv is wave-uniform, so ONE branch
// per layer, outside the k loop, picks the body unrolled for NT, NT - 1 or
// NT - 2 tiles (a guard per tile inside the loop made the compiler move the
// accumulators out of AGPRs every chunk).  The slots past the body's count
// keep their zero accumulators and the epilogues skip them.  NT is rounded up
// to an instantiation (hc_nt, head_plan), so a wave can own fewer than NT - 2
// tiles (5 slots, 9 or 10 tiles over four waves: 2 or 3 each): it runs the
// NT - 2 body, whose surplus slots read clamped rows and are dropped like the
// others.  At the C3 widths no wave has such a slot.  EX false keeps the one
// body of NT slots, every slot run: the one-row-tile forms (with the branch
// the forward's took up to 30 more registers, <5, 4, 1> 116 -> 146 and a wave
// per SIMD fewer, and the learn at a rank's 128 segments measured 0.5 - 0.8 %
// slower) and the input-gradient chain's 8-slot forms (their accumulators are
// VGPRs beside 64 mask values; with the branch they spill 100 - 270 bytes of
// scratch per lane).
template <int NT, int RT, bool CM = false, bool EX = true>
__device__ __forceinline__ void hc_run(HcStream<NT>& S, const float* sA, int lda,
                                       f32x4 (&acc)[RT][NT]) {
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[rt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (S.ntv == 0) return;
  const float* ap = sA + li * lda + 4 * lk;
  constexpr int N1 = NT > 1 ? NT - 1 : 1, N2 = NT > 2 ? NT - 2 : N1;
  if constexpr (NT == 1 || !EX) {
    hc_body<NT, NT, RT, CM>(S, ap, lda, acc);
  } else {
    if (S.ntv >= NT) hc_body<NT, NT, RT, CM>(S, ap, lda, acc);
    else if (N2 == N1 || S.ntv >= N1) hc_body<NT, N1, RT, CM>(S, ap, lda, acc);
    else hc_body<NT, N2, RT, CM>(S, ap, lda, acc);
  }
}

// the wave's tiles of a full-width layer into LDS rows: D(row 4lk + i, col li)
// of tile nt, row tile rt, is element [16 rt + 4lk + i][16 nt + li]; EPI 0:
// + bias, ReLU; 1: * [mask > 0] (mask row-major [rows][N] in global memory,
// rows r0..); columns N..16*CT-1 are written as zeros (the next layer's last
// chunk reads them)
// Its operands (the bias, or the 4 mask values of each of the lane's rows)
// are fetched by hc_epi_load BEFORE the layer's k loop, so their latency hides
// behind it instead of serializing one tile at a time after it.  EPI 0 uses
// e[0] only (the bias is the same for every row tile).
template <int NT, int EPI, int RT>
__device__ __forceinline__ void hc_epi_load(int nt0, int N, const float* bias, const float* mask,
                                            int64_t r0, int64_t rows, float (&e)[RT][NT][4]) {
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int nc = min(16 * (nt0 + 4 * t) + li, N - 1);     // clamped: unconditional loads
    if constexpr (EPI == 0) {
      e[0][t][0] = bias[nc];
    } else {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int64_t r = r0 + 16 * rt + 4 * lk + i;
          e[rt][t][i] = mask[(r < rows ? r : rows - 1) * N + nc];
        }
    }
  }
}

template <int NT, int EPI, int RT>
__device__ __forceinline__ void hc_store(const f32x4 (&acc)[RT][NT], const float (&e)[RT][NT][4],
                                         int nt0, int N, float* sO, int ldo) {
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const int CT = (N + 15) >> 4;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int nt = nt0 + 4 * t;
    if (nt >= CT) break;
    const int n = 16 * nt + li;
    const bool nv = n < N;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 16 * rt + 4 * lk + i;
        float v;
        if constexpr (EPI == 0) {
          v = acc[rt][t][i] + e[0][t][0];
          v = v > 0.f ? v : 0.f;
        } else {
          v = e[rt][t][i] > 0.f ? acc[rt][t][i] : 0.f;
        }
        sO[r * ldo + n] = nv ? v : 0.f;
      }
  }
}

// rows r0.. of an LDS tile [16 RT][ld] (N columns, N % 4 == 0, N <= HC_MAXK) to
// global [rows][N]: thread (r, q0) copies row r's float4 columns q0, q0 + 16,
// ... of each row tile; every LDS read of a row tile first, into distinct
// registers, then its stores (a loop reusing one register made each store wait
// for the previous one)
template <int RT>
__device__ __forceinline__ void hc_copy_out(const float* sO, int ld, int N, float* __restrict__ G,
                                           int64_t r0, int64_t rows) {
  if (G == nullptr) return;                      // (no backward reads them: not stored)
  constexpr int J = HC_MAXK / 4 / 16;
  const int nq = N >> 2, q0 = threadIdx.x & 15;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int r = (threadIdx.x >> 4) + 16 * rt;
    float4 v[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int q = q0 + 16 * j;
      v[j] = q < nq ? *reinterpret_cast<const float4*>(sO + r * ld + 4 * q) : float4{0.f, 0.f, 0.f, 0.f};
    }
    if (r0 + r >= rows) continue;
    float* g = G + (r0 + r) * N;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int q = q0 + 16 * j;
      if (q < nq) *reinterpret_cast<float4*>(g + 4 * q) = v[j];
    }
  }
}

// W [M][K] -> WT [K][M] in 32 x 32 tiles (tile index tix over both matrices)
__device__ __forceinline__ void hc_transpose_tile(const float* __restrict__ W, int M, int K,
                                                  float* __restrict__ WT, int tix, float* sT) {
  const int tk = (K + 31) >> 5;
  const int m0 = (tix / tk) * 32, k0 = (tix % tk) * 32;
  __syncthreads();
  // the tile's loads unconditional (clamped), pinned, then the conditional
  // LDS stores: a load under the bounds test was its own branch with a wait,
  // four round trips per tile (round 6)
  static_assert(32 * 32 % kWG == 0, "whole tile passes");
  constexpr int TP = 32 * 32 / kWG;
  float v[TP];
#pragma unroll
  for (int i = 0; i < TP; ++i) {
    const int e = threadIdx.x + i * kWG, r = e >> 5, c = e & 31;
    v[i] = W[(int64_t)min(m0 + r, M - 1) * K + min(k0 + c, K - 1)];
  }
#pragma unroll
  for (int i = 0; i < TP; ++i) asm volatile("" : "+v"(v[i]));
#pragma unroll
  for (int i = 0; i < TP; ++i) {
    const int e = threadIdx.x + i * kWG, r = e >> 5, c = e & 31;
    if (m0 + r < M && k0 + c < K) sT[r * 33 + c] = v[i];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 32 * 32; e += kWG) {
    const int r = e >> 5, c = e & 31;           // WT row k0 + r, column m0 + c
    if (k0 + r < K && m0 + c < M) WT[(int64_t)(k0 + r) * M + m0 + c] = sT[c * 33 + r];
  }
}

// Two row tiles, both layers of at most 5 tiles per wave: at most 168 registers
// (<5, 4, 2>: 128 VGPR + 40 AGPR), the three-waves-per-SIMD step, so the shared
// carve's LDS is what lets a third workgroup onto the CU.  The bound is NOT
// stated as __launch_bounds__(kWG, 3): any minimum above one makes the compiler
// keep the accumulators in VGPRs (124 registers, no AGPRs), and that form of
// <5, 4, 2> took 79 us against 62 us at two workgroups per CU and 68 us at
// three; a change that pushes a form past 168 registers
// shows in -Rpass-analysis=kernel-resource-usage as occupancy 2
template <int NT1, int NT2, int RT>
__global__ void __launch_bounds__(kWG)
head_fwd_kernel(HeadFwdArgs a) {
  if (a.skip && a.skip[0] != 0) return;
  constexpr int R = HC_R * RT;                    // rows per workgroup
  extern __shared__ __attribute__((aligned(16))) float hsm[];
  // X and HA2 share one region (X is dead once layer 1's k loop is done: the
  // barrier after its epilogue orders that before layer 2 writes HA2): 37.5 KB
  // at C3 widths and RT = 1, four workgroups per CU.  Shared carve (RT = 2,
  // a.shared): HA1 takes its turn in that region too (o1 == 0), each tile in
  // its own leading dim, so a layer's epilogue waits at a barrier until every
  // wave's k loop has read the tile it overwrites.  Every tile is written
  // whole, all R rows up to its last 16-chunk (padding zeroed), and read no
  // further: what a wider predecessor leaves beyond it is never read.
  float* s0 = hsm;                                // [R][ld0]  X
  float* s2 = hsm;                                // [R][ld2]  HA2
  float* s1 = hsm + a.o1;                         // [R][ld1]  HA1
  float* sR = hsm + a.oR;                         // [4][RT][64][4] partials of the last layer;
                                                  // [32][33] transpose tile
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * R;
  HEAD_T0();
  if (r0 < a.rows) {
    // layer 1's weight stream and bias first: in flight while X arrives
    HcStream<NT1> S1;
    S1.init(a.W1, a.K0, a.K0, a.h1, wave, 4, 0, 1);
    float e1[RT][NT1][4];
    hc_epi_load<NT1, 0, RT>(wave, a.h1, a.b1, nullptr, r0, a.rows, e1);
    // X rows into LDS (columns K0 .. ld0 - 4 zero: the last chunk's padding),
    // HC_XB 16-byte loads per thread in flight before their LDS stores (one
    // memory round trip per batch instead of one per float4; addresses
    // clamped, the padding zeroed at the store)
    const int q0 = (a.ld0 - 4) >> 2;
    for (int e0 = threadIdx.x; e0 < R * q0; e0 += HC_XB * kWG) {
      f32x4 v[HC_XB];
#pragma unroll
      for (int k = 0; k < HC_XB; ++k) {
        const int e = min(e0 + k * kWG, R * q0 - 1);
        const int r = e / q0, q = e - r * q0;
        const int64_t rr = r0 + r < a.rows ? r0 + r : a.rows - 1;
        v[k] = *reinterpret_cast<const f32x4*>(a.X + rr * a.ldx + min(4 * q, a.K0 - 4));
      }
#pragma unroll
      for (int k = 0; k < HC_XB; ++k) {
        const int e = e0 + k * kWG;
        if (e >= R * q0) break;
        const int r = e / q0, q = e - r * q0;
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        *reinterpret_cast<f32x4*>(s0 + r * a.ld0 + 4 * q) = 4 * q < a.K0 ? v[k] : z;
      }
    }
    __syncthreads();
    HEAD_TICK(0, 0);                              // X staged
    HcStream<NT2> S2;
    float e2[RT][NT2][4];
    {   // layer 1: HA1 = relu(X W1^T + b1)
      f32x4 acc[RT][NT1];
      // every load before this point has landed (the X rows went through
      // registers into LDS), but on the path where this thread staged no X
      // the waitcnt pass still counts the stream's first chunks and the bias
      // loads in flight, and that merged state set the k loop's header waits
      // to vmcnt(4) / vmcnt(1) instead of the ring depth (vmcnt(9..5)): an
      // explicit vmcnt(0) (expcnt / lgkmcnt left at their maxima) clears it
      __builtin_amdgcn_s_waitcnt(0x0F70);
      hc_run<NT1, RT, false, RT == 2>(S1, s0, a.ld0, acc);
      HEAD_TICK(0, 1);                            // layer 1 k loop
      S2.init(a.W2, a.h1, a.h1, a.h2, wave, 4, 0, 1);     // layer 2's stream, in flight
      hc_epi_load<NT2, 0, RT>(wave, a.h2, a.b2, nullptr, r0, a.rows, e2);
      if constexpr (RT == 2) {
        if (a.shared) hc_sync();                  // X read by every wave before HA1 lands on it
      }
      hc_store<NT1, 0, RT>(acc, e1, wave, a.h1, s1, a.ld1);
    }
    hc_sync();
    HEAD_TICK(0, 2);                              // epilogue 1 + barrier
    hc_copy_out<RT>(s1, a.ld1, a.h1, a.HA1, r0, a.rows);
    HEAD_TICK(0, 3);                              // HA1 copy-out issue
    HcStream<1> S3;
    {   // layer 2: HA2 = relu(HA1 W2^T + b2)
      f32x4 acc[RT][NT2];
      hc_run<NT2, RT, false, RT == 2>(S2, s1, a.ld1, acc);
      HEAD_TICK(0, 4);                            // layer 2 k loop
      S3.init(a.W3, a.h2, a.h2, a.out, 0, 1, wave, 4);    // layer 3's stream
      if constexpr (RT == 2) {
        if (a.shared) hc_sync();                  // HA1 read (k loop and copy-out) before HA2 lands on it
      }
      hc_store<NT2, 0, RT>(acc, e2, wave, a.h2, s2, a.ld2);
    }
    hc_sync();
    HEAD_TICK(0, 5);                              // epilogue 2 + barrier
    hc_copy_out<RT>(s2, a.ld2, a.h2, a.HA2, r0, a.rows);
    {   // layer 3 (out <= 16): the waves split the k chunks, fixed-order sum
      const float bn = a.b3[li < a.out ? li : a.out - 1];
      // the value targets of the lane's rows (value-gradient epilogue), in
      // flight through layer 3
      float vr[RT][4];
      if (a.vgrad) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            vr[rt][i] = a.vret[min(r0 + 16 * rt + 4 * lk + i, a.rows - 1)];
      }
      f32x4 acc[RT][1];
      hc_run<1, RT>(S3, s2, a.ld2, acc);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
        *reinterpret_cast<float4*>(sR + ((wave * RT + rt) * 64 + lane) * 4) =
            float4{acc[rt][0][0], acc[rt][0][1], acc[rt][0][2], acc[rt][0][3]};
      hc_sync();
      // value statistics of the rows (vpart; value_rows_kernel's per-row
      // terms, ppo.py:324-331), summed below in a fixed order
      double vs[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      if (wave == 0 && li < a.out) {
        // one wait for the bias / target loads (and the HA2 copy-out stores
        // issued before them): without it the waitcnt pass, unsure of the bias
        // register across the row branches, waited vmcnt(0) in every row —
        // on the previous row's Y store
        __builtin_amdgcn_s_waitcnt(0x0F70);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int r = 16 * rt + 4 * lk + i;
            if (r0 + r >= a.rows) continue;
            const float v = ((sR[((0 * RT + rt) * 64 + lane) * 4 + i] + sR[((1 * RT + rt) * 64 + lane) * 4 + i]) +
                             (sR[((2 * RT + rt) * 64 + lane) * 4 + i] + sR[((3 * RT + rt) * 64 + lane) * 4 + i])) + bn;
            const float y = a.tanh_out ? tanhf(v) : v;
            a.Y[(r0 + r) * a.ldy + li] = y;
            if (a.vgrad) {
              const float rv = vr[rt][i];
              a.vgrad[r0 + r] = a.vscale * (y - rv);
              if (a.vpart) {
                const float e = y - rv;
                const double dd = (double)rv - (double)y;
                vs[0] += (double)(e * e);
                vs[1] += dd; vs[2] += dd * dd;
                vs[3] += (double)rv; vs[4] += (double)rv * (double)rv;
              }
            }
          }
      }
      if (a.vpart && wave == 0) {        // lanes li >= out hold zeros
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          const double t = wave_sum_d(vs[k]);
          if (lane == 0) a.vpart[(int64_t)blockIdx.x * 5 + k] = t;
        }
      }
    }
  }
  HEAD_TICK(0, 6);                                // HA2 copy-out + layer 3
  // side job for the backward of the same phase: W1^T, W2^T
  if (a.W1T) {
    const int t1 = ((a.h1 + 31) >> 5) * ((a.K0 + 31) >> 5);
    const int t2 = ((a.h2 + 31) >> 5) * ((a.h1 + 31) >> 5);
    for (int tix = blockIdx.x; tix < t1 + t2; tix += gridDim.x) {
      if (tix < t1) hc_transpose_tile(a.W1, a.h1, a.K0, a.W1T, tix, sR);
      else hc_transpose_tile(a.W2, a.h2, a.h1, a.W2T, tix - t1, sR);
    }
  }
  HEAD_TICK(0, 7);                                // transposes
  HEAD_END(0);
}

// PG: the policy loss gradient of the workgroup's rows as the prologue (the
// action width is the template's 8: out == 8)
static_assert(sizeof(PolGradShared) <= HC_PG_LDS, "head_plan counts the prologue's static LDS");
template <int NTA, int NTB, int RT, bool PG>
__global__ void __launch_bounds__(kWG, RT == 1 ? 3 : 2)
head_bwd_kernel(HeadBwdArgs a) {
  if (a.skip && a.skip[0] != 0) return;
  constexpr int R = HC_R * RT;                    // rows per workgroup
  extern __shared__ __attribute__((aligned(16))) float hsm[];
  float* s2 = hsm;                                // [R][ld2]  dH2
  float* s1 = s2 + R * a.ld2;                     // [R][ld1]  dH1
  float* sZ = s1 + R * a.ld1;                     // [R][16]   dZ
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * R;
  const int out = a.out;
  HEAD_T0();
  // dZ rows (zero past out: the dH2 pass runs whole groups of 4 k), loaded
  // first, and with them everything the dZ W3 pass's first 64 column groups
  // read: the W3 row groups that exist (KG = ceil(out / 4), one for the value
  // head) and the HA2 masks of the wave's rows, whose addresses depend on
  // nothing the barrier orders — one memory round trip before the pass
  // instead of two.  dH1's weight stream (W2^T) is issued behind them and
  // stays in flight through the pass.
  const int zr = threadIdx.x >> 4, zk = threadIdx.x & 15;
  const int nq = a.h2 >> 2;              // <= 128 column groups: at most two passes of 64
  HcStream<NTA> SA;
  // The early issue holds 16 KG + 16 RT registers through the prologue and the
  // branch on KG triples the pass's code: the two-row-tile 5-slot forms (the
  // learner's at 1024 segments; 201 -> 239 VGPRs where two waves per SIMD
  // leave 256) take both.  The one-row-tile forms (bound: three waves, 168
  // VGPRs) spilled 36 - 168 bytes with either, the 2-slot two-row-tile forms
  // fell from three waves to two: those and the 8-slot forms keep the loads
  // after the barrier, of four clamped row groups (of the two that exist in
  // the policy prologue forms, whose out is 8).
  constexpr bool EARLY = RT == 2 && NTA == 5;
  PolGradShared* pshp = nullptr;
  if constexpr (PG) {
    __shared__ PolGradShared psh;
    pshp = &psh;
  }
  // dH2 = (dZ W3) * [HA2 > 0], K = out: lane = a 4-column group, wave = 4
  // rows of each row tile; the k-ordered fmaf chain from 0 (steps k >= out add
  // 0 * w).  Per column pass, every W3 row group and the HA2 masks of all row
  // tiles are loaded before the first FMA: one memory round trip per pass
  // instead of one per (row tile, k group) — the same FMAs in the same order.
  // Returns true where the policy prologue's decision ends the launch.
  // (the dZ loads and the weight stream's first chunks ahead of the branch on
  // KG: what is in flight across it is the same on every path)
  float zv[RT];
  if constexpr (!PG) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
      zv[rt] = a.dZ[min(r0 + 16 * rt + zr, a.rows - 1) * out + min(zk, out - 1)];
    SA.init(a.W2T, a.h2, a.h2, a.h1, wave, 4, 0, 1);
  }
  auto dz_w3 = [&](auto kgc) -> bool {
    constexpr int KG = decltype(kgc)::value;     // k groups of 4 loaded (out <= 4 KG)
    f32x4 w[KG][4], m[RT][4];
    auto ldwm = [&](int q) {
#pragma unroll
      for (int g = 0; g < KG; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          w[g][j] = *reinterpret_cast<const f32x4*>(a.W3 + (int64_t)min(4 * g + j, out - 1) * a.h2 + 4 * q);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int64_t rr = min(r0 + 16 * rt + 4 * wave + i, a.rows - 1);
          m[rt][i] = *reinterpret_cast<const f32x4*>(a.HA2 + rr * a.h2 + 4 * q);
        }
    };
    auto fma_store = [&](bool qv, int q) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        f32x4 v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int g = 0; g < KG; ++g) {
          if (4 * g >= out) break;
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float z = sZ[(16 * rt + 4 * wave + i) * 16 + 4 * g + j];
              v[i][0] = fmaf(z, w[g][j][0], v[i][0]); v[i][1] = fmaf(z, w[g][j][1], v[i][1]);
              v[i][2] = fmaf(z, w[g][j][2], v[i][2]); v[i][3] = fmaf(z, w[g][j][3], v[i][3]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = 16 * rt + 4 * wave + i;
          const f32x4 o = {m[rt][i][0] > 0.f ? v[i][0] : 0.f, m[rt][i][1] > 0.f ? v[i][1] : 0.f,
                           m[rt][i][2] > 0.f ? v[i][2] : 0.f, m[rt][i][3] > 0.f ? v[i][3] : 0.f};
          if (qv) {
            *reinterpret_cast<f32x4*>(s2 + r * a.ld2 + 4 * q) = o;
            if (r0 + r < a.rows) *reinterpret_cast<f32x4*>(a.dH2 + (r0 + r) * a.h2 + 4 * q) = o;
          }
        }
      }
    };
    const bool qv0 = lane < nq;
    const int qa = qv0 ? lane : nq - 1;
    if constexpr (PG) {
      // thread t < R: row r0 + t's inputs, then the pass's operands and the
      // weight stream, then the epoch's loss weights (and, one rank, its
      // decision: every load above is in flight meanwhile), then the row's dz
      // and d/dstd terms (pol_rows.hpp, the same ops as
      // policy_rows_grad_kernel's row pass)
      constexpr int AT = 8;
      PolGradShared& psh = *pshp;
      const int t = threadIdx.x;
      const int64_t n = r0 + t;
      const bool own = t < R && n < a.rows;
      PolGradRow<AT> x;
      if (own) x.load(a.pg, n, AT);
      SA.init(a.W2T, a.h2, a.h2, a.h1, wave, 4, 0, 1);
      if constexpr (EARLY) ldwm(qa);
      float wsurr, wkl;
      PolGradPre pre;
      // one 64-partial slab per round trip: a deeper group of slabs in flight
      // pushed the one-row-tile forms into scratch spills (<5, 2, 1>: 143 -> 168
      // VGPRs + 80 B); a rank's 128 segments have 42 partials
      if (pol_grad_weights<1>(a.pg, psh, wsurr, wkl, pre)) return true;
      const PolGradCols<AT> cols(pre, psh, AT);
      const AdvNorm nadv(a.pg, pre.mom);
      float glv[AT];
#pragma unroll
      for (int j = 0; j < AT; ++j) glv[j] = 0.f;
      if (t < R) {
        float dz[AT];
        if (own) {
          pol_grad_compute<AT>(a.pg, cols, nadv, x, wsurr, wkl, dz, glv);
          st_row<AT>(a.pg.dz + n * AT, dz, AT);
        } else {
#pragma unroll
          for (int j = 0; j < AT; ++j) dz[j] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) sZ[t * 16 + j] = j < AT ? dz[j] : 0.f;
      }
      if (wave == 0) {     // R <= 64: every row on wave 0; fixed butterfly order
#pragma unroll
        for (int j = 0; j < AT; ++j) {
          const float sg = wave_sum(glv[j]);
          if (lane == 0) a.pg.lvpart[(int64_t)blockIdx.x * AT + j] = sg;
        }
      }
    } else {
      if constexpr (EARLY) ldwm(qa);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) sZ[(16 * rt + zr) * 16 + zk] = zk < out ? zv[rt] : 0.f;
    }
    // padding columns of dH2 (the next layer's last chunk)
    const int h2p = a.ld2 - 4;
    for (int e = threadIdx.x; e < R * (h2p - a.h2); e += kWG) {
      const int r = e / (h2p - a.h2), c = e - r * (h2p - a.h2);
      s2[r * a.ld2 + a.h2 + c] = 0.f;
    }
    __syncthreads();
    if constexpr (EARLY) {
      // (the barrier waits for every load above; the pins keep the operand
      // loads on its far side, where the compiler would otherwise sink them to
      // their first use)
#pragma unroll
      for (int g = 0; g < KG; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(w[g][j]));
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(m[rt][i]));
    } else {
      ldwm(qa);
    }
    fma_store(qv0, qa);
    if (nq > 64) {                       // h2 > 256: the second 64 column groups
      const bool qv = 64 + lane < nq;
      const int q = qv ? 64 + lane : nq - 1;
      ldwm(q);
      fma_store(qv, q);
    }
    return false;
  };
  {
    bool stop;
    if constexpr (PG) {
      stop = dz_w3(std::integral_constant<int, 2>{});           // out == 8
    } else if constexpr (!EARLY) {
      stop = dz_w3(std::integral_constant<int, 4>{});
    } else {
      if (out <= 4) stop = dz_w3(std::integral_constant<int, 1>{});
      else if (out <= 8) stop = dz_w3(std::integral_constant<int, 2>{});
      else stop = dz_w3(std::integral_constant<int, 4>{});
    }
    if (stop) return;
  }
  // dH1's masks, in flight behind its k loop (issued here rather than with the
  // weight prefetch: fewer registers live through the dZ W3 pass)
  float eA[RT][NTA][4];
  hc_epi_load<NTA, 1, RT>(wave, a.h1, nullptr, a.HA1, r0, a.rows, eA);
  hc_sync();
  HEAD_TICK(1, 0);                                // dZ W3 pass
  HcStream<NTB> SB;
  {   // dH1 = (dH2 W2) * [HA1 > 0] = dH2 (W2^T)^T
    f32x4 acc[RT][NTA];
    hc_run<NTA, RT, true, (RT == 2 && NTA < 8)>(SA, s2, a.ld2, acc);
    HEAD_TICK(1, 1);                              // dH1 k loop
    if (a.dxn > 0)      // dX's weight stream (rows dx0.. of W1^T), in flight
      SB.init(a.W1T + (int64_t)a.dx0 * a.h1, a.h1, a.h1, a.dxn, wave, 4, 0, 1);
    hc_store<NTA, 1, RT>(acc, eA, wave, a.h1, s1, a.ld1);
  }
  hc_sync();
  HEAD_TICK(1, 2);                                // epilogue + barrier
  hc_copy_out<RT>(s1, a.ld1, a.h1, a.dH1, r0, a.rows);
  HEAD_TICK(1, 3);                                // dH1 copy-out issue
  if (a.dxn <= 0) { HEAD_END(1); return; }
  {   // dX = dH1 W1[:, dx0 : dx0 + dxn]
    f32x4 acc[RT][NTB];
    hc_run<NTB, RT, true, RT == 2>(SB, s1, a.ld1, acc);
    HEAD_TICK(1, 4);                              // dX k loop
    const int CT = (a.dxn + 15) >> 4;
#pragma unroll
    for (int t = 0; t < NTB; ++t) {
      const int nt = wave + 4 * t;
      if (nt >= CT) break;
      const int n = 16 * nt + li;
      if (n >= a.dxn) continue;
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int64_t r = r0 + 16 * rt + 4 * lk + i;
          if (r >= a.rows) continue;
          float v = acc[rt][t][i];
          if (a.mask) v = a.mask[r * a.ldm + n] > 0.f ? v : 0.f;
          a.dX[r * a.lddx + n] = v;
        }
    }
  }
  HEAD_TICK(1, 5);                                // dX epilogue
  HEAD_END(1);
}

#ifdef SMI_PROF
extern "C" int smi_head_phase_ticks(unsigned long long* out /* [2][10] */) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_head_ticks), sizeof(g_head_ticks)) != hipSuccess)
    return SMI_E_LAUNCH;
  static const unsigned long long zero[20] = {};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_head_ticks), zero, sizeof(zero)) == hipSuccess ? SMI_OK
                                                                                        : SMI_E_LAUNCH;
}
#endif

// ------------------------------------------------------------------ host side
static bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// shapes the fused chains take (the caller falls back to the layer GEMMs
// otherwise); the backward additionally needs dxn <= 320 (its dX tiles)
bool head_fused_ok(int in, int64_t ldx, int h1, int h2, int out, const float* X,
                   const float* W1, const float* W2, const float* W3) {
  return in >= 4 && in <= 320 && in % 4 == 0 && ldx % 4 == 0 &&
         h1 >= 4 && h1 <= HC_MAXK && h1 % 4 == 0 && h2 >= 4 && h2 <= HC_MAXK && h2 % 4 == 0 &&
         out >= 1 && out <= 16 && al16(X) && al16(W1) && al16(W2) && al16(W3);
}

// (hc_rt, head_bwd_blocks, hc_nt, head_plan: smi_shapes.hpp)

int launch_head_fwd_fused(const float* X, int64_t ldx, int64_t rows, int in, const float* W1,
                          const float* b1, int h1, const float* W2, const float* b2, int h2,
                          const float* W3, const float* b3, int out, int tanh_out, float* HA1,
                          float* HA2, float* Y, int64_t ldy, float* W1T, float* W2T,
                          hipStream_t st, const int* skip, const float* vret, float* vgrad,
                          float vscale, double* vpart) {
  if (rows <= 0) return SMI_OK;
  if (vgrad && (out != 1 || !vret)) return set_error(SMI_E_ARG, "head_forward: value epilogue needs out == 1");
  if (vpart && !vgrad) return set_error(SMI_E_ARG, "head_forward: value statistics need the value epilogue");
  const HeadPlan hp = head_plan(rows, in, h1, h2, 0);
  HeadFwdArgs a{X, ldx, in, W1, b1, W2, b2, W3, b3, h1, h2, out, tanh_out, HA1, HA2, Y, ldy,
                W1T, W2T, rows, skip, hp.ld0, hp.ld1, hp.ld2, hp.fwd_o1, hp.fwd_oR, hp.fwd_shared,
                vret, vgrad, vscale};
  a.vpart = vpart;
  const int rt = hp.rt;
  const size_t lds = (size_t)hp.fwd_lds;
  const dim3 grid((unsigned)hp.grid);
  const int m1 = hp.fwd_n1, n2 = hp.fwd_n2;
  const int kslot = ktime_begin(st);
  const char* form = "head_fwd_kernel";          // the instantiation launched (smi_last_launch)
#define SMI_HF(A, B)                                                                    \
  do {                                                                                  \
    if (rt == 2) {                                                                      \
      allow_lds(head_fwd_kernel<A, B, 2>, lds);                                         \
      hipLaunchKernelGGL((head_fwd_kernel<A, B, 2>), grid, dim3(kWG), lds, st, a);      \
      form = "head_fwd_kernel<" #A "," #B ",rt2>";                                      \
    } else {                                                                            \
      allow_lds(head_fwd_kernel<A, B, 1>, lds);                                         \
      hipLaunchKernelGGL((head_fwd_kernel<A, B, 1>), grid, dim3(kWG), lds, st, a);      \
      form = "head_fwd_kernel<" #A "," #B ",rt1>";                                      \
    }                                                                                   \
  } while (0)
  // layer-1 slots {2, 5, 8} x layer-2 slots {2, 3, 4, 5, 8} (head_plan)
#define SMI_HF2(A)                                        \
  do {                                                    \
    switch (n2) {                                         \
      case 2: SMI_HF(A, 2); break;                        \
      case 3: SMI_HF(A, 3); break;                        \
      case 4: SMI_HF(A, 4); break;                        \
      case 5: SMI_HF(A, 5); break;                        \
      default: SMI_HF(A, 8); break;                       \
    }                                                     \
  } while (0)
  if (m1 == 2) SMI_HF2(2);
  else if (m1 == 5) SMI_HF2(5);
  else SMI_HF2(8);
#undef SMI_HF2
#undef SMI_HF
  ktime_end(kslot, KT_GEMM_FWD,
            2.0 * (double)rows * ((double)in * h1 + (double)h1 * h2 + (double)h2 * out), st);
  return check_launch(form);
}

int launch_head_bwd_fused(const float* dZ, int out, int64_t rows, const float* W3,
                          const float* W2T, const float* W1T, int h1, int h2, int dx0, int dxn,
                          const float* HA1, const float* HA2, float* dH2, float* dH1, float* dX,
                          int64_t lddx, const float* mask, int64_t ldm, hipStream_t st,
                          const int* skip, const PolRowArgs* pg) {
  if (rows <= 0) return SMI_OK;
  if (pg && out != 8) return set_error(SMI_E_ARG, "head_backward: the policy prologue needs out == 8");
  const HeadPlan hp = head_plan(rows, 0, h1, h2, dxn);   // (the input width shapes the forward only)
  HeadBwdArgs a{dZ, out, W3, W2T, W1T, h1, h2, dx0, dxn, HA1, HA2, dH2, dH1, dX, lddx, mask, ldm,
                rows, skip, hp.ld2, hp.ld1};
  if (pg) a.pg = *pg;
  const int rt = hp.rt;
  const size_t lds = (size_t)hp.bwd_lds;
  const dim3 grid((unsigned)hp.grid);
  const int na = hp.bwd_na, nb = hp.bwd_nb;
  const int kslot = ktime_begin(st);
  const char* form = "head_bwd_kernel";
#define SMI_HB2(A, B, P)                                                               \
  do {                                                                                 \
    if (rt == 2) {                                                                     \
      allow_lds(head_bwd_kernel<A, B, 2, P>, lds);                                     \
      hipLaunchKernelGGL((head_bwd_kernel<A, B, 2, P>), grid, dim3(kWG), lds, st, a);  \
      form = P ? "head_bwd_kernel<" #A "," #B ",rt2,pg>" : "head_bwd_kernel<" #A "," #B ",rt2>"; \
    } else {                                                                           \
      allow_lds(head_bwd_kernel<A, B, 1, P>, lds);                                     \
      hipLaunchKernelGGL((head_bwd_kernel<A, B, 1, P>), grid, dim3(kWG), lds, st, a);  \
      form = P ? "head_bwd_kernel<" #A "," #B ",rt1,pg>" : "head_bwd_kernel<" #A "," #B ",rt1>"; \
    }                                                                                  \
  } while (0)
#define SMI_HB(A, B)                                                                   \
  do {                                                                                 \
    if (pg) SMI_HB2(A, B, true);                                                       \
    else SMI_HB2(A, B, false);                                                         \
  } while (0)
  if (na == 2 && nb == 2) SMI_HB(2, 2);
  else if (na == 2) SMI_HB(2, 5);
  else if (na == 5 && nb == 2) SMI_HB(5, 2);
  else if (na == 5) SMI_HB(5, 5);
  else if (nb == 2) SMI_HB(8, 2);
  else SMI_HB(8, 5);
#undef SMI_HB
#undef SMI_HB2
  ktime_end(kslot, KT_GEMM_DX,
            2.0 * (double)rows * ((double)out * h2 + (double)h2 * h1 + (double)h1 * dxn), st);
  return check_launch(form);
}

}  // namespace smi
