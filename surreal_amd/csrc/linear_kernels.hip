// linear_kernels.hip — layer-by-layer fp32 MFMA GEMMs for networks whose
// parameters do not fit one CU's LDS (PPO heads 300x200 over B*E rows, the
// LSTM input projection and weight gradients, DDPG actor 300x200 / critic
// 400x300; builders.py:35-175, ppo_net.py:137-152).  Every dense layer's
// forward, input-gradient and weight-gradient is the same LDS-tiled GEMM with
// a different operand view and epilogue:
//   fwd:  Y[m][n]  = act(b[n] + sum_k X[m][k] W[n][k])
//   dX:   dX[m][k] = mask(Xact[m][k] > 0) * sum_n dY[m][n] W[n][k]
//   dW:   dW[n][k] (+)= sum_m dY[m][n] X[m][k];  db[n] (+)= sum_m dY[m][n]
//         (db rides along as an extra all-ones column of X).  The reduction
//         over rows is split into KSPLIT slabs (dW is a 300x100 output over
//         ~20k rows: 10 tiles alone would leave 246 CUs idle); slab partials
//         go to the workspace and a fixed-order reducer adds them
//         (deterministic, no atomics).
// Tile 64x64, K-steps of 32, 256 threads: wave w owns rows [16w, 16w+16) x 64
// columns (4 accumulators of v_mfma_f32_16x16x4_f32).  The next K-step is
// loaded into registers while the current one runs on the MFMA pipe (LDS
// double buffer, one barrier per K-step).  LDS images follow the operand's
// contiguous dimension (leading dims 36 / 80: conflict-free MFMA operand
// reads and contiguous-dimension stores).  Global loads use clamped addresses
// and are zeroed afterwards (no predicated loads: see cdna_hip_programming.md).
// This unit holds the forward and input-gradient forms and the generic tiled
// engine; the weight-gradient kernels and their host side are linear_dw.hip.
#include <cmath>
#include <algorithm>
#include <type_traits>
#define SMI_GEMM_UNIT gemm_fwd
#include "gemm_args.hpp"

namespace smi {

constexpr int GBM = 64, GBN = 64, GBK = 32;
constexpr int LD_KC = 36;     // [row][k] images (k contiguous)
constexpr int LD_RC = 80;     // [k][row] images (row contiguous)
constexpr int G_STAGE = 2560; // floats per operand image per stage

// Operand loader: one 64 (rows) x 32 (k) tile, 2048 elements, 8 per thread
// (scalar) or 2 float4 per thread (VEC: along the contiguous dimension, when
// that dimension's extent and the other stride are multiples of 4 and the base
// is 16-byte aligned — decided once per launch, a uniform branch).  Rows >=
// rdata and k >= kmax read as zero (clamped addresses, then masked); the
// all-ones column (dW bias gradient) is synthesised, never loaded.
struct TileRegs { float v[8]; };

template <bool KCONTIG>
__device__ __forceinline__ void gemm_load(const float* __restrict__ P, int64_t rs, int64_t cs,
                                          int r0, int rdata, int k0, int kmax, int ones_col,
                                          bool vec, TileRegs& t) {
  // interior tile (all 64 rows and 32 k valid, no synthesised column): plain
  // 16-byte loads, no clamps or masks
  if (vec && ones_col < 0 && r0 + 64 <= rdata && k0 + 32 <= kmax) {
    const float* base = KCONTIG ? P + (int64_t)r0 * rs + k0 : P + (int64_t)k0 * cs + r0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int q = threadIdx.x + j * kWG;
      const float* src = KCONTIG ? base + (int64_t)(q >> 3) * rs + ((q & 7) << 2)
                                 : base + (int64_t)(q >> 4) * cs + ((q & 15) << 2);
      const float4 x = *reinterpret_cast<const float4*>(src);
      t.v[4 * j + 0] = x.x; t.v[4 * j + 1] = x.y; t.v[4 * j + 2] = x.z; t.v[4 * j + 3] = x.w;
    }
    return;
  }
  if (vec) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int q = threadIdx.x + j * kWG;
      if (KCONTIG) {            // 64 rows x 8 float4 along k
        const int r = q >> 3, k = (q & 7) << 2;
        const int rr = r0 + r, kk = k0 + k;
        const int rc = rr < rdata ? rr : rdata - 1;
        const int kc = kk < kmax ? kk : kmax - 4;
        const float4 x = *reinterpret_cast<const float4*>(P + (int64_t)rc * rs + kc);
        const bool ok = rr < rdata && kk < kmax;
        t.v[4 * j + 0] = ok ? x.x : 0.f; t.v[4 * j + 1] = ok ? x.y : 0.f;
        t.v[4 * j + 2] = ok ? x.z : 0.f; t.v[4 * j + 3] = ok ? x.w : 0.f;
      } else {                  // 32 k x 16 float4 along rows
        const int k = q >> 4, r = (q & 15) << 2;
        const int rr = r0 + r, kk = k0 + k;
        const int rc = rr < rdata ? rr : rdata - 4;
        const int kc = kk < kmax ? kk : kmax - 1;
        const float4 x = *reinterpret_cast<const float4*>(P + (int64_t)kc * cs + rc);
        const bool okk = kk < kmax, ok = okk && rr < rdata;
        t.v[4 * j + 0] = ok ? x.x : 0.f; t.v[4 * j + 1] = ok ? x.y : 0.f;
        t.v[4 * j + 2] = ok ? x.z : 0.f; t.v[4 * j + 3] = ok ? x.w : 0.f;
        if (ones_col >= 0 && okk) {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (rr + e == ones_col) t.v[4 * j + e] = 1.f;
        }
      }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int idx = threadIdx.x + j * kWG;
    const int r = KCONTIG ? (idx >> 5) : (idx & 63);
    const int k = KCONTIG ? (idx & 31) : (idx >> 6);
    const int rr = r0 + r, kk = k0 + k;
    const int rc = rr < rdata ? rr : rdata - 1;
    const int kc = kk < kmax ? kk : kmax - 1;
    const float x = P[(int64_t)rc * rs + (int64_t)kc * cs];
    t.v[j] = (rr < rdata && kk < kmax) ? x : 0.f;
    if (ones_col >= 0 && rr == ones_col && kk < kmax) t.v[j] = 1.f;
  }
}

template <bool KCONTIG>
__device__ __forceinline__ void gemm_store(float* __restrict__ S, bool vec, const TileRegs& t) {
  if (vec) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int q = threadIdx.x + j * kWG;
      const float4 x = float4{t.v[4 * j], t.v[4 * j + 1], t.v[4 * j + 2], t.v[4 * j + 3]};
      if (KCONTIG) {
        const int r = q >> 3, k = (q & 7) << 2;
        *reinterpret_cast<float4*>(S + r * LD_KC + k) = x;
      } else {
        const int k = q >> 4, r = (q & 15) << 2;
        *reinterpret_cast<float4*>(S + k * LD_RC + r) = x;
      }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int idx = threadIdx.x + j * kWG;
    const int r = KCONTIG ? (idx >> 5) : (idx & 63);
    const int k = KCONTIG ? (idx & 31) : (idx >> 6);
    if (KCONTIG) S[r * LD_KC + k] = t.v[j];
    else S[k * LD_RC + r] = t.v[j];
  }
}

// A is viewed with rows = m; B with rows = n (its "row" is the output column).
template <int EPI, bool AK, bool BK>
__global__ void __launch_bounds__(kWG)
gemm_kernel(GemmArgs g) {
  if (g.skip && g.skip[0] != 0) return;
  __shared__ __attribute__((aligned(16))) float sA[2][G_STAGE];
  __shared__ __attribute__((aligned(16))) float sB[2][G_STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const TileIdx ti = gemm_tile_index();
  const int m0 = ti.mt * GBM, n0 = ti.nt * GBN;
  const int kb = ti.z * g.kchunk;
  const int ke = min(g.K, kb + g.kchunk);
  const int nk = (ke - kb + GBK - 1) / GBK;
  // B(k, n): viewed as rows n (B "row" stride b_cs), k stride b_rs
  f32x4 tot[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) tot[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  // two K-steps of operands in flight in registers (R[0], R[1]) ahead of the
  // LDS double buffer: the global loads of step kt+2 are issued before step
  // kt's MFMAs, so each load has two compute phases to land
  TileRegs ra[2], rb[2];
  const int bdata = g.ones_col >= 0 ? g.ones_col : g.N;
  if (nk > 0) {
    gemm_load<AK>(g.A, g.a_rs, g.a_cs, m0, g.M, kb, ke, -1, g.avec, ra[0]);
    gemm_load<BK>(g.B, g.b_cs, g.b_rs, n0, bdata, kb, ke, g.ones_col, g.bvec, rb[0]);
  }
  if (nk > 1) {
    gemm_load<AK>(g.A, g.a_rs, g.a_cs, m0, g.M, kb + GBK, ke, -1, g.avec, ra[1]);
    gemm_load<BK>(g.B, g.b_cs, g.b_rs, n0, bdata, kb + GBK, ke, g.ones_col, g.bvec, rb[1]);
  }
  if (nk > 0) {
    gemm_store<AK>(sA[0], g.avec, ra[0]);
    gemm_store<BK>(sB[0], g.bvec, rb[0]);
  }
  __syncthreads();
  const int ar = wave * 16 + li;
  // one K-step from LDS image `cur`; register slot `cur` refills with step
  // kt+2, slot cur^1 (step kt+1) goes to the other LDS image afterwards.  The
  // loop is unrolled by two so the slots are compile-time registers.
  auto kstep = [&](int kt, auto cur_c) {
    constexpr int cur = decltype(cur_c)::value;
    if (kt + 2 < nk) {
      gemm_load<AK>(g.A, g.a_rs, g.a_cs, m0, g.M, kb + (kt + 2) * GBK, ke, -1, g.avec, ra[cur]);
      gemm_load<BK>(g.B, g.b_cs, g.b_rs, n0, bdata, kb + (kt + 2) * GBK, ke, g.ones_col, g.bvec,
                    rb[cur]);
    }
    const float* As = sA[cur];
    const float* Bs = sB[cur];
    // two-level accumulation: each K-step (32 products per output) starts a
    // fresh MFMA chain that is then added to the running sums — fp32 error of
    // a 32-term chain plus an nk-term chain instead of one 32*nk-term chain
    f32x4 acc[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    // every operand of the K-step is read from LDS first, then 32 MFMAs run
    // back to back on 4 independent accumulator chains
    float av[8], bv[4][8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = 4 * u + lk;
      av[u] = AK ? As[ar * LD_KC + k] : As[k * LD_RC + ar];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int n = c * 16 + li;
        bv[c][u] = BK ? Bs[n * LD_KC + k] : Bs[k * LD_RC + n];
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = mfma4(av[u], bv[c][u], acc[c]);
#pragma unroll
    for (int c = 0; c < 4; ++c) tot[c] += acc[c];
    if (kt + 1 < nk) {
      gemm_store<AK>(sA[cur ^ 1], g.avec, ra[cur ^ 1]);
      gemm_store<BK>(sB[cur ^ 1], g.bvec, rb[cur ^ 1]);
    }
    __syncthreads();
  };
  for (int kt = 0; kt < nk; kt += 2) {
    kstep(kt, std::integral_constant<int, 0>{});
    if (kt + 1 < nk) kstep(kt + 1, std::integral_constant<int, 1>{});
  }
  // epilogue: 4 rows x 4 columns per lane, biases hoisted per column
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int n = n0 + c * 16 + li;
    if (n >= g.N) continue;
    float bias_n = 0.f;
    if constexpr (EPI == EPI_FWD) bias_n = g.bias ? g.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + wave * 16 + lk * 4 + i;
      if (m >= g.M) continue;
      float v = tot[c][i];
      if constexpr (EPI == EPI_FWD) {
        if (g.part) {                           // split-K slab: raw sums
          g.part[((int64_t)ti.z * g.M + m) * g.N + n] = v;
          continue;
        }
        v += bias_n;
        if (g.act == ACT_RELU) v = v > 0.f ? v : 0.f;
        else if (g.act == ACT_TANH) v = tanhf(v);
        g.C[(int64_t)m * g.ldc + n] = v;
      } else if constexpr (EPI == EPI_DX) {
        if (g.part) {                           // split-K slab: raw sums
          g.part[((int64_t)ti.z * g.M + m) * g.N + n] = v;
          continue;
        }
        if (g.mask) v = g.mask[(int64_t)m * g.ldm + n] > 0.f ? v : 0.f;
        g.C[(int64_t)m * g.ldc + n] = v;
      } else {
        if (g.part) {
          g.part[((int64_t)ti.z * g.M + m) * g.N + n] = v;
        } else if (n == g.ones_col) {
          g.bias_out[m] = g.accumulate ? g.bias_out[m] + v : v;
        } else {
          float* dst = g.C + (int64_t)m * g.ldc + n;
          *dst = g.accumulate ? *dst + v : v;
        }
      }
    }
  }
}

// split-K reducer: C[m][n] (+)= sum_z part[z][m][n]; the ones column goes to
// bias_out[m].  A workgroup owns 64 consecutive elements x 4 slab lanes: lane
// zl sums slabs zl, zl+4, ... with 4 independent accumulators (loads in
// flight), then the 4 lane sums are combined in LDS in a fixed order
// (deterministic, no atomics).
__global__ void __launch_bounds__(kWG)
gemm_splitk_reduce_kernel(const float* __restrict__ part, int S, GemmArgs g, const float* bias,
                          int act, const float* mask) {
  if (g.skip && g.skip[0] != 0) return;
  __shared__ float red[4][64];
  const int M = g.M, N = g.N;
  const int64_t MN = (int64_t)M * N;
  const int el = threadIdx.x & 63, zl = threadIdx.x >> 6;
  const int64_t e = (int64_t)blockIdx.x * 64 + el;
  const int64_t ec = e < MN ? e : MN - 1;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int z = zl;
  if (S <= 64) {
    // every slab of the thread (z = zl + 4k) in flight at once, then the same
    // additions in the same order as the loop below (bit-identical): one
    // memory round trip instead of one per four slabs
    // (loads unconditional, slabs past S read a zero by address, and pinned
    // before the conditional adds below: with `zk < S ? load : 0` the compiler
    // sank each load into its own branch and waited on it there -- up to 16
    // round trips per block, round 6)
    // (addresses advanced by 4 slabs per k: the 64-bit index products per
    // load made the allocator reuse address registers and wait between loads)
    const float* pz = part + (int64_t)zl * MN + ec;
    const int64_t st4 = 4 * MN;
    float v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = *(zl + 4 * k < S ? pz + k * st4 : g_dwd_zero);
#pragma unroll
    for (int k = 0; k < 16; ++k) asm volatile("" : "+v"(v[k]));
    const int nfull = S > zl + 12 ? (S - zl - 12 + 15) / 16 : 0;   // z + 12 < S trips
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < nfull) {
        s0 += v[4 * j]; s1 += v[4 * j + 1]; s2 += v[4 * j + 2]; s3 += v[4 * j + 3];
      }
    }
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (k >= 4 * nfull && zl + 4 * k < S) s0 += v[k];
    z = S;
  }
  for (; z + 12 < S; z += 16) {
    s0 += part[(int64_t)z * MN + ec];
    s1 += part[(int64_t)(z + 4) * MN + ec];
    s2 += part[(int64_t)(z + 8) * MN + ec];
    s3 += part[(int64_t)(z + 12) * MN + ec];
  }
  for (; z < S; z += 4) s0 += part[(int64_t)z * MN + ec];
  red[zl][el] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (zl != 0 || e >= MN) return;
  float s = (red[0][el] + red[1][el]) + (red[2][el] + red[3][el]);
  const int m = (int)(e / N), n = (int)(e - (int64_t)m * N);
  if (bias) s += bias[n];                       // split-K forward epilogue
  if (act == ACT_RELU) s = s > 0.f ? s : 0.f;
  else if (act == ACT_TANH) s = tanhf(s);
  if (mask && !(mask[(int64_t)m * g.ldm + n] > 0.f)) s = 0.f;   // split-K input gradient
  dw_put(g, m, n, s);
}

// Small-K forward (K <= 64: the LSTM input projection x W_ih^T over the
// observation width, the first layer of the DDPG nets).  The tiled kernel is
// latency-bound there (two K-steps per 64x64 tile, prologue and epilogue
// dominate); this one stages the whole weight W[N][K] (zero-padded to 4*NKU
// k) in LDS once per workgroup, keeps a 64-row tile of X in registers as MFMA
// A operands, and sweeps all N columns in groups of four 16-column blocks
// (four independent NKU-long MFMA chains).  Workgroups are persistent over row
// tiles.
template <int NKU>
__global__ void __launch_bounds__(kWG)
gemm_smallk_fwd_kernel(const float* __restrict__ X, int64_t ldx, int M, int K,
                       const float* __restrict__ W, int64_t ldw, const float* __restrict__ bias,
                       int N, int act, float* __restrict__ Y, int64_t ldy, const int* skip) {
  if (skip && skip[0] != 0) return;
  extern __shared__ __attribute__((aligned(16))) float sW[];
  constexpr int LDK = 4 * NKU + 1;                  // odd: conflict-free B reads
  constexpr int LDO = 68;                           // output staging [16][68] per wave
  float* sb = sW + N * LDK;
  float* so = sb + ((N + 3) & ~3) + (threadIdx.x >> 6) * 16 * LDO;
  // staging: 8 independent loads in flight per thread (a plain loop waits for
  // each load before the next: ~80 serialised L2 round trips per thread)
  {
    const int tot = N * LDK;
    for (int e0 = threadIdx.x; e0 < tot; e0 += 8 * kWG) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int e = e0 + j * kWG;
        const int ec = e < tot ? e : tot - 1;
        const int n = ec / LDK, k = ec - n * LDK;
        const float x = W[(int64_t)n * ldw + (k < K ? k : K - 1)];
        v[j] = k < K ? x : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int e = e0 + j * kWG;
        if (e < tot) sW[e] = v[j];
      }
    }
  }
  for (int n = threadIdx.x; n < N; n += kWG) sb[n] = bias ? bias[n] : 0.f;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
  const bool vec_out = ((reinterpret_cast<uintptr_t>(Y) & 15) == 0) && (ldy % 4 == 0);
  for (int tile = blockIdx.x; tile * 64 < M; tile += gridDim.x) {
    const int m = tile * 64 + wave * 16 + li;
    const int mc = m < M ? m : M - 1;
    float a[NKU];
#pragma unroll
    for (int u = 0; u < NKU; ++u) {
      const int k = 4 * u + lk;
      const float x = X[(int64_t)mc * ldx + (k < K ? k : K - 1)];
      a[u] = k < K ? x : 0.f;
    }
    for (int nb = 0; nb < N; nb += 64) {
      f32x4 acc[4];
      const float* w[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int n = nb + c * 16 + li;
        w[c] = sW + (n < N ? n : N - 1) * LDK + lk;
      }
      // all B operands of the group first (one LDS round trip), then the MFMAs
      float bw[4][NKU];
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int u = 0; u < NKU; ++u) bw[c][u] = w[c][4 * u];
#pragma unroll
      for (int u = 0; u < NKU; ++u)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = mfma4(a[u], bw[c][u], acc[c]);
      // epilogue through the wave's LDS slab: rows leave as 16-byte stores
      // (a wave-instruction writes 4 rows x 256 contiguous bytes)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int col = nb + c * 16 + li;
        const float bn = col < N ? sb[col] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float v = acc[c][i] + bn;
          if (act == ACT_RELU) v = v > 0.f ? v : 0.f;
          else if (act == ACT_TANH) v = tanhf(v);
          so[(lk * 4 + i) * LDO + c * 16 + li] = v;
        }
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = j * 4 + (lane >> 4), c4 = (lane & 15) * 4;
        const int row = tile * 64 + wave * 16 + r, col = nb + c4;
        const float4 v = *reinterpret_cast<const float4*>(so + r * LDO + c4);
        if (row < M) {
          float* dst = Y + (int64_t)row * ldy + col;
          if (vec_out && col + 3 < N) {
            *reinterpret_cast<float4*>(dst) = v;
          } else {
            if (col < N) dst[0] = v.x;
            if (col + 1 < N) dst[1] = v.y;
            if (col + 2 < N) dst[2] = v.z;
            if (col + 3 < N) dst[3] = v.w;
          }
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
}

static int launch_smallk_fwd(const float* X, int64_t ldx, int M, int K, const float* W,
                             int64_t ldw, const float* b, int N, int act, float* Y, int64_t ldy,
                             hipStream_t st, const int* skip) {
  const int nku = (K + 3) / 4 <= 4 ? 4 : (K + 3) / 4 <= 8 ? 8 : (K + 3) / 4 <= 12 ? 12 : 16;
  const size_t lds = ((size_t)N * (4 * nku + 1) + ((N + 3) & ~3) + 4 * 16 * 68) * 4;
  const int tiles = (M + 63) / 64;
  const int kslot = ktime_begin(st);
  const char* form = "gemm_smallk_fwd_kernel";
#define SMI_SK_CASE(V)                                                                         \
  if (nku == V) {                                                                              \
    form = "gemm_smallk_fwd_kernel<" #V ">";                                                   \
    auto k = gemm_smallk_fwd_kernel<V>;                                                        \
    allow_lds(k, lds);                                                                         \
    static int cap = 0;                                                                        \
    if (!cap) cap = resident_grid(k, kWG, lds);                                                \
    const int grid = tiles < cap ? tiles : cap;                                                \
    hipLaunchKernelGGL(k, dim3(grid), dim3(kWG), lds, st, X, ldx, M, K, W, ldw, b, N, act, Y, \
                       ldy, skip);                                                             \
  }
  SMI_SK_CASE(4) SMI_SK_CASE(8) SMI_SK_CASE(12) SMI_SK_CASE(16)
#undef SMI_SK_CASE
  ktime_end(kslot, KT_GEMM_FWD, 2.0 * M * (double)N * K, st);
  return check_launch(form);
}

// Row-panel GEMM for the learner's tall activations (rows >> N, K small):
//   EPI_FWD: Y = act(X W^T + b)        EPI_DX: dX = (dY W) * [mask > 0]
// A workgroup owns 64 rows x 16*NTW output columns, one 16-row MFMA tile per
// wave.  The A operand goes from global memory straight into MFMA registers
// as 16-byte k-runs (lane (li, lk) loads row li, k 4lk..4lk+3 of a 16-k
// chunk; B is staged with the same k permutation), so every activation row
// is read once per column group; the weight chunk B[16 k][16*NTW n] is
// staged in LDS once per workgroup and shared by the four waves (one barrier
// per chunk).  k past K reads a zero row by address (g_dwd_zero).
constexpr int PN_LD = 20;

template <int EPI, int NTW>
__global__ void __launch_bounds__(kWG)
gemm_panel_kernel(GemmArgs g) {
  if (g.skip && g.skip[0] != 0) return;
  constexpr int NB = 16 * NTW;                    // columns per workgroup
  constexpr int BQ = (4 * NB + kWG - 1) / kWG;    // staged float4 per thread
  __shared__ __attribute__((aligned(16))) float sB[2][NB * PN_LD + 4];   // + dummy slot
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const TileIdx ti = gemm_tile_index();
  const int r0 = ti.mt * 64 + wave * 16;
  const int n0 = ti.nt * NB;
  const int nch = (g.K + 15) >> 4;
  const float* arow = g.A + (int64_t)min(r0 + li, g.M - 1) * g.a_rs;
  auto load_a = [&](int c) -> float4 {
    const int k = c * 16 + 4 * lk;
    return *reinterpret_cast<const float4*>(k < g.K ? arow + k : g_dwd_zero);
  };
  // staging: FWD B(k, n) = W[n][k] (k-contiguous rows); DX B(k, n) = W[k][n].
  // Slot q of this thread is element idx = tid + q*256 of the chunk; slots past
  // the chunk (idx >= 4*NB) load the zero row and write the dummy LDS slot (no
  // divergent branches: the staging values stay in named registers)
  auto load_b = [&](int c, int q) -> float4 {
    const int idx = tid + q * kWG;
    const float* src;
    if constexpr (EPI == EPI_FWD) {
      const int n = idx >> 2, k = c * 16 + ((idx & 3) << 2);
      const int nc = min(n0 + n, g.N - 1);
      src = (idx < 4 * NB && k < g.K) ? g.B + (int64_t)nc * g.b_cs + k : g_dwd_zero;
    } else {
      const int k = idx / (NB / 4), nq = (idx - k * (NB / 4)) << 2;
      const int kk = c * 16 + k;
      const int nc = min(n0 + nq, g.N - 4);
      src = (idx < 4 * NB && kk < g.K) ? g.B + (int64_t)kk * g.b_rs + nc : g_dwd_zero;
    }
    return *reinterpret_cast<const float4*>(src);
  };
  auto store_b = [&](float* S, int q, float4 r) {
    const int idx = tid + q * kWG;
    const bool ok = idx < 4 * NB;
    if constexpr (EPI == EPI_FWD) {
      const int n = idx >> 2, kq = (idx & 3) << 2;
      *reinterpret_cast<float4*>(S + (ok ? n * PN_LD + kq : NB * PN_LD)) = r;
    } else {
      const int k = idx / (NB / 4), nq = (idx - k * (NB / 4)) << 2;
      const int base = ok ? nq * PN_LD + k : NB * PN_LD;
      const int step = ok ? PN_LD : 1;
      S[base] = r.x; S[base + step] = r.y; S[base + 2 * step] = r.z; S[base + 3 * step] = r.w;
    }
  };
  f32x4 acc[NTW];
#pragma unroll
  for (int b = 0; b < NTW; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
  static_assert(BQ <= 3, "panel staging: at most 3 float4 per thread");
  float4 b0, b1, b2;
  float4 aC = load_a(0), aN;
  b0 = load_b(0, 0);
  if constexpr (BQ > 1) b1 = load_b(0, 1);
  if constexpr (BQ > 2) b2 = load_b(0, 2);
  store_b(sB[0], 0, b0);
  if constexpr (BQ > 1) store_b(sB[0], 1, b1);
  if constexpr (BQ > 2) store_b(sB[0], 2, b2);
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    const bool more = c + 1 < nch;
    if (more) {
      aN = load_a(c + 1);
      b0 = load_b(c + 1, 0);
      if constexpr (BQ > 1) b1 = load_b(c + 1, 1);
      if constexpr (BQ > 2) b2 = load_b(c + 1, 2);
    }
    const float* S = sB[c & 1];
    float4 bq[NTW];
#pragma unroll
    for (int b = 0; b < NTW; ++b)
      bq[b] = *reinterpret_cast<const float4*>(S + (16 * b + li) * PN_LD + 4 * lk);
#pragma unroll
    for (int b = 0; b < NTW; ++b) {
      acc[b] = mfma4(aC.x, bq[b].x, acc[b]);
      acc[b] = mfma4(aC.y, bq[b].y, acc[b]);
      acc[b] = mfma4(aC.z, bq[b].z, acc[b]);
      acc[b] = mfma4(aC.w, bq[b].w, acc[b]);
    }
    if (more) {
      float* S1 = sB[(c + 1) & 1];
      store_b(S1, 0, b0);
      if constexpr (BQ > 1) store_b(S1, 1, b1);
      if constexpr (BQ > 2) store_b(S1, 2, b2);
      aC = aN;
    }
    __syncthreads();
  }
#pragma unroll
  for (int b = 0; b < NTW; ++b) {
    const int n = n0 + 16 * b + li;
    if (n >= g.N) continue;
    float bias_n = 0.f;
    if constexpr (EPI == EPI_FWD) bias_n = g.bias ? g.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = r0 + 4 * lk + i;
      if (m >= g.M) continue;
      float v = acc[b][i];
      if constexpr (EPI == EPI_FWD) {
        v += bias_n;
        if (g.act == ACT_RELU) v = v > 0.f ? v : 0.f;
        else if (g.act == ACT_TANH) v = tanhf(v);
      } else {
        if (g.mask) v = g.mask[(int64_t)m * g.ldm + n] > 0.f ? v : 0.f;
      }
      g.C[(int64_t)m * g.ldc + n] = v;
    }
  }
}

// split-K target workgroup count
constexpr int kSplitkTarget = 512;

template <int EPI>
static void gemm_dispatch(const GemmArgs& g, dim3 grid, bool ak, bool bk, hipStream_t st) {
  if (ak && bk) hipLaunchKernelGGL((gemm_kernel<EPI, true, true>), grid, dim3(kWG), 0, st, g);
  else if (ak) hipLaunchKernelGGL((gemm_kernel<EPI, true, false>), grid, dim3(kWG), 0, st, g);
  else if (bk) hipLaunchKernelGGL((gemm_kernel<EPI, false, true>), grid, dim3(kWG), 0, st, g);
  else hipLaunchKernelGGL((gemm_kernel<EPI, false, false>), grid, dim3(kWG), 0, st, g);
}

// returns the launched instantiation's name (smi_last_launch)
template <int EPI>
static const char* panel_dispatch(const GemmArgs& g, dim3 grid, int ntw, hipStream_t st) {
#define SMI_PN(C)                                                                      \
  hipLaunchKernelGGL((gemm_panel_kernel<EPI, C>), grid, dim3(kWG), 0, st, g);          \
  return EPI == EPI_FWD ? "gemm_panel_kernel<fwd," #C ">" : "gemm_panel_kernel<dx," #C ">"
  switch (ntw) {
    case 1: SMI_PN(1);
    case 2: SMI_PN(2);
    case 4: SMI_PN(4);
    case 5: SMI_PN(5);
    case 7: SMI_PN(7);
    default: SMI_PN(10);
  }
#undef SMI_PN
}

// tall forward / input-gradient GEMMs with 16-byte operands: gemm_panel_kernel
static bool panel_ok(int epi, const GemmArgs& g) {
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  // below kPanelMinRows the row panels cannot fill the GPU and their serial K
  // loop is the latency: the tiled kernel with split-K takes those (measured at
  // 128 segments per GPU, 2688 / 3328 rows: forwards + input gradients 2.43 ->
  // 1.69 ms per learn, +0.72 ms of split-K reduces, learn 6.10 -> 5.81 ms)
  constexpr int kPanelMinRows = 4096;
  if (g.M < kPanelMinRows || g.N > 640 || g.K > 1024 || g.K < 1) return false;
  if (g.a_cs != 1 || g.a_rs % 4 || g.K % 4 || !al16(g.A) || !al16(g.B)) return false;
  if (epi == EPI_FWD) return g.b_rs == 1 && g.b_cs % 4 == 0;
  // input gradients: the transposing LDS stage costs more than it saves below
  // ~96 output columns (in the C3 learner 300->100 runs 16 % faster here than
  // on gemm_kernel)
  constexpr int kPanelDxMin = 96;
  if (epi == EPI_DX)
    return g.b_cs == 1 && g.b_rs % 4 == 0 && g.N % 4 == 0 && g.N >= kPanelDxMin;
  return false;
}

static int panel_launch(int epi, const GemmArgs& g, hipStream_t st) {
  // column-group width: fewest padded 16-column tiles, then fewer groups
  static const int cand[6] = {1, 2, 4, 5, 7, 10};
  const int t16 = (g.N + 15) / 16;
  int best = 10;
  double bcost = 1e30;
  for (int c : cand) {
    const int groups = (t16 + c - 1) / c;
    const double cost = groups * c + 0.3 * groups;
    if (cost < bcost) { bcost = cost; best = c; }
  }
  const dim3 grid((g.M + 63) / 64, (g.N + 16 * best - 1) / (16 * best), 1);
  const int kslot = ktime_begin(st);
  const char* form = epi == EPI_FWD ? panel_dispatch<EPI_FWD>(g, grid, best, st)
                                    : panel_dispatch<EPI_DX>(g, grid, best, st);
  ktime_end(kslot, epi == EPI_FWD ? KT_GEMM_FWD : KT_GEMM_DX, 2.0 * g.M * (double)g.N * g.K, st);
  return check_launch(form);
}

// Input gradient through a layer with at most 8 outputs (the value head's
// 200 -> 1, the action head's 200 -> 8): dX = (dY W) * [mask > 0] is a
// rank-<=8 update, pure streaming (read dY row + mask, write dX), so it skips
// the MFMA tiles (which pad K to 16/32).  Per element: the k-ordered fmaf
// chain from 0 (for K = 1 bit-identical to the tiled path).  A thread owns 4
// consecutive columns of 4 rows (the W slice in registers, 16-byte mask reads
// and stores, coalesced along the row).
template <int KK, bool V4, bool A4 = false>
__global__ void __launch_bounds__(kWG)
dx_smallk_kernel(GemmArgs g) {
  if (g.skip && g.skip[0] != 0) return;
  constexpr int RW = 4;                            // rows per thread
  const int nq = (g.N + 3) >> 2;
  const int64_t idx = (int64_t)blockIdx.x * kWG + threadIdx.x;
  if (idx >= (int64_t)((g.M + RW - 1) / RW) * nq) return;
  const int mg = (int)(idx / nq), n0 = (int)(idx - (int64_t)mg * nq) * 4;
  // W rows k (4 columns each), shared by the thread's RW rows
  float w[KK][4];
#pragma unroll
  for (int k = 0; k < KK; ++k) {
    const float* wr = g.B + (int64_t)min(k, g.K - 1) * g.b_rs;
    if constexpr (V4) {
      const float4 x = *reinterpret_cast<const float4*>(wr + n0);
      w[k][0] = x.x; w[k][1] = x.y; w[k][2] = x.z; w[k][3] = x.w;
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) w[k][t] = wr[min(n0 + t, g.N - 1)];
    }
  }
#pragma unroll
  for (int r = 0; r < RW; ++r) {
    const int m = mg * RW + r;
    if (m >= g.M) break;
    const float* arow = g.A + (int64_t)m * g.a_rs;
    float av[KK];
    if (KK % 4 == 0 && A4) {                       // K == KK: 16-byte row loads
#pragma unroll
      for (int q = 0; q < KK / 4; ++q) {
        const float4 x = reinterpret_cast<const float4*>(arow)[q];
        av[4 * q] = x.x; av[4 * q + 1] = x.y; av[4 * q + 2] = x.z; av[4 * q + 3] = x.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < KK; ++k) av[k] = k < g.K ? arow[k] : 0.f;
    }
    float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < KK; ++k) {
      if (k >= g.K) break;
#pragma unroll
      for (int t = 0; t < 4; ++t) v[t] = fmaf(av[k], w[k][t], v[t]);
    }
    const float* mrow = g.mask ? g.mask + (int64_t)m * g.ldm + n0 : nullptr;
    float* crow = g.C + (int64_t)m * g.ldc + n0;
    if constexpr (V4) {
      if (mrow) {
        const float4 mk = *reinterpret_cast<const float4*>(mrow);
        v[0] = mk.x > 0.f ? v[0] : 0.f; v[1] = mk.y > 0.f ? v[1] : 0.f;
        v[2] = mk.z > 0.f ? v[2] : 0.f; v[3] = mk.w > 0.f ? v[3] : 0.f;
      }
      *reinterpret_cast<float4*>(crow) = float4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (n0 + t >= g.N) break;
        crow[t] = (mrow && !(mrow[t] > 0.f)) ? 0.f : v[t];
      }
    }
  }
}

static int dx_smallk_launch(const GemmArgs& g, hipStream_t st) {
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const bool v4 = g.N % 4 == 0 && g.ldc % 4 == 0 && al16(g.C) && g.b_rs % 4 == 0 && al16(g.B) &&
                  (!g.mask || (g.ldm % 4 == 0 && al16(g.mask)));
  const int64_t n = (int64_t)((g.M + 3) / 4) * ((g.N + 3) / 4);
  const dim3 grid((unsigned)((n + kWG - 1) / kWG));
  const int kslot = ktime_begin(st);
  const char* form;
#define SMI_DXS(KK)                                                                        \
  do {                                                                                     \
    if (v4) hipLaunchKernelGGL((dx_smallk_kernel<KK, true>), grid, dim3(kWG), 0, st, g);   \
    else hipLaunchKernelGGL((dx_smallk_kernel<KK, false>), grid, dim3(kWG), 0, st, g);     \
    form = v4 ? "dx_smallk_kernel<" #KK ",v4>" : "dx_smallk_kernel<" #KK ">";              \
  } while (0)
  const bool a4 = (g.K == 4 || g.K == 8) && g.a_rs % 4 == 0 && al16(g.A);
  if (g.K == 1) SMI_DXS(1);
  else if (g.K <= 2) SMI_DXS(2);
  else if (g.K == 8 && a4 && v4) {
    hipLaunchKernelGGL((dx_smallk_kernel<8, true, true>), grid, dim3(kWG), 0, st, g);
    form = "dx_smallk_kernel<8,v4,a4>";
  }
  else if (g.K <= 4) SMI_DXS(4);
  else SMI_DXS(8);
#undef SMI_DXS
  ktime_end(kslot, KT_GEMM_DX, 2.0 * g.M * (double)g.N * g.K, st);
  return check_launch(form);
}

// Forwards and input gradients of short batches (M <= 4096 rows: DDPG's 512-row
// layers) in ONE launch without split-K: a workgroup owns one 16 x 16 output
// tile and its four waves split K (wave w takes the 16-k chunks c = w, w + 4,
// ...), every chunk's operands loaded up front (one memory round trip), a
// fixed-order LDS sum of the four waves' accumulators, then the epilogue (bias
// + activation, or the input gradient's ReLU mask).  Lane (i, q) = (lane & 15,
// lane >> 4) takes k = 16c + 4q + s at MFMA s of a chunk on both operands (the
// k order permuted identically: every chunk adds its exact 16-term sum), so a
// k-contiguous operand is one 16-byte load per chunk.  The split-K form this
// replaces needed a second launch (the reducer) and ran a 64 x 64 tile's
// serial K loop per slab.
template <int EPI>
__global__ void __launch_bounds__(kWG)
gemm_t16_kernel(GemmArgs g) {
  if (g.skip && g.skip[0] != 0) return;
  __shared__ f32x4 red[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int m0 = blockIdx.x * 16, n0 = blockIdx.y * 16;
  const int ra = min(m0 + i, g.M - 1), cb = min(n0 + i, g.N - 1);
  const float* Ar = g.A + (int64_t)ra * g.a_rs;
  const float* Bc = g.B + (int64_t)cb * g.b_cs;
  const int nch = (g.K + 15) >> 4;
  // 16-byte k runs only where k is the contiguous direction (avec / bvec are
  // also set for the other orientation)
  const bool a4 = g.avec && g.a_cs == 1, b4 = g.bvec && g.b_rs == 1;
  float av[T16_MAXC][4], bv[T16_MAXC][4];
#pragma unroll
  for (int j = 0; j < T16_MAXC; ++j) {
    const int c = wave + 4 * j;
    const int k0 = 16 * c + 4 * q;
    if (c >= nch) break;
    if (a4 && k0 + 3 < g.K) {
      const float4 x = *reinterpret_cast<const float4*>(Ar + k0);
      av[j][0] = x.x; av[j][1] = x.y; av[j][2] = x.z; av[j][3] = x.w;
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) av[j][t] = k0 + t < g.K ? Ar[(int64_t)(k0 + t) * g.a_cs] : 0.f;
    }
    if (b4 && k0 + 3 < g.K) {
      const float4 x = *reinterpret_cast<const float4*>(Bc + k0);
      bv[j][0] = x.x; bv[j][1] = x.y; bv[j][2] = x.z; bv[j][3] = x.w;
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) bv[j][t] = k0 + t < g.K ? Bc[(int64_t)(k0 + t) * g.b_rs] : 0.f;
    }
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < T16_MAXC; ++j) {
    if (wave + 4 * j >= nch) break;
#pragma unroll
    for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j][t], bv[j][t], acc, 0, 0, 0);
  }
  red[wave][lane] = acc;
  __syncthreads();
  if (EPI == EPI_FWD && wave == 1 && blockIdx.y == 0 && g.xsrc) {
    for (int e = lane; e < 16 * g.xcols; e += 64) {
      const int r = e / g.xcols, j = e - r * g.xcols;
      if (m0 + r < g.M) g.C[(int64_t)(m0 + r) * g.ldc + g.N + j] = g.xsrc[(int64_t)(m0 + r) * g.xlds + j];
    }
  }
  if (wave != 0) return;
  const f32x4 sum = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
  // D(row 4q + r, col i)
  const int n = n0 + i;
  if (n >= g.N) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = m0 + 4 * q + r;
    if (m >= g.M) continue;
    float v = sum[r];
    if constexpr (EPI == EPI_FWD) {
      if (g.bias) v += g.bias[n];
      if (g.act == ACT_RELU) v = v > 0.f ? v : 0.f;
      else if (g.act == ACT_TANH) v = tanhf(v);
    } else {
      if (g.mask && !(g.mask[(int64_t)m * g.ldm + n] > 0.f)) v = 0.f;
    }
    g.C[(int64_t)m * g.ldc + n] = v;
  }
}

// the forms chosen by shape alone.  Small-K forward (gemm_smallk_fwd_kernel):
static bool takes_smallk_fwd(int M, int N, int K) {
  return K >= 1 && K <= 64 && N >= 32 && N <= 512 && M >= 2048;
}
// the short-batch kernel (gemm_t16_kernel) for every forward / input gradient
// whose 64 x 64 tiling leaves the GPU mostly idle (< 256 tiles), split-K or not
static bool takes_t16(int M, int N, int K) {
  const int gm = (M + GBM - 1) / GBM, gn = (N + GBN - 1) / GBN;
  return gm * gn < 256 && M <= 4096 && K <= 4 * 16 * T16_MAXC;
}

// (EPI_DW: what launch_linear_bwd_dw's row-major forms did not take)
int gemm_launch(int epi, GemmArgs g, hipStream_t st) {
  if (g.M <= 0 || g.N <= 0) return SMI_OK;
  g.part = nullptr;
  if (epi == EPI_DX && g.K >= 1 && g.K <= 8 && g.a_cs == 1 && g.b_cs == 1)
    return dx_smallk_launch(g, st);
  if (epi != EPI_DW && !g.xsrc && panel_ok(epi, g)) return panel_launch(epi, g, st);
  const bool ak = g.a_cs == 1;         // A contiguous along k
  const bool bk = g.b_rs == 1;         // B contiguous along k (rows n)
  auto al16 = [](const float* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  // VEC needs the contiguous extent and the other stride in multiples of 4
  // (every K-slab boundary is then a multiple of 4 too: kchunk % 32 == 0)
  g.avec = al16(g.A) && (ak ? (g.K % 4 == 0 && g.a_rs % 4 == 0) : (g.a_rs == 1 && g.M % 4 == 0 && g.a_cs % 4 == 0));
  const int bdata = g.ones_col >= 0 ? g.ones_col : g.N;
  g.bvec = al16(g.B) && (bk ? (g.K % 4 == 0 && g.b_cs % 4 == 0) : (g.b_cs == 1 && bdata % 4 == 0 && g.b_rs % 4 == 0));
  // 128x128 weight-gradient tiles when both operands are row-contiguous
  // float4-able slabs and the output is large enough to need them
  const int breal = g.ones_col >= 0 ? g.ones_col : g.N;
  const bool dw128 = epi == EPI_DW && !ak && !bk && g.a_rs == 1 && g.b_cs == 1 &&
                     al16(g.A) && al16(g.B) && g.M % 4 == 0 && breal % 4 == 0 &&
                     g.a_cs % 4 == 0 && g.b_rs % 4 == 0 && g.M >= 96 && g.N >= 96 &&
                     g.K >= 1024;
  const int TM = dw128 ? D2_T : GBM, TN = dw128 ? D2_T : GBN;
  const int gm = (g.M + TM - 1) / TM, gn = (g.N + TN - 1) / TN;
  int S = 1;
  g.part = nullptr;
  g.kchunk = g.K > 0 ? g.K : 1;
  // split-K: weight gradients (K = rows), and forwards / input gradients whose
  // output has too few tiles to fill the GPU over K >= 128 (the pixel stem's
  // 2592 -> 256 FC; DDPG's 512-row layers: 40 tiles, a serial K loop per tile
  // otherwise; C4 +20 %).  The reducer applies bias/activation or the ReLU mask.
  constexpr int kFwdSplitkMin = 4 * GBK;
  const bool split_fwd = (epi == EPI_FWD || epi == EPI_DX) && gm * gn < 256 &&
                         g.K >= kFwdSplitkMin;
  if ((epi == EPI_FWD || epi == EPI_DX) && takes_t16(g.M, g.N, g.K)) {
    const dim3 grid16((g.M + 15) / 16, (g.N + 15) / 16);
    const int kslot = ktime_begin(st);
    if (epi == EPI_FWD) hipLaunchKernelGGL(gemm_t16_kernel<EPI_FWD>, grid16, dim3(kWG), 0, st, g);
    else hipLaunchKernelGGL(gemm_t16_kernel<EPI_DX>, grid16, dim3(kWG), 0, st, g);
    ktime_end(kslot, epi == EPI_FWD ? KT_GEMM_FWD : KT_GEMM_DX, 2.0 * g.M * (double)g.N * g.K, st);
    return check_launch(epi == EPI_FWD ? "gemm_t16_kernel<fwd>" : "gemm_t16_kernel<dx>");
  }
  if ((epi == EPI_DW && g.K > 4 * GBK) || split_fwd) {
    const int tiles = gm * gn;
    S = (kSplitkTarget + tiles - 1) / tiles;    // ~2-4 workgroups per CU
    const int smax = (g.K + 4 * GBK - 1) / (4 * GBK);   // >= 4 K-steps per slab
    if (S > smax) S = smax;
    const int64_t cap = smi_workspace_floats() / ((int64_t)g.M * g.N);
    if (S > cap) S = (int)cap;
    if (S < 1) S = 1;
    // one MFMA chain per slab: <= 512 rows (longer fixed slabs measured slower:
    // fewer workgroups in flight outweigh the smaller partial traffic)
    if (dw128 && (g.K + S - 1) / S > 512) S = (g.K + 511) / 512;
    if (S > cap) S = (int)cap;
    if (S < 1) S = 1;
    if (S > 1) {
      g.kchunk = ((g.K + S - 1) / S + 31) / 32 * 32;
      S = (g.K + g.kchunk - 1) / g.kchunk;
      g.part = workspace_f32((int64_t)S * g.M * g.N);
      if (!g.part) return set_error(SMI_E_ARG, "gemm: workspace unavailable for split-K");
    }
  }
  const dim3 grid(gm, gn, S);
  const int kslot = ktime_begin(st);
  if (dw128) dw128_dispatch(g, grid, st);
  else if (epi == EPI_FWD) gemm_dispatch<EPI_FWD>(g, grid, ak, bk, st);
  else if (epi == EPI_DX) gemm_dispatch<EPI_DX>(g, grid, ak, bk, st);
  else gemm_dispatch<EPI_DW>(g, grid, ak, bk, st);
  ktime_end(kslot, epi == EPI_FWD ? KT_GEMM_FWD : epi == EPI_DX ? KT_GEMM_DX : KT_GEMM_DW,
            dw_flops(g), st);                      // (no ones column: 2 M N K)
  // (named by epilogue: the operand orientation, and so gemm_kernel's AK / BK
  // arguments, is fixed per epilogue for the three C-ABI layer calls)
  int rc = check_launch(dw128 ? "gemm_dw128_kernel" : epi == EPI_FWD ? "gemm_kernel<fwd>"
                        : epi == EPI_DX ? "gemm_kernel<dx>" : "gemm_kernel<dw>");
  if (rc || S == 1) return rc;
  // the reducer is the last launch of a split-K GEMM: its name carries the
  // kernel whose slabs it sums, so smi_last_launch still tells the form
  return splitk_reduce(g, S, epi, st,
                       dw128 ? "gemm_splitk_reduce_kernel<gemm_dw128_kernel>"
                       : epi == EPI_FWD ? "gemm_splitk_reduce_kernel<gemm_kernel<fwd>>"
                       : epi == EPI_DX ? "gemm_splitk_reduce_kernel<gemm_kernel<dx>>"
                                       : "gemm_splitk_reduce_kernel<gemm_kernel<dw>>");
}

int splitk_reduce(const GemmArgs& g, int S, int epi, hipStream_t st, const char* what) {
  const int rslot = ktime_begin(st);
  const int64_t MN = (int64_t)g.M * g.N;
  const int rg = (int)((MN + 63) / 64);
  const bool fwd = epi == EPI_FWD;
  hipLaunchKernelGGL(gemm_splitk_reduce_kernel, dim3(rg), dim3(kWG), 0, st, g.part, S, g,
                     fwd ? g.bias : nullptr, fwd ? g.act : ACT_NONE,
                     epi == EPI_DX ? g.mask : nullptr);
  ktime_end(rslot, KT_GEMM_REDUCE, (double)S * MN, st);
  return check_launch(what);
}

// out[i] = sum_{z < S} part[z][i] in a fixed order (no accumulate)
int launch_slab_reduce(const float* part, int S, int64_t n, float* out, hipStream_t st,
                       const int* skip) {
  if (n < 1 || S < 1) return SMI_OK;
  const int rg = (int)((n + 63) / 64);
  GemmArgs g{};
  g.M = 1; g.N = (int)n; g.C = out; g.ldc = n; g.ones_col = -1; g.skip = skip;
  hipLaunchKernelGGL(gemm_splitk_reduce_kernel, dim3(rg), dim3(kWG), 0, st, part, S, g, nullptr,
                     ACT_NONE, nullptr);
  return check_launch("gemm_splitk_reduce_kernel");
}

int launch_linear_fwd(const float* X, int64_t ldx, int M, int K, const float* W, int64_t ldw,
                      const float* b, int N, int act, float* Y, int64_t ldy, hipStream_t st,
                      const int* skip) {
  if (takes_smallk_fwd(M, N, K))
    return launch_smallk_fwd(X, ldx, M, K, W, ldw, b, N, act, Y, ldy, st, skip);
  GemmArgs g{};
  g.M = M; g.N = N; g.K = K;
  g.A = X; g.a_rs = ldx; g.a_cs = 1;
  g.B = W; g.b_rs = 1; g.b_cs = ldw;        // B(k,n) = W[n][k]
  g.C = Y; g.ldc = ldy; g.bias = b; g.act = act; g.ones_col = -1; g.skip = skip;
  return gemm_launch(EPI_FWD, g, st);
}

// launch_linear_fwd plus Y[:, N : N + xcols] = S[:, :xcols] (one launch on the
// short-batch kernel, else the forward and a column copy)
int launch_linear_fwd_cat(const float* X, int64_t ldx, int M, int K, const float* W, int64_t ldw,
                          const float* b, int N, int act, float* Y, int64_t ldy, const float* S,
                          int64_t lds, int xcols, hipStream_t st) {
  const bool t16 = !takes_smallk_fwd(M, N, K) && takes_t16(M, N, K) && M > 0;
  if (!t16) {
    RC_CHECK(launch_linear_fwd(X, ldx, M, K, W, ldw, b, N, act, Y, ldy, st));
    return launch_copy_cols(S, lds, M, xcols, Y + N, ldy, st);
  }
  GemmArgs g{};
  g.M = M; g.N = N; g.K = K;
  g.A = X; g.a_rs = ldx; g.a_cs = 1;
  g.B = W; g.b_rs = 1; g.b_cs = ldw;
  g.C = Y; g.ldc = ldy; g.bias = b; g.act = act; g.ones_col = -1;
  g.xsrc = S; g.xlds = lds; g.xcols = xcols;
  return gemm_launch(EPI_FWD, g, st);
}

int launch_linear_bwd_dx(const float* dY, int64_t ldg, int M, int N, const float* W, int64_t ldw,
                         int K, const float* mask, int64_t ldm, float* dX, int64_t lddx,
                         hipStream_t st, const int* skip) {
  GemmArgs g{};
  g.M = M; g.N = K; g.K = N;
  g.A = dY; g.a_rs = ldg; g.a_cs = 1;
  g.B = W; g.b_rs = ldw; g.b_cs = 1;        // B(k=n', n=k') = W[n'][k']
  g.C = dX; g.ldc = lddx; g.mask = mask; g.ldm = ldm; g.ones_col = -1; g.skip = skip;
  return gemm_launch(EPI_DX, g, st);
}

}  // namespace smi
