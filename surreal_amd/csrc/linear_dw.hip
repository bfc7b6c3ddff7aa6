// linear_dw.hip — the dense layers' weight gradients (linear_kernels.hip's
// header has the arithmetic): the row-major forms (gemm_dwd_kernel, the grouped
// launch and its reducer, the short-batch form, the launch shared with the
// LSTM's BPTT), gemm_dw128_kernel, and the queue that groups a backward phase's
// GEMMs.  Slab lengths: dw_plan.hpp; other layouts: gemm_kernel<dw>.
#include <cmath>
#include <algorithm>
#include <type_traits>
#define SMI_GEMM_UNIT gemm_dw
#include "gemm_args.hpp"
#include "lstm_cell.hpp"

namespace smi {

// Weight-gradient GEMM with 128x128 output tiles (dW[m][n] = sum_r dY[r][m]
// X[r][n], r = the B*E rows).  The 64x64 kernel re-reads dY once per 64
// output columns and X once per 64 output rows (5x / 4x for the 300x200
// head): at these shapes the launch moves ~5x its unique bytes through L2 and
// is bound by that, not by the MFMAs.  128x128 halves both re-read factors
// and raises MFMAs per LDS operand read (16 MFMAs per 10 reads).  Both
// operands are row-contiguous slabs of 32 rows: float4 loads straight into
// [k][col] LDS images (row pitch 144: a half-wave's 32 lanes hit 32 banks),
// one K-step of register prefetch, one barrier per K-step.  Wave w owns
// output rows [32w, 32w+32) x 128 columns (16 accumulators).  The reduction
// is one MFMA chain per K-slab (split-K keeps slabs <= 512 rows); slab
// partials go to the fixed-order reducer as in gemm_kernel.
constexpr int D2_LD = 144;     // (D2_T: gemm_args.hpp)

__device__ __forceinline__ void dw2_load(const float* __restrict__ P, int64_t rs, int c0,
                                         int cdata, int ones_col, int k0, int kmax, float4 (&r)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = threadIdx.x + j * kWG;            // 32 rows x 32 float4
    const int k = q >> 5, c = c0 + ((q & 31) << 2);
    const int kk = k0 + k;
    const int kc = kk < kmax ? kk : kmax - 1;
    const int cc = c + 3 < cdata ? c : (cdata >= 4 ? cdata - 4 : 0);
    float4 v = *reinterpret_cast<const float4*>(P + (int64_t)kc * rs + cc);
    const bool okk = kk < kmax;
    v.x = okk && c < cdata ? v.x : 0.f;
    v.y = okk && c + 1 < cdata ? v.y : 0.f;
    v.z = okk && c + 2 < cdata ? v.z : 0.f;
    v.w = okk && c + 3 < cdata ? v.w : 0.f;
    if (ones_col >= 0 && okk) {
      if (c == ones_col) v.x = 1.f;
      if (c + 1 == ones_col) v.y = 1.f;
      if (c + 2 == ones_col) v.z = 1.f;
      if (c + 3 == ones_col) v.w = 1.f;
    }
    r[j] = v;
  }
}

__device__ __forceinline__ void dw2_store(float* __restrict__ S, const float4 (&r)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = threadIdx.x + j * kWG;
    *reinterpret_cast<float4*>(S + (q >> 5) * D2_LD + ((q & 31) << 2)) = r[j];
  }
}

__global__ void __launch_bounds__(kWG)
gemm_dw128_kernel(GemmArgs g) {
  if (g.skip && g.skip[0] != 0) return;
  __shared__ __attribute__((aligned(16))) float sA[2][32 * D2_LD];
  __shared__ __attribute__((aligned(16))) float sB[2][32 * D2_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const TileIdx ti = gemm_tile_index();
  const int m0 = ti.mt * D2_T, n0 = ti.nt * D2_T;
  const int kb = ti.z * g.kchunk;
  const int ke = min(g.K, kb + g.kchunk);
  const int nk = (ke - kb + 31) / 32;
  const int bdata = g.ones_col >= 0 ? g.ones_col + 1 : g.N;   // the ones column is synthesised
  const int bload = g.ones_col >= 0 ? g.ones_col : g.N;       // real columns of X
  f32x4 acc[2][8];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  float4 ra[4], rb[4];
  (void)bdata;
  if (nk > 0) {
    dw2_load(g.A, g.a_cs, m0, g.M, -1, kb, ke, ra);
    dw2_load(g.B, g.b_rs, n0, bload, g.ones_col, kb, ke, rb);
    dw2_store(sA[0], ra);
    dw2_store(sB[0], rb);
  }
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) {
      dw2_load(g.A, g.a_cs, m0, g.M, -1, kb + (kt + 1) * 32, ke, ra);
      dw2_load(g.B, g.b_rs, n0, bload, g.ones_col, kb + (kt + 1) * 32, ke, rb);
    }
    const float* As = sA[cur];
    const float* Bs = sB[cur];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int kr = (4 * u + lk) * D2_LD;
      float av[2], bv[8];
#pragma unroll
      for (int a = 0; a < 2; ++a) av[a] = As[kr + wave * 32 + a * 16 + li];
#pragma unroll
      for (int b = 0; b < 8; ++b) bv[b] = Bs[kr + b * 16 + li];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = mfma4(av[a], bv[b], acc[a][b]);
    }
    if (kt + 1 < nk) {
      dw2_store(sA[cur ^ 1], ra);
      dw2_store(sB[cur ^ 1], rb);
    }
    __syncthreads();
  }
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const int n = n0 + b * 16 + li;
    if (n >= g.N) continue;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m0 + wave * 32 + a * 16 + lk * 4 + i;
        if (m >= g.M) continue;
        const float v = acc[a][b][i];
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

void dw128_dispatch(const GemmArgs& g, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL(gemm_dw128_kernel, grid, dim3(kWG), 0, st, g);
}

// Weight gradient with operands straight from global memory into MFMA
// registers (no LDS staging, no barriers in the main loop).  dW[m][n] =
// sum_r dY[r][m] * X[r][n] reduces over the rows, which is the MFMA k index;
// a 16x16x4 MFMA's A operand for lane (li, lk) is (row lk, column li) and its
// B operand (row lk, column li), so one wave loads a 4-row step of BOTH
// operands as row-contiguous vectors: lane li takes MT consecutive dY columns
// m0 + MT*li + t (one per MFMA m-tile t) and 4 consecutive X columns per
// 64-column half, i.e. 16-byte loads that feed MT x NT MFMAs.  The output
// columns are thereby interleaved across tiles; the epilogue undoes that.  The
// four waves of a workgroup take interleaved 4-row steps of one row slab (P
// steps prefetched in registers) and are combined through LDS in a fixed
// order; slabs go to the split-K partials.  Row-major dY/X of the heads, the
// LSTM input/recurrent weights and the DDPG nets all take this path.
constexpr int DWD_OCC = 2;         // workgroups per CU gemm_dwd_kernel is built for

// Rows past the slab and the synthesised bias column are selected by ADDRESS
// (a zero row / a {1, 0, 0, 0} vector in device memory), never by masking the
// loaded value: the loads then feed the MFMAs untouched and the compiler keeps
// all P steps in flight.  Columns past M / N read clamped addresses; they only
// reach outputs the epilogue drops.

// Fitted edge tiles (MT or NT of 1..3 sub-tiles: the M / N remainder of a
// grouped GEMM, dw_plan): lane li reads its MT (NT) consecutive columns with
// ONE load, a dword / dwordx2 / dwordx3 through a 4-byte-aligned vector type,
// and sub-tile j takes component j -- an MFMA does not care which output
// column sits in which tile position.  The run is clamped to end at the
// operand's last column (lanes past the end repeat earlier columns), so the
// epilogue derives each position's column from the same clamp (dwd_fit_col)
// and drops the repeats.  The bias column of a fitted N edge is the first
// component of the first lane past the data, read from g_dwd_one.
typedef float dwd_v2 __attribute__((ext_vector_type(2), aligned(4)));
typedef float dwd_v3 __attribute__((ext_vector_type(3), aligned(4)));
// W consecutive floats at p (4-byte aligned for W < 4, 16-byte for W == 4) with
// one load; GLOBAL: through an address-space-1 pointer (dwd_main_fast)
template <int W, bool GLOBAL>
__device__ __forceinline__ float4 dwd_ldw(const float* p) {
#define SMI_LDW(T_) (GLOBAL ? *(const __attribute__((address_space(1))) T_*)p : *(const T_*)p)
  if constexpr (W == 4) { const f32x4 x = SMI_LDW(f32x4); return float4{x[0], x[1], x[2], x[3]}; }
  else if constexpr (W == 3) { const dwd_v3 x = SMI_LDW(dwd_v3); return float4{x[0], x[1], x[2], 0.f}; }
  else if constexpr (W == 2) { const dwd_v2 x = SMI_LDW(dwd_v2); return float4{x[0], x[1], 0.f, 0.f}; }
  else return float4{SMI_LDW(float), 0.f, 0.f, 0.f};
#undef SMI_LDW
}

// the column that position (lane li, component j) of a W-wide fitted edge
// starting at column c0 holds, data columns [.., lim); -1: none (a repeat)
template <int W>
__device__ __forceinline__ int dwd_fit_col(int c0, int lim, int li, int j) {
  const int cb = c0 + W * li;
  const int c = min(cb, lim - W) + j;
  return c >= cb ? c : -1;
}

template <int MT, int NT, bool VA, bool VB, int NB = NT>
__device__ __forceinline__ void dwd_load(const GemmArgs& g, int r, int ke, int m0, int n0, int bdata,
                                         float (&av)[MT], float (&bv)[NT]) {
  const int li = threadIdx.x & 15;
  const bool ok = r < ke;
  const float* Ar = ok ? g.A + (int64_t)r * g.a_cs : g_dwd_zero;
  const float* Br = ok ? g.B + (int64_t)r * g.b_rs : g_dwd_zero;
  // second source (columns >= split_col): its row base, shifted so that column
  // cb reads Br2 + cb (rows past the slab read the zero row at offset cb - split)
  const float* Br2 = g.B2 ? (ok ? g.B2 + (int64_t)r * g.b2_rs - g.split_col
                                : g_dwd_zero - g.split_col)
                          : Br;
  const int split = g.B2 ? g.split_col : 0x7fffffff;
  const float* one = ok ? g_dwd_one : g_dwd_zero;
  if constexpr (MT == 4 && VA) {
    const int c = min(m0 + 4 * li, g.M - 4);
    const float4 x = *reinterpret_cast<const float4*>(Ar + c);
    av[0] = x.x; av[1] = x.y; av[2] = x.z; av[3] = x.w;
  } else if constexpr (MT == 2 || MT == 3) {
    const float4 x = dwd_ldw<MT, false>(Ar + min(m0 + MT * li, g.M - MT));
    av[0] = x.x; av[1] = x.y;
    if constexpr (MT == 3) av[2] = x.z;
  } else {
#pragma unroll
    for (int t = 0; t < MT; ++t) av[t] = Ar[min(m0 + MT * li + t, g.M - 1)];
  }
  if constexpr (NT < 4) {
    const int cb = n0 + NT * li;
    const int c = min(cb, bdata - NT);
    const float* src = cb < bdata ? (c >= split ? Br2 : Br) + c
                                  : (g.ones_col >= 0 && cb < bdata + NT ? one : g_dwd_zero);
    const float4 x = dwd_ldw<NT, false>(src);
    bv[0] = x.x;
    if constexpr (NT >= 2) bv[1] = x.y;
    if constexpr (NT == 3) bv[2] = x.z;
    return;
  }
#pragma unroll
  for (int h = 0; h < NB / 4; ++h) {
    const int cb = n0 + 64 * h + 4 * li;
    if constexpr (VB) {
      const float* src = cb < bdata ? (cb >= split ? Br2 : Br) + cb
                                    : (cb == g.ones_col ? one : g_dwd_zero);
      const float4 x = *reinterpret_cast<const float4*>(src);
      bv[4 * h] = x.x; bv[4 * h + 1] = x.y; bv[4 * h + 2] = x.z; bv[4 * h + 3] = x.w;
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int c = cb + t;
        bv[4 * h + t] = *(c < bdata ? (c >= split ? Br2 : Br) + c
                                    : (c == g.ones_col ? one : g_dwd_zero));
      }
    }
  }
}

// Unchecked streaming loop over a slab whose rows are all valid (every slab
// but possibly the last: slab lengths are multiples of the prefetch window)
// with 16-byte operands: the lane's operand addresses are formed once and
// advanced by RS rows per step, so a step is its loads and MFMAs only — no
// per-step 64-bit row products, clamps, zero-row selects or exec-masked
// branches (the checked loop spends ~40 VALU/SALU ops per step on them).
// The last DWD_P steps are peeled without loads (no reads past the slab).
// Same MFMA chains in the same order as the checked loop: bit-identical.
template <int MT, int NT, int NB, int RS>
__device__ __forceinline__ void dwd_main_fast(const GemmArgs& g, int rw, int nsteps, int m0, int n0,
                                              int bdata, f32x4 (&acc)[MT][NT]) {
  static_assert(NB == NT || (NT == 8 && NB == 4), "fast dW loop: whole tiles or the lower half of 8");
  constexpr int GW = NT < 4 ? NT : 4;             // columns per B load (NT < 4: the fitted edge's one run)
  constexpr int NH = NB / GW;
  const int li = threadIdx.x & 15;
  const float* pa = g.A + (int64_t)rw * g.a_cs + min(m0 + MT * li, g.M - MT);
  const int64_t sa = (int64_t)RS * g.a_cs;
  const float* pb[NH];
  int64_t sb[NH];
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    const int cb = n0 + 64 * h + GW * li;
    if (cb < bdata) {
      const int c = NT < 4 ? min(cb, bdata - NT) : cb;   // (a fitted run ends with the data)
      if (g.B2 && c >= g.split_col) {
        pb[h] = g.B2 + (int64_t)rw * g.b2_rs + (c - g.split_col);
        sb[h] = (int64_t)RS * g.b2_rs;
      } else {
        pb[h] = g.B + (int64_t)rw * g.b_rs + c;
        sb[h] = (int64_t)RS * g.b_rs;
      }
    } else {
      const bool ones = NT < 4 ? g.ones_col >= 0 && cb < bdata + NT : cb == g.ones_col;
      pb[h] = ones ? g_dwd_one : g_dwd_zero;
      sb[h] = 0;
    }
  }
  float4 av[DWD_P], bv[DWD_P][NH];
  // global (addrspace 1) loads spelled out: with the prologue pinned below the
  // compiler no longer infers the address space and emits flat loads, which
  // also count against lgkmcnt
  // (dwd_ldw: one load instruction per operand per step whatever the width)
  auto load = [&](int p) {
    av[p] = dwd_ldw<MT, true>(pa);
    pa += sa;
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      bv[p][h] = dwd_ldw<GW, true>(pb[h]);
      pb[h] += sb[h];
    }
  };
  auto step = [&](int p) {
    const float a4[4] = {av[p].x, av[p].y, av[p].z, av[p].w};
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const float4 q = bv[p][b >> 2];
      const float bb = (b & 3) == 0 ? q.x : (b & 3) == 1 ? q.y : (b & 3) == 2 ? q.z : q.w;
#pragma unroll
      for (int a = 0; a < MT; ++a) acc[a][b] = mfma4(a4[a], bb, acc[a][b]);
    }
  };
  // the prologue's loads are pinned in step order too: the loop header's
  // vmcnt is the merge of the preheader and the back edge, so one prologue
  // load issued out of order (the scheduler put b0 seventh of eight) made
  // every iteration wait at vmcnt(1), i.e. on the loads just issued
#pragma unroll
  for (int p = 0; p < DWD_P; ++p) {
    load(p);
    __builtin_amdgcn_sched_barrier(0);
  }
  // sched_barrier pins each refill right behind the MFMAs of the step it
  // replaces: without it the scheduler sinks all DWD_P refills to the end of
  // the unrolled body and the next iteration waits on them (vmcnt(9..0)), i.e.
  // no prefetch distance at all
  // 16-wide tail tiles (MT == 1, whatever their width) run the longest slabs
  // of a balanced grouped launch (~2.5x the rows of a full tile's slab): their
  // MFMA chain restarts every DWD_P steps and the blocks are summed in a second
  // register set, so a wave's fp32 chain is DWD_P + steps / DWD_P long instead
  // of steps long (the value head's 1-row gradient sums 21504 rows with heavy
  // cancellation).  The other fitted classes share their band's slabs with
  // the full tiles and keep the full tiles' single chain.
  constexpr bool kRestart = MT == 1;
  f32x4 tot[MT][NT];
  if constexpr (kRestart) {
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
      for (int b = 0; b < NT; ++b) tot[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int s0 = DWD_P; s0 < nsteps; s0 += DWD_P) {
#pragma unroll
    for (int p = 0; p < DWD_P; ++p) {
      step(p);
      load(p);
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (kRestart) {
#pragma unroll
      for (int a = 0; a < MT; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          tot[a][b] += acc[a][b];
          acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
  }
#pragma unroll
  for (int p = 0; p < DWD_P; ++p) step(p);
  if constexpr (kRestart) {
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
      for (int b = 0; b < NB; ++b) acc[a][b] = tot[a][b] + acc[a][b];
  }
}

// WV waves per workgroup (4: one per SIMD; 8: two per SIMD, each wave takes
// every WV-th 4-row step of the slab, so a SIMD interleaves two waves' loads
// and MFMAs; the waves' sums meet in LDS in a fixed tree order)
template <int MT, int NT, bool VA, bool VB, int WV>
__device__ __forceinline__ void dwd_tile(const GemmArgs& g, const DwEnt& e, const TileIdx ti,
                                         float4* dwd_red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  // (rows and columns of the GEMM, not of the rectangle: dw_put and the
  // operand loads take them as they are)
  const int m0 = e.m0 + ti.mt * 16 * MT, n0 = e.n0 + ti.nt * 16 * NT;
  const int mend = e.m0 + e.M, nend = e.n0 + e.N;
  const int kb = ti.z * e.kchunk;
  const int ke = min(g.K, kb + e.kchunk);
  constexpr int RS = 4 * WV;                      // rows per step of the workgroup
  const int nsteps = (ke - kb + RS - 1) / RS;
  const int bdata = g.ones_col >= 0 ? g.ones_col : g.N;
  const int rw = kb + 4 * wave + lk;              // this lane's row in step 0
  f32x4 acc[MT][NT];
#pragma unroll
  for (int a = 0; a < MT; ++a)
#pragma unroll
    for (int b = 0; b < NT; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
  // loads are unconditional (rows past the slab read clamped and zeroed) so
  // the compiler's vmcnt waits stay partial across the unrolled P steps;
  // slabs are multiples of 4*WV*P rows, only the last one runs zero steps
  // NB of the NT column sub-tiles carry data: a tile whose upper 64-column
  // half lies past N (e.g. columns 320..383 of a 301-wide gradient) runs the
  // half-width loop (wave-uniform choice, no loads or MFMAs for that half)
  auto mainloop = [&](auto nbc) {
    constexpr int NB = decltype(nbc)::value;
    float av[DWD_P][MT], bv[DWD_P][NT];
#pragma unroll
    for (int p = 0; p < DWD_P; ++p)
      dwd_load<MT, NT, VA, VB, NB>(g, rw + RS * p, ke, m0, n0, bdata, av[p], bv[p]);
    for (int s0 = 0; s0 < nsteps; s0 += DWD_P) {
#pragma unroll
      for (int p = 0; p < DWD_P; ++p) {
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
          for (int a = 0; a < MT; ++a) acc[a][b] = mfma4(av[p][a], bv[p][b], acc[a][b]);
        dwd_load<MT, NT, VA, VB, NB>(g, rw + RS * (s0 + p + DWD_P), ke, m0, n0, bdata, av[p], bv[p]);
        __builtin_amdgcn_sched_barrier(0);     // keep the refill here (see dwd_main_fast)
      }
    }
  };
  // full slabs whose operands each load with one instruction take the
  // unchecked streaming loop (4-wide operands: 16-byte loads, VA / VB; fitted
  // widths 1..3: always)
  constexpr bool kFast = (VB || NT < 4) && (VA || MT < 4);
  bool fast = false;
  if constexpr (kFast)
    fast = nsteps >= DWD_P && nsteps % DWD_P == 0 && kb + nsteps * RS <= ke;
  constexpr int NBH = NT > 4 ? 4 : NT;
  if (NT == 8 && n0 + 64 >= nend) {
    if constexpr (kFast) {
      if (fast) dwd_main_fast<MT, NT, NBH, RS>(g, rw, nsteps, m0, n0, bdata, acc);
      else mainloop(std::integral_constant<int, NBH>{});
    } else {
      mainloop(std::integral_constant<int, NBH>{});
    }
  } else {
    if constexpr (kFast) {
      if (fast) dwd_main_fast<MT, NT, NT, RS>(g, rw, nsteps, m0, n0, bdata, acc);
      else mainloop(std::integral_constant<int, NT>{});
    } else {
      mainloop(std::integral_constant<int, NT>{});
    }
  }
  // combine the waves in a fixed tree: at stride h, waves [h, 2h) add into
  // waves [0, h), two at a time through the two LDS buffers (WV = 4 gives
  // (w0 + w2) + (w1 + w3))
  auto put = [&](float4* buf) {
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
      for (int b = 0; b < NT; ++b) {
        const f32x4 v = acc[a][b];
        buf[(a * NT + b) * 64 + lane] = float4{v[0], v[1], v[2], v[3]};
      }
  };
  auto add = [&](const float4* buf) {
#pragma unroll
    for (int a = 0; a < MT; ++a)
#pragma unroll
      for (int b = 0; b < NT; ++b) {
        const float4 v = buf[(a * NT + b) * 64 + lane];
        acc[a][b] += f32x4{v.x, v.y, v.z, v.w};
      }
  };
#pragma unroll
  for (int h = WV / 2; h >= 1; h >>= 1) {
#pragma unroll
    for (int c = 0; c < h; c += 2) {
      if (wave >= h + c && wave < h + c + 2) put(dwd_red + (wave - h - c) * MT * NT * 64);
      __syncthreads();
      if (wave >= c && wave < c + 2 && wave < h) add(dwd_red + (wave - c) * MT * NT * 64);
      __syncthreads();
    }
  }
  if (wave != 0) return;
  // D(row lk*4+i, col li) of tile (a, b) is dW[m][n] with
  // m = m0 + MT*(lk*4+i) + a, n = n0 + 64*(b/4) + 4*li + b%4 (fitted edges:
  // the clamped runs of dwd_fit_col; a fitted N edge's bias column is
  // component 0 of the first lane past the data)
  auto out = [&](int m, int n, float v) {
    if (e.part) e.part[((int64_t)ti.z * e.M + (m - e.m0)) * e.N + (n - e.n0)] = v;
    else dw_put(g, m, n, v);
  };
  const bool vec_part = e.part && (e.N & 3) == 0;
#pragma unroll
  for (int a = 0; a < MT; ++a)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int m = m0 + MT * (lk * 4 + i) + a;
      if constexpr (MT == 2 || MT == 3) m = dwd_fit_col<MT>(m0, g.M, lk * 4 + i, a);
      if (m < 0 || m >= mend) continue;
      if constexpr (NT < 4) {
        const int cb = n0 + NT * li;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          int n = cb < bdata ? dwd_fit_col<NT>(n0, bdata, li, t)
                             : (t == 0 && g.ones_col >= 0 && cb < bdata + NT ? g.ones_col : -1);
          if (n < 0 || n >= nend) continue;
          out(m, n, acc[a][t][i]);
        }
        continue;
      }
#pragma unroll
      for (int h = 0; h < NT / 4; ++h) {
        const int nb = n0 + 64 * h + 4 * li;
        if (vec_part) {
          if (nb < nend)
            *reinterpret_cast<float4*>(e.part + ((int64_t)ti.z * e.M + (m - e.m0)) * e.N + (nb - e.n0)) =
                float4{acc[a][4 * h][i], acc[a][4 * h + 1][i], acc[a][4 * h + 2][i],
                       acc[a][4 * h + 3][i]};
          continue;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int n = nb + t;
          if (n >= nend) continue;
          out(m, n, acc[a][4 * h + t][i]);
        }
      }
    }
}

template <int MT, int NT, bool VA, bool VB>
__global__ void __launch_bounds__(256, DWD_OCC)
gemm_dwd_kernel(GemmArgs g) {
  if (g.skip && g.skip[0] != 0) return;
  extern __shared__ float4 dwd_red[];            // 2 x [MT*NT][64] float4
  DwEnt e{};                                     // the whole output as one rectangle
  e.part = g.part; e.M = g.M; e.N = g.N; e.kchunk = g.kchunk;
  dwd_tile<MT, NT, VA, VB, 4>(g, e, gemm_tile_index(), dwd_red);
}

// one workgroup of a grouped launch: orig = its index among the launch's nwg
// dW workgroups (the XCD-contiguous remap, xcd_contiguous, assumes orig and
// the hardware's blockIdx agree mod 8)
template <int WV>
__device__ __forceinline__ void dwd_group_run(const DwGroup& G, int orig, int nwg, float4* dwd_red) {
  const int w = xcd_contiguous(orig, nwg);
  int ei = 0;
  while (ei + 1 < G.n && w >= G.wg0[ei + 1]) ++ei;
  // (copies: the tile bodies below then read these, not G -- with every class
  // reading the kernel argument itself the compiler stops resolving its uses
  // to the argument segment and keeps a copy of all of G in scratch)
  const DwEnt e = G.e[ei];
  const GemmArgs g = G.g[e.gi];
  if (g.skip && g.skip[0] != 0) return;
  const int local = w - G.wg0[ei];
  TileIdx ti;
  ti.nt = local % e.gn;
  ti.mt = (local / e.gn) % e.gm;
  ti.z = local / (e.gn * e.gm);
  // the entry's tile class: MT x NT sub-tiles; VA / VB: 16-byte loads of a
  // 4-wide operand (fitted widths 1..3 always load with one instruction)
#define SMI_DWT(MT_, NT_, VA_, VB_) \
  case dw_cls(MT_, NT_, VA_, VB_): dwd_tile<MT_, NT_, VA_, VB_, WV>(g, e, ti, dwd_red); break;
#define SMI_DWT3(NT_, VB_) SMI_DWT(1, NT_, false, VB_) SMI_DWT(2, NT_, false, VB_) SMI_DWT(3, NT_, false, VB_)
  switch (e.cls) {
    SMI_DWT(4, DWG_NT, true, true) SMI_DWT(4, DWG_NT, true, false)
    SMI_DWT(4, DWG_NT, false, true) SMI_DWT(4, DWG_NT, false, false)
    SMI_DWT(1, DWG_NT, false, true) SMI_DWT(1, DWG_NT, false, false)
    default: break;
  }
  // (the fitted classes run on the 4-wave launch only: dw_fit_level)
  if constexpr (WV == 4) {
    switch (e.cls) {
      SMI_DWT(2, DWG_NT, false, true) SMI_DWT(3, DWG_NT, false, true)
      SMI_DWT(2, DWG_NT, false, false) SMI_DWT(3, DWG_NT, false, false)
      SMI_DWT(4, 1, true, false) SMI_DWT(4, 2, true, false) SMI_DWT(4, 3, true, false)
      SMI_DWT(4, 1, false, false) SMI_DWT(4, 2, false, false) SMI_DWT(4, 3, false, false)
      SMI_DWT3(1, false) SMI_DWT3(2, false) SMI_DWT3(3, false)
      default: break;
    }
  }
#undef SMI_DWT3
#undef SMI_DWT
}

__global__ void __launch_bounds__(256, DWG_OCC)
gemm_dwd_group_kernel(DwGroup G) {
  extern __shared__ float4 dwd_red[];
  dwd_group_run<4>(G, blockIdx.x, gridDim.x, dwd_red);
}

// BPTT of the one-segment-per-workgroup VALU form (workgroups < la.B) and
// the weight gradients already queued in the phase's group (the heads'; the
// others) in ONE launch: the heads' gradients need nothing from the BPTT, so
// they run on the CUs the recurrence leaves idle (la.B segments on one CU
// each) instead of after it
template <int BR>
__global__ void __launch_bounds__(kVT, 1)
lstm_bwd_dw_kernel(LstmBwdArgs la, DwGroup G) {
  extern __shared__ float4 dwd_red[];
  if ((int)blockIdx.x < la.B) {
    lstm_bwd_q_body<BR>(la, blockIdx.x);
    return;
  }
  dwd_group_run<8>(G, blockIdx.x - la.B, gridDim.x - la.B, dwd_red);
}

// the partials of every GEMM of a group, each element summed over its slabs in
// the fixed order of gemm_splitk_reduce_kernel.  With an epilogue task
// (G.x.on): every block also writes the fp64 sum of squares of the values it
// stored to x.sq[block] (fixed order: lane values, wave butterfly, waves in
// order), and one more block (block 0) runs the task itself: the log_var
// gradient from its row partials, that block's sum of squares, the partial
// count and the optimizer step bump (what sumsq_part_kernel and
// logvar_grad_kernel did as launches of their own)
__device__ void dw_epilogue_block(const DwEpilogue& x, int nsq) {
  __shared__ double red[kWG / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float q = 0.f;
  if (x.lvpart) {
    // d log_var[j] = std_j * sum_blocks lvpart[.][j] (logvar_grad_kernel's order);
    // a wave takes its columns j = wave + 4 i two at a time (both columns'
    // partials in flight together: 16 of the lane's partials per column per
    // trip, the same additions in the same order per column)
    constexpr int NW = kWG / 64;
    for (int j0 = wave; j0 < x.lv_A; j0 += 2 * NW) {
      const int jj[2] = {j0, min(j0 + NW, x.lv_A - 1)};      // (a clamped second column is dropped)
      float t[2] = {0.f, 0.f};
      int i = lane;
      for (; i + 15 * 64 < x.lv_nb; i += 16 * 64) {
        float v[2][16];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int k = 0; k < 16; ++k) v[c][k] = x.lvpart[(int64_t)(i + 64 * k) * x.lv_A + jj[c]];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int k = 0; k < 16; ++k) t[c] += v[c][k];
      }
      {
        // the tail's loads unconditional (past the end: a zero by address) and
        // pinned before the conditional adds: a load whose only use sat under
        // its lane condition was sunk into that branch, one round trip each
        float v[2][16];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int k = 0; k < 16; ++k) {
            const int ik = i + 64 * k;
            v[c][k] = *(ik < x.lv_nb ? x.lvpart + (int64_t)ik * x.lv_A + jj[c] : g_dwd_zero);
          }
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int k = 0; k < 16; ++k) asm volatile("" : "+v"(v[c][k]));
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int k = 0; k < 16; ++k)
            if (i + 64 * k < x.lv_nb) t[c] += v[c][k];
      }
      const float e0 = expf(x.lv[jj[0]]), e1 = expf(x.lv[jj[1]]);
      const float g0 = wave_sum(t[0]) * e0;
      const float g1 = wave_sum(t[1]) * e1;
      if (lane == 0) {
        x.lv_out[jj[0]] = g0;
        q += g0 * g0;
        if (j0 + NW < x.lv_A) {
          x.lv_out[jj[1]] = g1;
          q += g1 * g1;
        }
      }
    }
  }
  if (!x.sq) {
    if (threadIdx.x == 0 && x.step) x.step[0] += 1;
    if (threadIdx.x == 0 && x.runs) x.runs[0] += 1;
    return;
  }
  const double t = block_sum_d((double)q, red);
  if (threadIdx.x == 0) {
    x.sq[nsq] = t;
    x.np[0] = nsq + 1;
    if (x.step) x.step[0] += 1;
    if (x.runs) x.runs[0] += 1;
  }
}

// one element's sum over its S slabs as lane zl of the reducer sees it: slabs
// z = zl, zl + 4, ... into four accumulators (z, z + 4, z + 8, z + 12 of each
// 16-slab trip), the rest into the first; p = the element's slab-0 address.
// For S <= 64 every slab is loaded before the first add (one memory round trip):
// the loads are unconditional (slabs past S read a zero by address) and pinned
// before the conditional adds -- with `zk < S ? load : 0` the compiler sank
// each load into its own branch and waited on it there, and 64-bit index
// products per load made it reuse address registers between loads (round 6)
template <int U>
__device__ __forceinline__ void red_slabs(const float* const (&p)[U], int64_t MN, int S, int zl,
                                          float (&r)[U]) {
  float s0[U], s1[U], s2[U], s3[U];
#pragma unroll
  for (int u = 0; u < U; ++u) s0[u] = s1[u] = s2[u] = s3[u] = 0.f;
  int z = zl;
  if (S <= 64) {
    const int64_t st4 = 4 * MN;
    float v[U][16];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float* pz = p[u] + (int64_t)zl * MN;
#pragma unroll
      for (int k = 0; k < 16; ++k) v[u][k] = *(zl + 4 * k < S ? pz + k * st4 : g_dwd_zero);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int k = 0; k < 16; ++k) asm volatile("" : "+v"(v[u][k]));
    const int nfull = S > zl + 12 ? (S - zl - 12 + 15) / 16 : 0;   // z + 12 < S trips
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < nfull) {
          s0[u] += v[u][4 * j]; s1[u] += v[u][4 * j + 1]; s2[u] += v[u][4 * j + 2]; s3[u] += v[u][4 * j + 3];
        }
      }
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k >= 4 * nfull && zl + 4 * k < S) s0[u] += v[u][k];
    }
    z = S;
  }
  for (; z + 12 < S; z += 16) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      s0[u] += p[u][(int64_t)z * MN];
      s1[u] += p[u][(int64_t)(z + 4) * MN];
      s2[u] += p[u][(int64_t)(z + 8) * MN];
      s3[u] += p[u][(int64_t)(z + 12) * MN];
    }
  }
  for (; z < S; z += 4)
#pragma unroll
    for (int u = 0; u < U; ++u) s0[u] += p[u][(int64_t)z * MN];
#pragma unroll
  for (int u = 0; u < U; ++u) r[u] = (s0[u] + s1[u]) + (s2[u] + s3[u]);
}

// U: 64-element groups per block (block = 64 U consecutive elements; lane el
// of wave zl sums slabs zl, zl + 4, ... of elements el + 64 u).  Every element
// gets the additions of gemm_splitk_reduce_kernel in the same order whatever
// U is; U = 4 dispatches a quarter of the workgroups with 4x the loads in
// flight per thread (kRedU, host side; U = 1: the epilogue task alone)
template <int U>
__global__ void __launch_bounds__(kWG)
gemm_group_reduce_kernel(DwGroup G) {
  __shared__ float red[4][64 * U];
  __shared__ double sqr[kWG / 64];
  // the epilogue task (when on) is block 0: dispatched first, its chain of
  // dependent steps overlaps the reduction blocks instead of trailing them
  const int ep = G.x.on ? 1 : 0;
  if (ep && blockIdx.x == 0) {
    if (G.x.skip && G.x.skip[0] != 0) return;
    dw_epilogue_block(G.x, G.rb0[G.n]);
    return;
  }
  const int b = (int)blockIdx.x - ep;
  int ei = 0;
  while (ei + 1 < G.n && b >= G.rb0[ei + 1]) ++ei;
  const DwEnt& en = G.e[ei];
  const GemmArgs& g = G.g[en.gi];
  if (g.skip && g.skip[0] != 0) return;
  const int S = en.S;
  const int64_t MN = (int64_t)en.M * en.N;
  const int el = threadIdx.x & 63, zl = threadIdx.x >> 6;
  const int64_t eb = (int64_t)(b - G.rb0[ei]) * 64 * U;
  const float* p[U];
#pragma unroll
  for (int u = 0; u < U; ++u) p[u] = en.part + min(eb + el + 64 * u, MN - 1);
  float r[U];
  red_slabs<U>(p, MN, S, zl, r);
#pragma unroll
  for (int u = 0; u < U; ++u) red[zl][el + 64 * u] = r[u];
  __syncthreads();
  float q = 0.f;
  for (int i = threadIdx.x; i < 64 * U; i += kWG) {
    const int64_t e = eb + i;
    if (e < MN) {
      const float v = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
      const int m = (int)(e / en.N), n = (int)(e - (int64_t)m * en.N);
      q += dw_put(g, en.m0 + m, en.n0 + n, v);
    }
  }
  if (!G.x.sq) return;
  const double t = block_sum_d((double)q, sqr);
  if (threadIdx.x == 0) G.x.sq[b] = t;
}

// waves per dW workgroup, one per SIMD (measured: 8 waves, two per SIMD, 5-10 %
// slower per launch and 6 % slower end to end at C3; the weight gradients that
// share the BPTT's launch run in its 8-wave workgroups)
constexpr int kDwdWaves = 4;

template <int MT, int NT>
static void dwd_dispatch(const GemmArgs& g, dim3 grid, bool va, bool vb, hipStream_t st) {
  const size_t lds = (size_t)2 * MT * NT * 64 * sizeof(float4);
  const dim3 blk(64 * kDwdWaves);
  if (va && vb) hipLaunchKernelGGL((gemm_dwd_kernel<MT, NT, true, true>), grid, blk, lds, st, g);
  else if (va) hipLaunchKernelGGL((gemm_dwd_kernel<MT, NT, true, false>), grid, blk, lds, st, g);
  else if (vb) hipLaunchKernelGGL((gemm_dwd_kernel<MT, NT, false, true>), grid, blk, lds, st, g);
  else hipLaunchKernelGGL((gemm_dwd_kernel<MT, NT, false, false>), grid, blk, lds, st, g);
}

// 16-byte facts of a row-major weight gradient: a / b: the dY / X (both sources)
// bases are aligned; va / vb: extents and row strides also let a 4-wide dY / X
// operand load as 16-byte vectors (each caller adds its own condition on M)
struct DwAlign { bool a, b, va, vb; };
static DwAlign dw_align(const GemmArgs& g) {
  auto al16 = [](const float* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const int bdata = g.ones_col >= 0 ? g.ones_col : g.N;
  DwAlign r;
  r.a = al16(g.A);
  r.b = al16(g.B) && (!g.B2 || al16(g.B2));
  r.va = r.a && g.M % 4 == 0 && g.a_cs % 4 == 0;
  r.vb = r.b && bdata >= 4 && bdata % 4 == 0 && g.b_rs % 4 == 0 &&
         (!g.B2 || (g.b2_rs % 4 == 0 && g.split_col % 4 == 0));
  return r;
}

// weight gradient over row-major dY / X (a_rs == 1, b_cs == 1): gemm_dwd_kernel
static int dwd_launch(GemmArgs g, hipStream_t st) {
  const int MT = g.M > 32 ? 4 : 1, NT = g.N > 64 ? 8 : 4;
  const DwAlign al = dw_align(g);
  const bool va = MT == 4 && al.va, vb = al.vb;
  const int gm = (g.M + 16 * MT - 1) / (16 * MT), gn = (g.N + 16 * NT - 1) / (16 * NT);
  const int tiles = gm * gn;
  constexpr int kDwdTarget = 256;   // measured: ~1 workgroup per CU beats deeper splits (partials)
  int S = (kDwdTarget + tiles - 1) / tiles;
  const int smax = (g.K + 32 * kDwdWaves - 1) / (32 * kDwdWaves);   // >= 8 steps per wave
  if (S > smax) S = smax;
  const int64_t cap = smi_workspace_floats() / ((int64_t)g.M * g.N);
  if (S > cap) S = (int)cap;
  if (S < 1) S = 1;
  g.part = nullptr;
  g.kchunk = g.K;
  if (S > 1) {
    const int rs = 4 * kDwdWaves * DWD_P;          // rows per prefetch window
    g.kchunk = ((g.K + S - 1) / S + rs - 1) / rs * rs;
    S = (g.K + g.kchunk - 1) / g.kchunk;
  }
  if (S > 1) {
    g.part = workspace_f32((int64_t)S * g.M * g.N);
    if (!g.part) return set_error(SMI_E_ARG, "gemm: workspace unavailable for split-K");
  }
  const dim3 grid(gm, gn, S);
  const int kslot = ktime_begin(st);
  if (MT == 4 && NT == 8) dwd_dispatch<4, 8>(g, grid, va, vb, st);
  else if (MT == 4) dwd_dispatch<4, 4>(g, grid, va, vb, st);
  else if (NT == 8) dwd_dispatch<1, 8>(g, grid, false, vb, st);
  else dwd_dispatch<1, 4>(g, grid, false, vb, st);
  ktime_end(kslot, KT_GEMM_DW, dw_flops(g), st);
  const int rc = check_launch("gemm_dwd_kernel");
  if (rc || S == 1) return rc;
  return splitk_reduce(g, S, EPI_DW, st, "gemm_splitk_reduce_kernel<gemm_dwd_kernel>");
}

// ---- grouped weight gradients (gemm_dwd_group_kernel) ----------------------
// the queue of the calling thread (begin ... flush bracket one call sequence)
struct DwQueue {
  DwGroup grp;
  bool on = false;
  double flops = 0.0;
  // set when a weight gradient issued inside an open bracket did not join the
  // group (group full, or a shape / layout the grouped kernel does not take):
  // with a fused sum of squares (x.sq) its gradient would be missing from the
  // clip_grad_norm_ partials, so the flush fails instead of clipping wrongly
  bool missed = false;
  // entries already launched with the BPTT (launch_lstm_bwd_dw) whose partials
  // the group's reducer still sums, and the workspace floats they hold
  // (reserved: workspace_reserve)
  DwGroup pre;
  bool pre_on = false;
  int64_t pre_need = 0;
};
static thread_local DwQueue g_dwq;

// opens a bracket with nothing left of an earlier one (a bracket abandoned
// without its flush: no stale pre partials, no workspace still reserved)
int dw_group_begin() {
  DwQueue& q = g_dwq;
  q.on = true;
  q.missed = false;
  q.grp.ng = q.grp.n = 0;
  q.grp.x = DwEpilogue{};
  q.flops = 0.0;
  q.pre_on = false;
  q.pre.ng = q.pre.n = 0;
  q.pre_need = 0;
  workspace_reserve(0);
  return SMI_OK;
}

// the reducer's epilogue task of the open group (dw_group_flush launches one
// more reducer block for it); with x.sq every weight gradient of the bracket
// must join the group (the fused sum of squares covers only the group)
int dw_group_epilogue(const DwEpilogue& x) {
  if (!g_dwq.on) return set_error(SMI_E_ARG, "dw group: no open group for the epilogue");
  g_dwq.grp.x = x;
  g_dwq.grp.x.on = 1;
  return SMI_OK;
}

static bool dw_group_add(const GemmArgs& g) {
  DwQueue& q = g_dwq;
  if (!q.on) return false;
  if (q.grp.ng >= kDwGemmMax) {
    q.missed = true;
    return false;
  }
  const DwAlign al = dw_align(g);
  const bool va = al.va && g.M >= 4;
  const int i = q.grp.ng++;
  q.grp.g[i] = g;
  // (bits 4 / 8: the dY / X bases are 16-byte aligned, the rule for the fitted
  // edges' 2- and 3-wide loads, which take any row stride and extent)
  q.grp.vec[i] = (va ? 2 : 0) + (al.vb ? 1 : 0) + (al.a ? 4 : 0) + (al.b ? 8 : 0);
  q.flops += dw_flops(g);
  return true;
}

// one weight gradient; rowmajor: row-major dY / X inside the grouped kernel's
// range.  In this order: queued in the open group; else flagged as missed by an
// open bracket and launched now, on gemm_dwd_kernel or (any other layout or
// size) on the tiled engine
static int dw_issue(const GemmArgs& g, bool rowmajor, hipStream_t st) {
  if (rowmajor && dw_group_add(g)) return SMI_OK;
  if (g_dwq.on) g_dwq.missed = true;     // runs outside the open group
  return rowmajor ? dwd_launch(g, st) : gemm_launch(EPI_DW, g, st);
}

// Workgroups of one grouped launch resident at once (CUs x occupancy).
static int dwd_group_slots(size_t lds) {
  static int slots = 0;
  if (!slots) {
    slots = resident_grid(gemm_dwd_group_kernel, 256, lds);
    if (slots < 1) slots = 256;
    // planned for the occupancy the kernel is built for (DWG_OCC),
    // not for what a build that happens to need fewer registers could reach:
    // the slot count sets the slab lengths, and with them every result's
    // rounding (a leaner build reached 4 per CU and moved every slab)
    int dev = 0, cus = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
        cus > 0 && slots > cus * DWG_OCC)
      slots = cus * DWG_OCC;
  }
  return slots;
}

// the planner over plain integers (CPU tests; no device call): gemms = ng x
// {M, N, K, vec, ones, split_col}; out = up to max_ent x {gi, m0, n0, M, N,
// mt, nt, kchunk, S, wg0, rb0, part_off}, tot = {workgroups, reducer blocks,
// floats of partials, rows per prefetch window}.  Returns the entry count.
extern "C" int smi_diag_dw_plan(const int* gemms, int ng, int waves, int slots, int64_t cap_floats,
                                int max_ent, int64_t* out, int64_t* tot) {
  if (!gemms || !out || !tot || ng < 1 || ng > kDwGemmMax || (waves != 4 && waves != 8) ||
      slots < 1 || max_ent < 1)
    return set_error(SMI_E_ARG, "smi_diag_dw_plan: bad arguments");
  DwPlanGemm pg[kDwGemmMax];
  for (int i = 0; i < ng; ++i) {
    pg[i] = DwPlanGemm{gemms[6 * i], gemms[6 * i + 1], gemms[6 * i + 2], gemms[6 * i + 3],
                       gemms[6 * i + 4], gemms[6 * i + 5]};
    if (!dw_group_takes(pg[i].M, pg[i].N) || pg[i].K < 1)
      return set_error(SMI_E_ARG, "smi_diag_dw_plan: GEMM outside the grouped kernel's range");
  }
  DwPlan P;
  if (dw_plan(pg, ng, waves, slots, cap_floats, max_ent, 0, P))
    return set_error(SMI_E_ARG, "smi_diag_dw_plan: the partials do not fit");
  for (int i = 0; i < P.n; ++i) {
    const DwPlanEnt& e = P.e[i];
    const int64_t row[12] = {e.gi, e.m0, e.n0, e.M, e.N, e.mt, e.nt, e.kchunk, e.S,
                             P.wg0[i], P.rb0[i], e.part_off};
    for (int j = 0; j < 12; ++j) out[12 * i + j] = row[j];
  }
  tot[0] = P.wg0[P.n]; tot[1] = P.rb0[P.n]; tot[2] = P.need; tot[3] = 4 * waves * DWD_P;
  return P.n;
}

// Plans G's ng queued GEMMs (dw_plan) and places the partials ws_off floats
// into the workspace; wv: waves per workgroup of the launch that runs them,
// slots: its resident workgroups.  Sets G.e / n / wg0 / rb0 and need (floats
// used from ws_off).
static int dw_prepare(DwGroup& G, int wv, int slots, int64_t ws_off, int64_t& need, int max_ent,
                      int target_fixed = 0) {
  DwPlanGemm pg[kDwGemmMax];
  for (int i = 0; i < G.ng; ++i) {
    const GemmArgs& g = G.g[i];
    pg[i] = DwPlanGemm{g.M, g.N, g.K, G.vec[i], g.ones_col >= 0 ? 1 : 0, g.B2 ? g.split_col : -1};
  }
  DwPlan P;
  if (dw_plan(pg, G.ng, wv, slots, smi_workspace_floats() - ws_off, max_ent, target_fixed, P))
    return set_error(SMI_E_ARG, "gemm: workspace too small for the grouped dW partials");
  need = P.need;
  float* base = workspace_f32(ws_off + need);
  if (!base) return set_error(SMI_E_ARG, "gemm: workspace too small for the grouped dW partials");
  base += ws_off;
  G.n = P.n;
  for (int i = 0; i < P.n; ++i) {
    const DwPlanEnt& p = P.e[i];
    DwEnt& e = G.e[i];
    e.part = base + p.part_off;
    e.gi = p.gi; e.m0 = p.m0; e.n0 = p.n0; e.M = p.M; e.N = p.N;
    e.kchunk = p.kchunk; e.S = p.S; e.gm = p.gm; e.gn = p.gn; e.cls = p.cls;
  }
  for (int i = 0; i <= P.n; ++i) { G.wg0[i] = P.wg0[i]; G.rb0[i] = P.rb0[i]; }
  return SMI_OK;
}

// Weight gradients of short batches without split-K: one 16 x 16 tile of one
// group entry per workgroup, the four waves splitting the rows in 16-row
// chunks (wave w takes c = w, w + 4, ...) through a ring of DR chunks in
// flight, two accumulator chains (even / odd chunk of the wave), a fixed-order
// LDS sum of the four waves, then the destination written directly (dw_put:
// no partials, no reducer launch).  Lane (i, q) reads dY[k][m0 + i] and
// X[k][n0 + i] for k = 16c + 4q + s: 16 consecutive floats per row on both
// operands.  The two-source B of the LSTM's [x_t | h_{t-1}] (B2) and the
// bias column are formed per lane.  Measured on the LSTM's gradient at 3200
// rows (a rank's batch): 28-30 us against 21.6 us on the grouped dW launch
// (800 scalar operand loads per lane), so only short groups take it.
constexpr int DWT_DR = 8;   // chunks in flight per wave (the trip's accumulators)
__global__ void __launch_bounds__(kWG)
gemm_dwt16_kernel(DwGroup G) {
  __shared__ f32x4 red[4][64];
  const int b = blockIdx.x;
  int gi = 0;
  while (gi + 1 < G.ng && b >= G.wg0[gi + 1]) ++gi;
  const GemmArgs& g = G.g[gi];
  if (g.skip && g.skip[0] != 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, q = lane >> 4;
  const int local = b - G.wg0[gi], gn16 = (g.N + 15) >> 4;
  const int m0 = (local / gn16) * 16, n0 = (local % gn16) * 16;
  const int mi = min(m0 + i, g.M - 1), ni = n0 + i;
  const int bdata = g.ones_col >= 0 ? g.ones_col : g.N;
  const float* Ar = g.A + (int64_t)mi * g.a_rs;
  // column ni of B: the first source, the second (B2: columns >= split_col),
  // a padding column (c1_real <= ni < split_col), the bias column or past N
  const float* Bc = g.B;
  int64_t bs = g.b_rs;
  bool bz = false, bone = false;
  if (ni == g.ones_col) bone = true;
  else if (ni >= bdata || ni >= g.N) bz = true;
  else if (g.B2 && ni >= g.split_col) { Bc = g.B2 + (ni - g.split_col); bs = g.b2_rs; }
  else if (g.B2 && ni >= g.c1_real) bz = true;
  else Bc = g.B + (int64_t)ni * g.b_cs;
  const int nch = (g.K + 15) >> 4;
  const int nw = nch > wave ? (nch - wave + 3) >> 2 : 0;        // this wave's chunks
  float av[DWT_DR][4], bv[DWT_DR][4];
  auto ld = [&](int j, int slot) {
    const int c = wave + 4 * j;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int k = 16 * c + 4 * q + t;
      const bool kv = j < nw && k < g.K;
      av[slot][t] = kv ? Ar[(int64_t)k * g.a_cs] : 0.f;
      bv[slot][t] = kv ? (bone ? 1.f : bz ? 0.f : Bc[(int64_t)k * bs]) : 0.f;
    }
  };
#pragma unroll
  for (int d = 0; d < DWT_DR; ++d) ld(d, d);
  // each ring trip: one fresh MFMA chain per slot (16 products), the trip's
  // four chains summed in a fixed tree into the running total (short fp32
  // chains: at 3200 rows a single chain per wave was ~2x the oracle's fp32
  // spread on the C3 rank fixture's update bars)
  f32x4 tot = {0.f, 0.f, 0.f, 0.f};
  for (int j0 = 0; j0 < nw; j0 += DWT_DR) {
    f32x4 acc[DWT_DR];
#pragma unroll
    for (int d = 0; d < DWT_DR; ++d) {
      acc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (j0 + d < nw) {
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[d] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[d][t], bv[d][t], acc[d], 0, 0, 0);
      }
      ld(j0 + d + DWT_DR, d);
    }
    tot += ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  }
  red[wave][lane] = tot;
  __syncthreads();
  if (wave != 0) return;
  const f32x4 sum = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
  if (ni >= g.N) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = m0 + 4 * q + r;
    if (m < g.M) dw_put(g, m, ni, sum[r]);
  }
}

static void dwt16_prefix(DwGroup& G) {
  G.wg0[0] = 0;
  for (int i = 0; i < G.ng; ++i)
    G.wg0[i + 1] = G.wg0[i] + ((G.g[i].M + 15) / 16) * ((G.g[i].N + 15) / 16);
}

constexpr size_t kDwdLds = (size_t)2 * 4 * DWG_NT * 64 * sizeof(float4);

// the form name of a grouped launch or of its reducer (smi_last_launch): the
// distinct tile classes of its entries in entry order, MT x NT sub-tiles, a
// 4-wide operand marked v (16-byte loads) or s (per-column loads), e.g.
// gemm_group_reduce_kernel<gemm_dwd_group_kernel<4vx4v,1x4v,4vx3,1x3>>
static const char* dw_group_name(const DwGroup& G, bool reducer) {
  static thread_local char buf[2][320];
  char* b = buf[reducer ? 1 : 0];
  size_t o = (size_t)snprintf(b, sizeof(buf[0]), "%s", reducer ? "gemm_group_reduce_kernel<gemm_dwd_group_kernel<"
                                                            : "gemm_dwd_group_kernel<");
  int seen[kDwGroupMax], ns = 0;
  for (int i = 0; i < G.n; ++i) {
    const int c = G.e[i].cls;
    bool dup = false;
    for (int j = 0; j < ns; ++j) dup = dup || seen[j] == c;
    if (dup) continue;
    seen[ns++] = c;
    const int mt = c & 7, nt = (c >> 3) & 15;
    o += (size_t)snprintf(b + o, sizeof(buf[0]) - o, "%s%d%sx%d%s", ns > 1 ? "," : "", mt,
                          mt == 4 ? ((c >> 7) & 1 ? "v" : "s") : "", nt,
                          nt >= 4 ? ((c >> 8) & 1 ? "v" : "s") : "");
  }
  snprintf(b + o, sizeof(buf[0]) - o, "%s", reducer ? ">>" : ">");
  return b;
}

int dw_group_flush(hipStream_t st) {
  DwQueue& q = g_dwq;
  q.on = false;
  DwGroup& G = q.grp;
  const bool missed = q.missed;
  q.missed = false;
  const bool pre = q.pre_on;
  q.pre_on = false;
  // the pre partials stay reserved through this flush's own requests (its
  // partials land above them), released on every return
  struct Release { ~Release() { workspace_reserve(0); } } release_;
  if (G.x.on && G.x.sq && missed)
    return set_error(SMI_E_ARG, "dw group: a fused sum of squares needs every dW GEMM of the "
                                "bracket in the group (one ran outside it)");
  G.n = 0;
  if (G.ng == 0 && !pre) {
    if (!G.x.on) return SMI_OK;
    if (G.x.sq) return set_error(SMI_E_ARG, "dw group: fused sum of squares over an empty group");
    G.rb0[0] = 0;                                   // the epilogue task alone
    hipLaunchKernelGGL(gemm_group_reduce_kernel<1>, dim3(1), dim3(kWG), 0, st, G);
    return check_launch("gemm_group_reduce_kernel");
  }
  // short batches (every entry <= 512 rows, one group, no epilogue task):
  // 16 x 16 tiles written directly, no partials and no reducer
  if (!pre && !G.x.on) {
    bool small = G.ng > 0;
    for (int i = 0; i < G.ng; ++i) small = small && G.g[i].K <= 4 * 16 * T16_MAXC;
    if (small) {
      dwt16_prefix(G);
      const int kslot = ktime_begin(st);
      hipLaunchKernelGGL(gemm_dwt16_kernel, dim3(G.wg0[G.ng]), dim3(kWG), 0, st, G);
      ktime_end(kslot, KT_GEMM_DW, q.flops, st);
      return check_launch("gemm_dwt16_kernel");
    }
  }
  int64_t need = 0;
  if (G.ng > 0) {
    if (pre && q.pre.ng + G.ng > kDwGemmMax) return set_error(SMI_E_ARG, "dw group: too many GEMMs");
    RC_CHECK(dw_prepare(G, kDwdWaves, dwd_group_slots(kDwdLds), 0, need,
                        kDwGroupMax - (pre ? q.pre.n : 0)));
    const int kslot = ktime_begin(st);
    hipLaunchKernelGGL(gemm_dwd_group_kernel, dim3(G.wg0[G.n]), dim3(256), kDwdLds, st, G);
    ktime_end(kslot, KT_GEMM_DW, q.flops, st);
    RC_CHECK(check_launch(dw_group_name(G, false)));
  }
  // the reducer sums the partials of the entries launched with the BPTT and
  // of these, in one launch
  DwGroup R = G;
  if (pre) {
    R = q.pre;
    R.x = G.x;
    if (R.n + G.n > kDwGroupMax) return set_error(SMI_E_ARG, "dw group: too many entries");
    for (int i = 0; i < G.ng; ++i) R.g[R.ng + i] = G.g[i];
    for (int i = 0; i < G.n; ++i) {
      const int j = R.n + i;
      R.e[j] = G.e[i];
      R.e[j].gi += R.ng;
      R.rb0[j + 1] = R.rb0[j] + (G.rb0[i + 1] - G.rb0[i]);
    }
    R.ng += G.ng;
    R.n += G.n;
    need += q.pre_need;
  }
  const int rslot = ktime_begin(st);
  hipLaunchKernelGGL(gemm_group_reduce_kernel<kRedU>, dim3(R.rb0[R.n] + (R.x.on ? 1 : 0)), dim3(kWG), 0,
                     st, R);
  ktime_end(rslot, KT_GEMM_REDUCE, (double)need, st);
  return check_launch(dw_group_name(R, true));
}

int launch_lstm_bwd_dw(const float* dh, const float* gates, const float* cbuf, const float* w_hh,
                       int S, int B, int H, float* dgates, hipStream_t st, const int* skip) {
  const int br = lstm_bwd_q_form(B, H, w_hh);
  DwQueue& q = g_dwq;
  if (!q.on || q.pre_on || q.grp.ng == 0 || br == 0 || S <= 0 || B <= 0)
    return SMI_E_NOFIT;
  int cus = 0, dev = 0;
  (void)hipGetDevice(&dev);
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
  if (cus - B < 32) return SMI_E_NOFIT;             // too few CUs left beside the recurrence
  DwGroup Ga = q.grp;
  int64_t need = 0;
  // balanced for the CUs the recurrence leaves idle (a fixed one-round target
  // of cus - B workgroups with equal slabs: 50.6 vs 30.9 us per launch at 128
  // segments — slab rounding pushed the count past one round)
  // (entries: one stays free for every GEMM the group may still queue)
  RC_CHECK(dw_prepare(Ga, 8, cus - B, 0, need, kDwGroupMax - (kDwGemmMax - Ga.ng)));
  // one workgroup per CU (the LDS request): the recurrence's workgroups keep
  // their CUs to themselves, the weight gradients take the others
  const size_t lds = std::max(kDwdLds, (size_t)84 * 1024);
  LstmBwdArgs la{dh, gates, cbuf, w_hh, S, B, H, dgates, skip};
  const dim3 grid((unsigned)(B + Ga.wg0[Ga.n]));
  const int kslot = ktime_begin(st);
#define SMI_BD(BR_)                                                                          \
  do {                                                                                       \
    allow_lds(lstm_bwd_dw_kernel<BR_>, lds);                                                 \
    hipLaunchKernelGGL((lstm_bwd_dw_kernel<BR_>), grid, dim3(kVT), lds, st, la, Ga);         \
  } while (0)
  if (br == 16) SMI_BD(16);
  else if (br == 25) SMI_BD(25);
  else SMI_BD(32);
#undef SMI_BD
  ktime_end(kslot, KT_LSTM_BWD, 8.0 * B * H * (double)H * (S - 1), st);
  RC_CHECK(check_launch("lstm_bwd_dw_kernel"));
  q.pre = Ga;
  q.pre_on = true;
  q.pre_need = need;
  workspace_reserve(need);     // no launch before the flush may reuse these partials
  q.grp.ng = q.grp.n = 0;                           // the group queues the rest
  q.flops = 0.0;                                    // (its launch times the rest only)
  return SMI_OK;
}

// weight gradients of two layers fed by the same dY over [X1 | X2] (the LSTM:
// W_ih over x_t, W_hh over h_{t-1}, one bias gradient shared by b_ih / b_hh)
// in ONE launch: dY read once, one split-K reduce.  X1 has K1 real columns and
// row stride ldx1 (a multiple of 4 >= K1: the padding columns are computed and
// dropped so both sources load as 16-byte vectors).
int launch_linear_bwd_dw2(const float* dY, int64_t ldg, int M, int N, const float* X1,
                          int64_t ldx1, int K1, const float* X2, int64_t ldx2, int K2,
                          float* dW1, int64_t ld1, float* dW2, int64_t ld2, float* db1,
                          float* db2, hipStream_t st, const int* skip) {
  const int K1p = (int)ldx1;
  if (K1p < K1 || K1p % 4) return set_error(SMI_E_ARG, "bwd_dw2: ldx1 must be a multiple of 4 >= K1");
  GemmArgs g{};
  g.M = N; g.N = K1p + K2 + 1; g.K = M;
  g.A = dY; g.a_rs = 1; g.a_cs = ldg;
  g.B = X1; g.b_rs = ldx1; g.b_cs = 1;
  g.B2 = X2; g.b2_rs = ldx2; g.split_col = K1p; g.c1_real = K1;
  g.C = dW1; g.ldc = ld1; g.C2 = dW2; g.ldc2 = ld2;
  g.ones_col = K1p + K2; g.bias_out = db1; g.bias_out2 = db2; g.skip = skip;
  if (!dw_group_takes(g.M, g.N)) return set_error(SMI_E_ARG, "bwd_dw2: shape not supported");
  return dw_issue(g, true, st);
}

int launch_linear_bwd_dw(const float* dY, int64_t ldg, int M, int N, const float* X, int64_t ldx,
                         int K, float* dW, int64_t lddw, float* db, int accumulate,
                         hipStream_t st, const int* skip) {
  GemmArgs g{};
  g.M = N; g.N = db ? K + 1 : K; g.K = M;
  g.A = dY; g.a_rs = 1; g.a_cs = ldg;       // A(m=n, k=r) = dY[r][n]
  g.B = X; g.b_rs = ldx; g.b_cs = 1;        // B(k=r, n=k') = X[r][k'] (k' == K: 1)
  g.C = dW; g.ldc = lddw; g.accumulate = accumulate; g.skip = skip;
  g.ones_col = db ? K : -1;
  g.bias_out = db;
  if (g.M <= 0 || g.N <= 0) return SMI_OK;
  const bool rowmajor = g.a_rs == 1 && g.b_cs == 1 && g.K >= 1 &&
                        (g.ones_col >= 0 ? g.ones_col : g.N) >= 1 && dw_group_takes(g.M, g.N);
  return dw_issue(g, rowmajor, st);
}

}  // namespace smi
