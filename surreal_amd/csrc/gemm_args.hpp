// gemm_args.hpp — what the two GEMM units share: linear_kernels.hip (forwards
// and input gradients) and linear_dw.hip (weight gradients).
#pragma once
#ifndef SMI_GEMM_UNIT
#error "define SMI_GEMM_UNIT (the unit's namespace for its zero row) before gemm_args.hpp"
#endif
#include "smi_device.hpp"
#include "smi_internal.hpp"
#include "dw_plan.hpp"

namespace smi {

enum { EPI_FWD = 0, EPI_DX = 1, EPI_DW = 2 };

struct GemmArgs {
  int M, N, K;
  // A(m,k) = A[m*a_rs + k*a_cs], B(k,n) = B[k*b_rs + n*b_cs]
  const float* A; int64_t a_rs, a_cs;
  const float* B; int64_t b_rs, b_cs;
  float* C; int64_t ldc;          // C[m*ldc + n]
  const float* bias;              // EPI_FWD
  int act;                        // EPI_FWD: ACT_*
  const float* mask; int64_t ldm; // EPI_DX: zero where mask[m*ldm+n] <= 0 (may be null)
  int accumulate;                 // EPI_DW (no split): C += result
  int ones_col;                   // EPI_DW: B(k, ones_col) == 1 (bias gradient column), -1 none
  float* bias_out;                // EPI_DW: column ones_col goes to bias_out[m]
  int kchunk;                     // K range of blockIdx.z: [z*kchunk, min(K, (z+1)*kchunk))
  float* part;                    // split-K partials [gridDim.z][M][N] (nullptr: no split)
  const int* skip;                // device flag: nonzero -> no-op (early stop)
  int avec, bvec;                 // 16-byte operand loads (set by gemm_launch)
  // EPI_DW with a two-source B (the LSTM's [x_t | h_{t-1}], one launch for the
  // W_ih and W_hh gradients): B2 != null makes columns n >= split_col read
  // B2[k*b2_rs + n - split_col] and land in C2 (ld ldc2); columns c1_real <= n
  // < split_col are padding (never stored); bias_out2 receives a copy of the
  // bias column (b_ih and b_hh have the same gradient).
  const float* B2; int64_t b2_rs; int split_col, c1_real;
  float* C2; int64_t ldc2; float* bias_out2;
  // EPI_FWD on the short-batch kernel: also C[m][N + j] = xsrc[m*xlds + j],
  // j < xcols (CriticNetworkX's cat(h1, action): the action block of the
  // next layer's input written by the layer that writes h1)
  const float* xsrc; int64_t xlds; int xcols;
};

// where output (m, n) of a weight gradient goes (bias column, the second
// destination of a two-source B, padding); returns the sum of squares of the
// values it stored (each destination element once: b_ih and b_hh both hold the
// bias gradient, so it counts twice, as in clip_grad_norm_ over both)
__device__ __forceinline__ float dw_put(const GemmArgs& g, int m, int n, float v) {
  if (n == g.ones_col) {
    const float b = g.accumulate ? g.bias_out[m] + v : v;
    g.bias_out[m] = b;
    if (g.bias_out2) {
      const float b2 = g.accumulate ? g.bias_out2[m] + v : v;
      g.bias_out2[m] = b2;
      return b * b + b2 * b2;
    }
    return b * b;
  }
  float* dst;
  if (g.B2 && n >= g.split_col) dst = g.C2 + (int64_t)m * g.ldc2 + (n - g.split_col);
  else if (g.B2 && n >= g.c1_real) return 0.f;               // padding column
  else dst = g.C + (int64_t)m * g.ldc + n;
  const float r = g.accumulate ? *dst + v : v;
  *dst = r;
  return r * r;
}

// flops of a weight gradient as ktime_end counts them: the bias column costs a
// row sum, the padding columns of a two-source B do no work
inline double dw_flops(const GemmArgs& g) {
  const int nreal = (g.ones_col >= 0 ? g.N - 1 : g.N) - (g.B2 ? g.split_col - g.c1_real : 0);
  return 2.0 * g.M * (double)nreal * g.K + (g.ones_col >= 0 ? (double)g.M * g.K : 0.0);
}

// XCD-aware tile order (cdna_hip_programming.md T1): the dispatcher deals
// consecutive workgroups round-robin over the 8 XCDs (private L2 each); the
// bijective remap gives every XCD a contiguous run of the logical order, in
// which n-tiles of one m-tile (sharing A rows) and the tiles of one split-K
// slab (sharing the slab's rows of both operands) are neighbours.
// orig: the workgroup's index among the launch's nwg (it must agree with the
// hardware's dispatch order mod 8); returns its place in the logical order
__device__ __forceinline__ int xcd_contiguous(int orig, int nwg) {
  int w = orig;
  if (nwg > 8) {
    const int x = orig & 7, q = nwg >> 3, r = nwg & 7;
    w = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (orig >> 3);
  }
  return w;
}
struct TileIdx { int mt, nt, z; };
__device__ __forceinline__ TileIdx gemm_tile_index() {
  const int gm = gridDim.x, gn = gridDim.y;
  const int nwg = gm * gn * gridDim.z;
  const int orig = blockIdx.x + gm * (blockIdx.y + gn * blockIdx.z);
  const int w = xcd_contiguous(orig, nwg);
  TileIdx t;
  t.nt = w % gn;
  t.mt = (w / gn) % gm;
  t.z = w / (gn * gm);
  return t;
}

// short-batch 16 x 16-tile kernels (gemm_t16_kernel, gemm_dwt16_kernel): 16-k
// chunks per wave, K <= 4 * 16 * 8 = 512
constexpr int T16_MAXC = 8;

// one tile of a grouped launch: rectangle [m0, m0 + M) x [n0, n0 + N) of GEMM
// gi's output in tiles of MT x NT sub-tiles, S slabs of kchunk rows each
struct DwEnt {
  float* part;                   // split-K partials [S][M][N]
  int gi;                        // the GEMM (DwGroup::g)
  int m0, n0, M, N;
  int kchunk, S;
  int gm, gn;                    // tiles
  int cls;                       // dw_cls(): tile class MT x NT and the 16-byte operand flags
};

struct DwGroup {
  DwEpilogue x;                  // optional epilogue task of the reducer (smi_internal.hpp)
  GemmArgs g[kDwGemmMax];
  DwEnt e[kDwGroupMax];
  int wg0[kDwGroupMax + 1];      // workgroup prefix (by entry; gemm_dwt16_kernel: by GEMM)
  int rb0[kDwGroupMax + 1];      // reducer-block prefix
  int vec[kDwGemmMax];           // 2*VA + VB of each GEMM's 16-byte operand loads
  int ng, n;                     // GEMMs, entries
};
// kernel arguments: 4 KiB (lstm_bwd_dw_kernel passes the BPTT's arguments too)
static_assert(sizeof(DwGroup) + 128 <= 4096, "DwGroup must fit the kernel-argument segment");

// zero row / ones vector selected by address (dwd_load, the reducers, the
// panel kernel).  No relocatable device code in this build, so the two units
// cannot share a __device__ global: each names its own pair (the namespace
// SMI_GEMM_UNIT), 32 KiB more device memory and nothing else.  Not `static`:
// tools/kernel_diff.py showed an internal zero row become a .rodata constant
// (its loads may then fold to 0, the masking these rows exist to avoid) and,
// where a kernel's lambda uses it, an externalised symbol behind a GOT load.
constexpr int DWD_ZMAX = 8192;
namespace SMI_GEMM_UNIT {
__device__ __attribute__((aligned(16))) float g_dwd_zero[DWD_ZMAX];
__device__ __attribute__((aligned(16))) float g_dwd_one[4] = {1.f, 0.f, 0.f, 0.f};
}  // namespace SMI_GEMM_UNIT
using namespace SMI_GEMM_UNIT;

// ---- host functions that cross between linear_kernels.hip and linear_dw.hip --
// linear_kernels.hip: the tiled engine (a weight gradient the row-major forms
// of linear_dw.hip do not take: gemm_dw128_kernel or gemm_kernel<dw>), and the
// split-K reducer; what: "gemm_splitk_reduce_kernel<the producer's form>"
// (smi_last_launch)
int gemm_launch(int epi, GemmArgs g, hipStream_t st);
int splitk_reduce(const GemmArgs& g, int S, int epi, hipStream_t st, const char* what);
// linear_dw.hip: gemm_dw128_kernel over gemm_launch's grid of D2_T x D2_T tiles
constexpr int D2_T = 128;
void dw128_dispatch(const GemmArgs& g, dim3 grid, hipStream_t st);

}  // namespace smi
