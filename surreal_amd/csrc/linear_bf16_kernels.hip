// linear_bf16_kernels.hip — the dense layer's forward and input gradient with
// bf16 operands on v_mfma_f32_16x16x32_bf16 (8 times the multiply-adds of
// v_mfma_f32_16x16x4_f32 per instruction):
//   fwd:  Y[m][n]  = act(b[n] + sum_k X[m][k] W[n][k])
//   dX:   dX[m][k] = [mask[m][k] > 0] * sum_n dY[m][n] W[n][k]
// Tensors stay fp32 in memory: an operand becomes bf16 on its way from the
// prefetch registers into LDS and nowhere else (pack8, bf16_stage.hpp: nearest
// even, NaN and infinities preserved).  A product of two bf16 values is exact
// in fp32 and the MFMA accumulates in fp32: after staging the only rounding is
// that of the fp32 sums.  Bias, activation and the mask test are fp32 in the
// epilogue, written as in linear_kernels.hip.  The weight gradient with bf16
// operands is the third kernel of this unit (below, before the host part).
//
// Both are  C[m][j] = sum_z A[m][z] B[j][z]  (fwd: A = X, B = W, z = k;
// dX: A = dY, B = W^T, z = n).  256 threads; wave w owns rows 16 w .. 16 w + 15 of
// a 64-row tile and all of its 16 NT columns (NT accumulators): NT = 4, the
// 64 x 64 form, or NT = 1, the 64 x 16 form of the head layers (6, 1, A N <= 16
// outputs), where a 64-wide tile would spend 3 of 4 MFMAs on padding.  The
// reduction runs in chunks of 64: per chunk a lane reads its row's two 16-byte
// A vectors and 2 NT B vectors (row l & 15, z group l >> 4), then 2 MFMAs per
// accumulator.  Two LDS stages, one barrier per chunk: the global loads of
// chunk c + 1 are issued into registers before chunk c's MFMAs and rounded
// into the other stage after them.
//
// LDS: both images are [row][z] with z contiguous, all traffic in 16-byte
// vectors of 8 bf16, a row is 9 of them (8 of data + 1 of padding = 144 bytes =
// 36 dwords).  Operand read: the 16 lanes of a quarter wave hold rows r0 ..
// r0 + 15 (r0 a multiple of 16: 36 r0 mod 64 = 0) at one z group, so they start
// at dwords 36 r mod 64 = 0 36 8 44 16 52 24 60 32 4 40 12 48 20 56 28: 16
// different multiples of 4, their ds_read_b128 cover each of the 64 banks once.
// Staging stores, 16 bytes each:
//   z-contiguous operand (X, dY; W in the forward): thread (row t >> 3,
//     vector t & 7) — 8 lanes along a row and the next 8 on the next row, 2-way
//     on 4 banks at worst.  Two 16-byte global loads (or 8 dwords) of 8
//     consecutive z become one store.
//   W in the input gradient (z = n is W's row: not contiguous): transposed in
//     registers.  Thread t < 32 NT takes column quad cq = (t & 3) | (t >> 5) << 2
//     and z octet zo = (t >> 2) & 7: 8 loads of 16 bytes W[8 zo + e][4 cq ..
//     4 cq + 3] (4 lanes cover 64 contiguous bytes, lane + 32 the next 64), then
//     per column the 8 rounded values along z as one vector at row 4 cq + c,
//     vector zo: dword 36 (4 cq + c) + 4 zo = 16 (t & 3) + 4 zo + 36 c mod 64, and
//     16 consecutive lanes have 4 values of t & 3 and 4 of zo within one half
//     of its range: 16 different multiples of 4, every bank once.  No 2-byte
//     LDS stores.  Waves 0 and 1 do this (32 values per thread); waves 2 and 3
//     stage dY (rows t' >> 3 + 16 h, 32 values per thread), so every thread
//     prefetches 32 floats in both directions.
//
// Edges: any M, K, N >= 1.  Every load has a clamped address and its value is
// zeroed afterwards by a select (no predicated loads, 0 * NaN never formed
// from padding).  16-byte or dword loads are decided once per launch and
// operand (GemmArgs avec / bvec) from the base alignment, the leading dimension
// and the contiguous extent, all in multiples of 4 floats: operands inside a
// flat parameter buffer start anywhere.
//
// Split-K (linear_bf16_plan.hpp): an output with fewer than 256 tiles over a
// reduction of at least 4 chunks is cut over gridDim.z into slabs of a
// multiple of 64, at least two chunks each; partial sums go to the library
// workspace and the fixed-order reducer of linear_kernels.hip applies the
// epilogue.  No atomics: two calls on the same inputs give the same bits.
//
// Sum order of one output: within a 32-wide k-step the instruction's own
// chain; the two k-steps of a chunk and the chunks of a slab ascending into the
// running accumulator; slabs ascending (four interleaved lanes) in the reducer.
#include <cmath>
#define SMI_GEMM_UNIT gemm_bf16
#include "gemm_args.hpp"
#include "bf16_stage.hpp"
#include "bf16_loads.hpp"
#include "linear_bf16_plan.hpp"

namespace smi {

namespace {

constexpr int LDV = kLinBfLdv;
static_assert(kWG == 256 && kLinBfRows == 64 && kLinBfChunk == 64 && LDV == 9,
              "the staging maps below are written for 256 threads and 64 x 64 slices");

}  // namespace      (load_z8, load_t4x8: bf16_loads.hpp)

// grid (row tiles, column tiles, slabs); g.A / g.B / g.C in gemm_args.hpp's
// terms: fwd B(z, j) = W[j][z] (b_cs = ldw), dX B(z, j) = W[z][j] (b_rs = ldw)
template <int EPI, int NT>
__global__ void __launch_bounds__(kWG)
linear_bf16_kernel(GemmArgs g) {
  if (g.skip && g.skip[0] != 0) return;
  constexpr int BR = 16 * NT;                         // columns of the tile = rows of the B image
  __shared__ uint4 As[2][kLinBfRows * LDV];
  __shared__ uint4 Bs[2][BR * LDV];
  const int tid = threadIdx.x, l = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const TileIdx ti = gemm_tile_index();
  const int m0 = ti.mt * kLinBfRows, n0 = ti.nt * BR;
  const int zb = ti.z * g.kchunk;
  const int ze = min(g.K, zb + g.kchunk);
  const int nc = (ze - zb + kLinBfChunk - 1) / kLinBfChunk;
  const int t2 = tid & 127;                           // index within the wave pair (dX)
  const int cq = (t2 & 3) | ((t2 >> 5) << 2), zo = (t2 >> 2) & 7;

  float pf[32];
  auto fetch = [&](int z0) {
    if constexpr (EPI == EPI_FWD) {
      const int z = z0 + 8 * (tid & 7);
#pragma unroll
      for (int h = 0; h < 2; ++h)
        load_z8(g.A, g.a_rs, m0 + (tid >> 3) + 32 * h, g.M, z, ze, g.avec, pf + 8 * h);
      if constexpr (NT == 4) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
          load_z8(g.B, g.b_cs, n0 + (tid >> 3) + 32 * h, g.N, z, ze, g.bvec, pf + 16 + 8 * h);
      } else {
        if (w < 2) load_z8(g.B, g.b_cs, n0 + (tid >> 3), g.N, z, ze, g.bvec, pf + 16);
      }
    } else {
      if (w < 2) {
        if (t2 < 32 * NT) load_t4x8(g.B, g.b_rs, z0 + 8 * zo, ze, n0 + 4 * cq, g.N, g.bvec, pf);
      } else {
#pragma unroll
        for (int h = 0; h < 4; ++h)
          load_z8(g.A, g.a_rs, m0 + (t2 >> 3) + 16 * h, g.M, z0 + 8 * (t2 & 7), ze, g.avec,
                  pf + 8 * h);
      }
    }
  };
  auto stage = [&](int s) {
    uint4* Sa = As[s];
    uint4* Sb = Bs[s];
    if constexpr (EPI == EPI_FWD) {
      Sa[(tid >> 3) * LDV + (tid & 7)] = pack8(pf);
      Sa[((tid >> 3) + 32) * LDV + (tid & 7)] = pack8(pf + 8);
      if constexpr (NT == 4) {
        Sb[(tid >> 3) * LDV + (tid & 7)] = pack8(pf + 16);
        Sb[((tid >> 3) + 32) * LDV + (tid & 7)] = pack8(pf + 24);
      } else {
        if (w < 2) Sb[(tid >> 3) * LDV + (tid & 7)] = pack8(pf + 16);
      }
    } else {
      if (w < 2) {
        if (t2 < 32 * NT) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            float col[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) col[e] = pf[4 * e + c];
            Sb[(4 * cq + c) * LDV + zo] = pack8(col);
          }
        }
      } else {
#pragma unroll
        for (int h = 0; h < 4; ++h) Sa[((t2 >> 3) + 16 * h) * LDV + (t2 & 7)] = pack8(pf + 8 * h);
      }
    }
  };

  f32x4 acc[NT];
#pragma unroll
  for (int c = 0; c < NT; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int lm = l & 15, lg = l >> 4;
  if (nc > 0) {
    fetch(zb);
    stage(0);
  }
  __syncthreads();
  for (int c = 0; c < nc; ++c) {
    const bool more = c + 1 < nc;
    if (more) fetch(zb + (c + 1) * kLinBfChunk);
    const uint4* ap = As[c & 1] + (16 * w + lm) * LDV + lg;
    const uint4* bp = Bs[c & 1] + lm * LDV + lg;
    // every operand of the chunk first (one LDS round trip), then its MFMAs
    uint4 a[2], b[NT][2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      a[kk] = ap[4 * kk];
#pragma unroll
      for (int t = 0; t < NT; ++t) b[t][kk] = bp[16 * t * LDV + 4 * kk];
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = mfma32(a[kk], b[t][kk], acc[t]);
    if (more) stage((c + 1) & 1);
    __syncthreads();
  }

  // epilogue: 4 rows x NT columns per lane (D[row 4 lg + e][col lm])
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n = n0 + 16 * t + lm;
    if (n >= g.N) continue;
    float bias_n = 0.f;
    if constexpr (EPI == EPI_FWD) bias_n = (g.bias && !g.part) ? g.bias[n] : 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int m = m0 + 16 * w + 4 * lg + e;
      if (m >= g.M) continue;
      float v = acc[t][e];
      if (g.part) {                                   // split-K slab: raw sums
        g.part[((int64_t)ti.z * g.M + m) * g.N + n] = v;
        continue;
      }
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

// ------------------------------------------------------- weight gradient
//   dW[o][i] (+)= sum_r bf16(dY[r][o]) bf16(X[r][i])     db[o] (+)= sum_r dY[r][o]
// C[o][i] = sum_z A[o][z] B[i][z] with z = r the batch row: BOTH operands are
// reduction-major in memory (r is the outer index of dY and of X), so both
// tiles take the register transpose W takes in the input gradient.  MT = 4: a
// 64 (out) x 64 (in) tile, wave w owns out rows 16 w .. 16 w + 15 and four
// accumulators along in; MT = 1: the 16 (out) x 64 (in) tile of the head layers
// (out <= 16), where the four waves' accumulators lie along in (wave w owns in
// columns 16 w .. 16 w + 15) and the A image has 16 rows.  Chunks of 64 rows, two
// stages, one barrier per chunk, the next chunk prefetched into registers, as
// above.
//
// Staging: waves 0 and 1 transpose the dY tile, waves 2 and 3 the X tile, 32
// floats per thread.  Thread t2 = tid & 127 of a wave pair takes column quad
// cq = (t2 & 3) | (t2 >> 5) << 2 (16 quads = 64 columns; MT = 1: only t2 < 32
// stage dY, 4 quads) and row octet zo = (t2 >> 2) & 7: 8 loads of 16 bytes
// P[r0 + 8 zo + e][4 cq .. 4 cq + 3] (4 lanes cover 64 contiguous bytes of a row),
// then per column the 8 rounded values along r as one 16-byte vector at image
// row 4 cq + c, vector zo.  Banks, for both images alike: the store starts at
// dword 36 (4 cq + c) + 4 zo = 16 (t2 & 3) + 4 zo + 36 c mod 64; 16 consecutive
// lanes hold 4 values of t2 & 3 and 4 consecutive zo of one half of its range:
// 16 different multiples of 4, every bank once.  The operand reads are those of
// the other two kernels (row l & 15 of a 16-row block, vector l >> 4).
//
// db comes from the UNROUNDED dy, in fp32, without a launch of its own: in the
// workgroups of in-tile 0 the dY threads add what they prefetched, before
// pack8, to four per-thread column sums (rows ascending); after the last chunk
// the 8 row-octet threads of a column are added through LDS, zo ascending, and
// thread o writes db[o] or, split, column in_dim of the slab's partial image
// (the reducer's ones_col / bias_out path).
//
// Split over the rows (linear_bf16_dw_plan): slabs of a multiple of 64 rows
// over gridDim.z, partials [slab][out][in (+ 1)] in the library workspace, the
// fixed-order reducer applies `accumulate`; unsplit, this epilogue does.
template <int MT>
__global__ void __launch_bounds__(kWG)
linear_bf16_dw_kernel(GemmArgs g) {
  if (g.skip && g.skip[0] != 0) return;
  constexpr int AR = 16 * MT;                         // rows of the A image: the out tile
  constexpr int NA = MT == 4 ? 4 : 1;                 // accumulators per wave
  __shared__ uint4 As[2][AR * LDV];
  __shared__ uint4 Bs[2][kLinBfRows * LDV];
  __shared__ float dbs[8][AR];
  const int tid = threadIdx.x, l = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const TileIdx ti = gemm_tile_index();
  const int o0 = ti.mt * AR, i0 = ti.nt * kLinBfRows;
  const int in_dim = g.ones_col >= 0 ? g.ones_col : g.N;
  const int zb = ti.z * g.kchunk;
  const int ze = min(g.K, zb + g.kchunk);
  const int nc = (ze - zb + kLinBfChunk - 1) / kLinBfChunk;
  const int t2 = tid & 127;
  const int cq = (t2 & 3) | ((t2 >> 5) << 2), zo = (t2 >> 2) & 7;
  const bool dyt = w < 2 && t2 < 32 * MT;             // this thread stages dY
  const bool bias = g.ones_col >= 0 && ti.nt == 0;    // this workgroup sums db (uniform)

  float pf[32];
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};
  auto fetch = [&](int z0) {
    if (w < 2) {
      if (dyt) load_t4x8(g.A, g.a_cs, z0 + 8 * zo, ze, o0 + 4 * cq, g.M, g.avec, pf);
    } else {
      load_t4x8(g.B, g.b_rs, z0 + 8 * zo, ze, i0 + 4 * cq, in_dim, g.bvec, pf);
    }
  };
  auto stage = [&](int s) {
    if (w < 2 && !dyt) return;
    if (bias && dyt) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) bsum[c] += pf[4 * e + c];
    }
    uint4* S = w < 2 ? As[s] : Bs[s];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float col[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) col[e] = pf[4 * e + c];
      S[(4 * cq + c) * LDV + zo] = pack8(col);
    }
  };

  f32x4 acc[NA];
#pragma unroll
  for (int t = 0; t < NA; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int lm = l & 15, lg = l >> 4;
  const int ar = MT == 4 ? 16 * w : 0, br = MT == 4 ? 0 : 16 * w;
  if (nc > 0) {
    fetch(zb);
    stage(0);
  }
  __syncthreads();
  for (int c = 0; c < nc; ++c) {
    const bool more = c + 1 < nc;
    if (more) fetch(zb + (c + 1) * kLinBfChunk);
    const uint4* ap = As[c & 1] + (ar + lm) * LDV + lg;
    const uint4* bp = Bs[c & 1] + (br + lm) * LDV + lg;
    uint4 a[2], b[NA][2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      a[kk] = ap[4 * kk];
#pragma unroll
      for (int t = 0; t < NA; ++t) b[t][kk] = bp[16 * t * LDV + 4 * kk];
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int t = 0; t < NA; ++t) acc[t] = mfma32(a[kk], b[t][kk], acc[t]);
    if (more) stage((c + 1) & 1);
    __syncthreads();
  }

  // epilogue: D[out row 4 lg + e][in column lm] of each accumulator
#pragma unroll
  for (int t = 0; t < NA; ++t) {
    const int i = i0 + br + 16 * t + lm;
    if (i >= in_dim) continue;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int o = o0 + ar + 4 * lg + e;
      if (o >= g.M) continue;
      const float v = acc[t][e];
      if (g.part) {                                   // slab: raw sums
        g.part[((int64_t)ti.z * g.M + o) * g.N + i] = v;
      } else {
        float* d = g.C + (int64_t)o * g.ldc + i;
        *d = g.accumulate ? *d + v : v;
      }
    }
  }
  if (!bias) return;
  if (dyt) {
#pragma unroll
    for (int c = 0; c < 4; ++c) dbs[zo][4 * cq + c] = bsum[c];
  }
  __syncthreads();
  const int o = o0 + tid;
  if (tid >= AR || o >= g.M) return;
  float s = dbs[0][tid];
#pragma unroll
  for (int z = 1; z < 8; ++z) s += dbs[z][tid];
  if (g.part) g.part[((int64_t)ti.z * g.M + o) * g.N + g.ones_col] = s;
  else g.bias_out[o] = g.accumulate ? g.bias_out[o] + s : s;
}

// ------------------------------------------------------------------- host
static int linear_bf16_launch(int epi, GemmArgs g, hipStream_t st) {
  if (g.M <= 0) return SMI_OK;
  auto al16 = [](const float* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const bool fwd = epi == EPI_FWD;
  // A is z-contiguous in both directions; B in the forward only
  g.avec = al16(g.A) && g.a_rs % 4 == 0 && g.K % 4 == 0;
  g.bvec = fwd ? al16(g.B) && g.b_cs % 4 == 0 && g.K % 4 == 0
               : al16(g.B) && g.b_rs % 4 == 0 && g.N % 4 == 0;
  const LinBfPlan pl = linear_bf16_plan(g.M, g.N, g.K, smi_workspace_floats());
  g.kchunk = pl.kchunk;
  g.part = nullptr;
  if (pl.splits > 1) {
    g.part = workspace_f32((int64_t)pl.splits * g.M * g.N);
    if (!g.part) return set_error(SMI_E_ARG, "linear bf16: workspace unavailable for split-K");
  }
  const dim3 grid(pl.gm, pl.gn, pl.splits);
  const char* form;
  const char* red;
  const int kslot = ktime_begin(st);
#define SMI_LBF(E, NTV, NAME)                                                               \
  do {                                                                                      \
    hipLaunchKernelGGL((linear_bf16_kernel<E, NTV>), grid, dim3(kWG), 0, st, g);            \
    form = "linear_bf16_kernel<" NAME ">";                                                  \
    red = "gemm_splitk_reduce_kernel<linear_bf16_kernel<" NAME ">>";                        \
  } while (0)
  if (fwd) { if (pl.nt == 4) SMI_LBF(EPI_FWD, 4, "fwd,64"); else SMI_LBF(EPI_FWD, 1, "fwd,16"); }
  else { if (pl.nt == 4) SMI_LBF(EPI_DX, 4, "dx,64"); else SMI_LBF(EPI_DX, 1, "dx,16"); }
#undef SMI_LBF
  ktime_end(kslot, fwd ? KT_GEMM_FWD : KT_GEMM_DX, 2.0 * g.M * (double)g.N * g.K, st);
  const int rc = check_launch(form);
  if (rc || pl.splits == 1) return rc;
  // the reducer is the last launch of a split call and names the form it sums
  return splitk_reduce(g, pl.splits, epi, st, red);
}

int launch_linear_fwd_bf16(const float* X, int64_t ldx, int M, int K, const float* W, int64_t ldw,
                           const float* b, int N, int act, float* Y, int64_t ldy, hipStream_t st,
                           const int* skip) {
  GemmArgs g{};
  g.M = M; g.N = N; g.K = K;
  g.A = X; g.a_rs = ldx; g.a_cs = 1;
  g.B = W; g.b_rs = 1; g.b_cs = ldw;        // B(k, n) = W[n][k]
  g.C = Y; g.ldc = ldy; g.bias = b; g.act = act; g.ones_col = -1; g.skip = skip;
  return linear_bf16_launch(EPI_FWD, g, st);
}

int launch_linear_bwd_dx_bf16(const float* dY, int64_t ldg, int M, int N, const float* W,
                              int64_t ldw, int K, const float* mask, int64_t ldm, float* dX,
                              int64_t lddx, hipStream_t st, const int* skip) {
  GemmArgs g{};
  g.M = M; g.N = K; g.K = N;
  g.A = dY; g.a_rs = ldg; g.a_cs = 1;
  g.B = W; g.b_rs = ldw; g.b_cs = 1;        // B(z = n', j = k') = W[n'][k']
  g.C = dX; g.ldc = lddx; g.mask = mask; g.ldm = ldm; g.ones_col = -1; g.skip = skip;
  return linear_bf16_launch(EPI_DX, g, st);
}

// launches at the call: never queued into an open dW group, whose state it
// does not read or change (the group's partials are placed at its flush)
int launch_linear_bwd_dw_bf16(const float* dY, int64_t ldg, int M, int N, const float* X,
                              int64_t ldx, int K, float* dW, int64_t lddw, float* db,
                              int accumulate, hipStream_t st, const int* skip) {
  if (M <= 0) return SMI_OK;
  auto al16 = [](const float* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  GemmArgs g{};
  g.M = N; g.N = db ? K + 1 : K; g.K = M;
  g.A = dY; g.a_rs = 1; g.a_cs = ldg;       // A(o, r) = dY[r][o]
  g.B = X; g.b_rs = ldx; g.b_cs = 1;        // B(r, i) = X[r][i]; column K: the bias gradient
  g.C = dW; g.ldc = lddw; g.accumulate = accumulate; g.skip = skip;
  g.ones_col = db ? K : -1;
  g.bias_out = db;
  // both operands are read in quads along their columns
  g.avec = al16(dY) && ldg % 4 == 0 && N % 4 == 0;
  g.bvec = al16(X) && ldx % 4 == 0 && K % 4 == 0;
  const LinBfPlan pl = linear_bf16_dw_plan(N, K, M, smi_workspace_floats());
  g.kchunk = pl.kchunk;
  g.part = nullptr;
  if (pl.splits > 1) {
    g.part = workspace_f32((int64_t)pl.splits * g.M * g.N);
    if (!g.part) return set_error(SMI_E_ARG, "linear bf16: workspace unavailable for split-K");
  }
  const dim3 grid(pl.gm, pl.gn, pl.splits);
  const int kslot = ktime_begin(st);
  if (pl.nt == 4) hipLaunchKernelGGL(linear_bf16_dw_kernel<4>, grid, dim3(kWG), 0, st, g);
  else hipLaunchKernelGGL(linear_bf16_dw_kernel<1>, grid, dim3(kWG), 0, st, g);
  ktime_end(kslot, KT_GEMM_DW, dw_flops(g), st);
  const int rc = check_launch(pl.nt == 4 ? "linear_bf16_kernel<dw,64>" : "linear_bf16_kernel<dw,16>");
  if (rc || pl.splits == 1) return rc;
  return splitk_reduce(g, pl.splits, EPI_DW, st,
                       pl.nt == 4 ? "gemm_splitk_reduce_kernel<linear_bf16_kernel<dw,64>>"
                                  : "gemm_splitk_reduce_kernel<linear_bf16_kernel<dw,16>>");
}

}  // namespace smi
