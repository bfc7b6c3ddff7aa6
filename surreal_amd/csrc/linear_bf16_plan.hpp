// linear_bf16_plan.hpp — tile form and split-K choice of the bf16 dense layers
// (linear_bf16_kernels.hip).  Host-only arithmetic, a pure function of the GEMM
// shape and the workspace size: the same call always runs the same form with
// the same slabs on every device, so its bits do not depend on where it runs.
#pragma once
#include <stdint.h>

namespace smi {

constexpr int kLinBfRows = 64;     // output rows per workgroup: 16 per wave
constexpr int kLinBfChunk = 64;    // reduction elements staged per step: two 16x16x32 MFMA k-steps
constexpr int kLinBfLdv = kLinBfChunk / 8 + 1;   // LDS row in 16-byte vectors of 8 bf16: 8 + 1 pad
constexpr int kLinBfNarrow = 16;   // outputs up to this wide take the 16-column tile
// split-K: outputs with fewer tiles than one MI355X has CUs, cut towards two
// workgroups per CU (constants, not device queries: see above)
constexpr int kLinBfFill = 256;
constexpr int kLinBfTarget = 512;

struct LinBfPlan {
  int nt;        // 16-column MFMA tiles per wave: 4 (64 x 64 tile) or 1 (64 x 16)
  int gm, gn;    // tiles along the rows and the columns of the output
  int splits;    // slabs of the reduction (gridDim.z); 1: no split, no reducer
  int kchunk;    // reduction elements per slab, a multiple of kLinBfChunk
};

inline int64_t lin_bf_ceil(int64_t a, int64_t b) { return (a + b - 1) / b; }

// C [M][N] = sum over K; ws_floats: the capacity of the split-K workspace
inline LinBfPlan linear_bf16_plan(int M, int N, int K, int64_t ws_floats) {
  LinBfPlan p{};
  p.nt = N <= kLinBfNarrow ? 1 : 4;
  p.gm = (int)lin_bf_ceil(M, kLinBfRows);
  p.gn = (int)lin_bf_ceil(N, 16 * p.nt);
  const int64_t chunks = lin_bf_ceil(K, kLinBfChunk);
  p.splits = 1;
  p.kchunk = (int)(chunks * kLinBfChunk);
  const int64_t tiles = (int64_t)p.gm * p.gn;
  if (tiles < 1 || tiles >= kLinBfFill || chunks < 4) return p;
  int64_t want = lin_bf_ceil(kLinBfTarget, tiles);
  if (want > chunks / 2) want = chunks / 2;            // a slab holds at least two chunks
  const int64_t cap = ws_floats / ((int64_t)M * N);
  if (want > cap) want = cap;
  if (want < 2) return p;
  const int64_t per = lin_bf_ceil(chunks, want);
  p.splits = (int)lin_bf_ceil(chunks, per);            // no empty slab; the last may be ragged
  p.kchunk = (int)(per * kLinBfChunk);
  return p;
}

// The weight gradient dW [out][in] = sum over the rows (linear_bf16_dw_kernel):
// 64 x 64 tiles, or 16 (out) x 64 (in) for the head layers; nt is the count of
// 16-row blocks along out (4 or 1), kchunk the rows of a slab.  A slab's partial
// image holds in + 1 columns (the last: the bias gradient), whether or not the
// call asks for db: the plan is a function of the shape alone.
inline LinBfPlan linear_bf16_dw_plan(int out, int in, int rows, int64_t ws_floats) {
  LinBfPlan p{};
  p.nt = out <= kLinBfNarrow ? 1 : 4;
  p.gm = (int)lin_bf_ceil(out, 16 * p.nt);
  p.gn = (int)lin_bf_ceil(in, kLinBfRows);
  const int64_t chunks = lin_bf_ceil(rows, kLinBfChunk);
  p.splits = 1;
  p.kchunk = (int)(chunks * kLinBfChunk);
  const int64_t tiles = (int64_t)p.gm * p.gn;
  if (tiles < 1 || tiles >= kLinBfFill || chunks < 4) return p;
  int64_t want = lin_bf_ceil(kLinBfTarget, tiles);
  if (want > chunks / 2) want = chunks / 2;            // a slab holds at least two chunks
  const int64_t cap = ws_floats / ((int64_t)out * (in + 1));
  if (want > cap) want = cap;
  if (want < 2) return p;
  const int64_t per = lin_bf_ceil(chunks, want);
  p.splits = (int)lin_bf_ceil(chunks, per);            // no empty slab; the last may be ragged
  p.kchunk = (int)(per * kLinBfChunk);
  return p;
}

// static LDS of a form: two stages of the A (64 rows) and B (16 nt rows) images
constexpr int linear_bf16_lds_bytes(int nt) { return 2 * (kLinBfRows + 16 * nt) * kLinBfLdv * 16; }

}  // namespace smi
