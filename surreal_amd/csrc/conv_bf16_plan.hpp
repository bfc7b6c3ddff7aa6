// conv_bf16_plan.hpp — tile, LDS and scratch arithmetic of the bf16 form of the
// general convolution layer (conv_bf16_kernels.hip).  Host-only arithmetic on
// top of conv_plan.hpp: the geometry (ConvGeom, conv_geom_ok), the 64 x 64
// output tiles, the stride-parity classes and the tile counts are the fp32
// form's; the reduction chunk and the LDS row differ.
#pragma once
#include "conv_plan.hpp"

namespace smi {

constexpr int kConvBfChunk = 64;   // reduction elements staged per step: two 16x16x32 MFMA k-steps
constexpr int kConvBfLdv = kConvBfChunk / 8 + 1;   // LDS row stride in 16-byte vectors of 8 bf16:
                                                   // 9 (144 bytes, 36 dwords; bank argument in
                                                   // conv_bf16_kernels.hip)

// weight gradient: conv_dw_plan with the reduction over n Ho Wo in steps of 64
inline ConvDwPlan conv_bf16_dw_plan(const ConvGeom& g, int64_t n) {
  ConvDwPlan q{};
  q.tiles = (int)(conv_ceil(g.cout, kConvTile) * conv_ceil(g.K, kConvTile));
  q.chunks = conv_ceil(n * g.P, kConvBfChunk);
  q.slab = (int64_t)g.cout * g.K + g.cout;
  if (q.chunks < 1) { q.per = 0; q.splits = 0; return q; }
  int64_t want = conv_ceil(kConvDwTarget, q.tiles);
  if (want > kConvMaxSplits) want = kConvMaxSplits;
  if (want > q.chunks) want = q.chunks;
  q.per = conv_ceil(q.chunks, want);
  q.splits = (int)conv_ceil(q.chunks, q.per);      // no empty split
  return q;
}

inline int64_t conv_bf16_scratch_bytes(const ConvGeom& g, int64_t n) {
  const ConvDwPlan q = conv_bf16_dw_plan(g, n);
  return 4 * (int64_t)q.splits * q.slab;
}

// static LDS of every kernel: the A and B tiles
constexpr int conv_bf16_lds_bytes() { return 2 * kConvTile * kConvBfLdv * 16; }

}  // namespace smi
