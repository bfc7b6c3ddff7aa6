// conv_plan.hpp — geometry, tile, LDS and scratch arithmetic of the general
// convolution layer (conv_kernels.hip).  Host-only arithmetic with no device
// or runtime call in it: tests/conv_plan_main.cpp sweeps it on the CPU under
// the sanitizers; the kernels read the same numbers through ConvGeom.
//
// One layer over NCHW tensors:
//   Ho = (H + 2 pad - k) / stride + 1, Wo likewise (integer division)
//   1 <= k <= 8, 1 <= stride <= min(k, 4), 0 <= pad < k, 1 <= cin, cout <= 128
// All three kernels are implicit GEMMs  C[R][Q] = sum_z A[R][z] * B[Q][z]  on
// 64 x 64 output tiles, reduced in chunks of 32:
//   forward          R = cout,  Q = n Ho Wo output pixels,   z = cin k k
//   backward input   R = cin,   Q = the input pixels of ONE stride-parity class
//                    (ry, rx) = ((iy + pad) % s, (ix + pad) % s),
//                    z = cout x the class's dense taps ky = ry + s jy, kx = rx + s jx
//   backward weight  R = cout,  Q = cin k k,  z = n Ho Wo, split over workgroups
#pragma once
#include <stdint.h>
#include "smi_shapes.hpp"      // SMI_HD (empty outside hipcc)

namespace smi {

constexpr int kConvTile = 64;      // rows and columns of an output tile
constexpr int kConvChunk = 32;     // reduction elements staged per step
constexpr int kConvLd = kConvChunk + 2;   // LDS row stride (floats): MFMA operand reads and the
                                          // staging stores are bank-conflict free at 34
constexpr int kConvMaxSplits = 256;  // weight gradient: workgroups along the n Ho Wo reduction
constexpr int kConvDwTarget = 1024;  // ... and the number of workgroups the split aims at (4 per CU:
                                     // the patch gather is latency bound at one wave per SIMD)

struct ConvGeom {
  int cin, h, w, cout, k, s, p;
  int ho, wo;
  int K;          // cin k k
  int P;          // ho wo
};

inline bool conv_geom_ok(int cin, int h, int w, int cout, int k, int s, int p) {
  if (k < 1 || k > 8 || s < 1 || s > 4 || s > k || p < 0 || p >= k) return false;
  if (cin < 1 || cin > 128 || cout < 1 || cout > 128 || h < 1 || w < 1) return false;
  if (h > (1 << 14) || w > (1 << 14)) return false;
  if (h + 2 * p < k || w + 2 * p < k) return false;          // Ho, Wo >= 1
  // one image's input and output index stay an int
  const int64_t ho = (h + 2 * p - k) / s + 1, wo = (w + 2 * p - k) / s + 1;
  if ((int64_t)cin * h * w > INT32_MAX || (int64_t)cout * ho * wo > INT32_MAX) return false;
  return true;
}

// (only for arguments conv_geom_ok accepts)
inline ConvGeom conv_geom(int cin, int h, int w, int cout, int k, int s, int p) {
  ConvGeom g{cin, h, w, cout, k, s, p, 0, 0, 0, 0};
  g.ho = (h + 2 * p - k) / s + 1;
  g.wo = (w + 2 * p - k) / s + 1;
  g.K = cin * k * k;
  g.P = g.ho * g.wo;
  return g;
}

inline int64_t conv_ceil(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- stride-parity classes of the input gradient
// positions i in [0, len) with (i + pad) % s == r:  i = first + s j, j in [0, count)
SMI_HD inline int conv_class_first(int r, int s, int p) { return ((r - p) % s + s) % s; }
SMI_HD inline int conv_class_count(int len, int r, int s, int p) {
  const int f = conv_class_first(r, s, p);
  return f >= len ? 0 : (len - f + s - 1) / s;
}
// taps of class r along one axis: k' = r + s j < k
SMI_HD inline int conv_class_taps(int k, int r, int s) { return r >= k ? 0 : (k - r + s - 1) / s; }

// ---- tiles
inline int64_t conv_fwd_tiles(const ConvGeom& g, int64_t n) {
  return conv_ceil(n * g.P, kConvTile) * conv_ceil(g.cout, kConvTile);
}
// pixel tiles of class (ry, rx); the grid's y dimension is the class
inline int64_t conv_dx_class_tiles(const ConvGeom& g, int64_t n, int ry, int rx) {
  const int64_t q = n * conv_class_count(g.h, ry, g.s, g.p) * conv_class_count(g.w, rx, g.s, g.p);
  return conv_ceil(q, kConvTile) * conv_ceil(g.cin, kConvTile);
}
inline int64_t conv_dx_max_tiles(const ConvGeom& g, int64_t n) {
  int64_t m = 0;
  for (int ry = 0; ry < g.s; ++ry)
    for (int rx = 0; rx < g.s; ++rx) {
      const int64_t t = conv_dx_class_tiles(g, n, ry, rx);
      m = t > m ? t : m;
    }
  return m;
}

// ---- weight gradient: the reduction over n Ho Wo in `chunks` steps of 32,
// `per` consecutive chunks per split, `splits` partial images in the scratch
struct ConvDwPlan {
  int tiles;          // 64 x 64 tiles of dW [cout][K]
  int64_t chunks;
  int64_t per;
  int splits;
  int64_t slab;       // floats of one partial: cout K (dW) + cout (db)
};

inline ConvDwPlan conv_dw_plan(const ConvGeom& g, int64_t n) {
  ConvDwPlan q{};
  q.tiles = (int)(conv_ceil(g.cout, kConvTile) * conv_ceil(g.K, kConvTile));
  q.chunks = conv_ceil(n * g.P, kConvChunk);
  q.slab = (int64_t)g.cout * g.K + g.cout;
  if (q.chunks < 1) { q.per = 0; q.splits = 0; return q; }
  int64_t want = conv_ceil(kConvDwTarget, q.tiles);
  if (want > kConvMaxSplits) want = kConvMaxSplits;
  if (want > q.chunks) want = q.chunks;
  if (want < 1) want = 1;
  q.per = conv_ceil(q.chunks, want);
  q.splits = (int)conv_ceil(q.chunks, q.per);      // no empty split
  return q;
}

inline int64_t conv_scratch_bytes(const ConvGeom& g, int64_t n) {
  const ConvDwPlan q = conv_dw_plan(g, n);
  return 4 * (int64_t)q.splits * q.slab;
}

// static LDS of every kernel: the A and B tiles
constexpr int conv_lds_bytes() { return 2 * kConvTile * kConvLd * 4; }

}  // namespace smi
