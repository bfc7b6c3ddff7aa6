// stem_plan.hpp — the pixel stem of free shape (CNNStemNetwork, builders.py:8-33,
// with model.conv_spec): n unpadded Conv2d(cout_i, k_i, stride_i) + ReLU layers,
// 1 <= n <= 4, then Flatten -> Linear(F) -> ReLU, on obs / 255.  Host-only
// arithmetic with no device or runtime call in it (tests/stem_plan_main.cpp
// sweeps it on the CPU under the sanitizers): the layers' geometry
// (conv_plan.hpp), the flat parameter layout, the activation layout, the
// backward's scratch carve, and which of the two implementations runs:
//   fused    cnn_kernels.hip, one workgroup per image, the reference's default
//            spec on the frames cnn_check and the LDS of a CU accept;
//   general  one conv_kernels.hip launch per layer and direction, every other
//            accepted spec and frame.
#pragma once
#include <stdint.h>
#include "smi_shapes.hpp"
#include "conv_plan.hpp"

namespace smi {

constexpr int kStemMaxLayers = 4;

struct StemSpec {
  int n;
  int cout[kStemMaxLayers], k[kStemMaxLayers], stride[kStemMaxLayers];
  int F;
};

inline StemSpec stem_spec_default(int F) { return StemSpec{2, {16, 32, 0, 0}, {8, 4, 0, 0}, {4, 2, 0, 0}, F}; }

inline StemSpec stem_spec(int n, const int* cout, const int* k, const int* stride, int F) {
  StemSpec s{};
  s.n = n; s.F = F;
  for (int i = 0; i < kStemMaxLayers && i < n; ++i) {
    s.cout[i] = cout ? cout[i] : 0; s.k[i] = k ? k[i] : 0; s.stride[i] = stride ? stride[i] : 0;
  }
  return s;
}

inline bool stem_is_default(const StemSpec& s) {
  return s.n == 2 && s.cout[0] == 16 && s.k[0] == 8 && s.stride[0] == 4 && s.cout[1] == 32 &&
         s.k[1] == 4 && s.stride[1] == 2;
}

// 0: accepted.  -1: the layer count or F; i + 1: layer i is outside the general
// kernel's ranges (conv_geom_ok without padding) or the frame it receives is
// smaller than its window
inline int stem_check(const StemSpec& s, int C, int H, int W) {
  if (s.n < 1 || s.n > kStemMaxLayers || s.F < 1) return -1;
  int c = C, h = H, w = W;
  for (int i = 0; i < s.n; ++i) {
    if (!conv_geom_ok(c, h, w, s.cout[i], s.k[i], s.stride[i], 0)) return i + 1;
    const ConvGeom g = conv_geom(c, h, w, s.cout[i], s.k[i], s.stride[i], 0);
    c = g.cout; h = g.ho; w = g.wo;
  }
  return 0;
}

// (only for arguments stem_check accepts)
struct StemPlan {
  int n, C, H, W, F;
  ConvGeom g[kStemMaxLayers];
  int64_t act[kStemMaxLayers];         // floats of one row of activation i: cout_i Ho_i Wo_i
  int64_t act_row;                     // their sum
  int64_t flat;                        // act[n - 1], the Linear layer's input width
  int64_t img;                         // bytes per uint8 image
  // flat parameter layout (floats), torch module order:
  // [conv_i.weight (cout_i, cin_i, k_i, k_i) | conv_i.bias] ..., [fc.weight (F, flat) | fc.bias]
  int64_t oW[kStemMaxLayers], ob[kStemMaxLayers], oWf, obf, total;
  int64_t nconv;                       // conv parameters = oWf
  bool fused;                          // the implementation a call runs (stem_fused_ok)
};

// the fused stem takes the spec and frame: the default layers on a frame that
// passes cnn_check and both LDS limits of cnn_kernels.hip
inline bool stem_fused_ok(const StemSpec& s, int C, int H, int W) {
  if (!stem_is_default(s) || H < 1 || W < 1 || C < 1 || C > 128 || H > (1 << 14) || W > (1 << 14))
    return false;
  const CnnGeom g = cnn_geom(C, H, W, s.F);
  return cnn_check_msg(g) == nullptr && cnn_fwd_lds(g) <= kCuLdsBytes && cnn_bwd_lds(g) <= kCuLdsBytes;
}

inline StemPlan stem_plan(const StemSpec& s, int C, int H, int W) {
  StemPlan p{};
  p.n = s.n; p.C = C; p.H = H; p.W = W; p.F = s.F;
  p.img = (int64_t)C * H * W;
  int c = C, h = H, w = W;
  int64_t o = 0;
  for (int i = 0; i < s.n; ++i) {
    p.g[i] = conv_geom(c, h, w, s.cout[i], s.k[i], s.stride[i], 0);
    p.act[i] = (int64_t)p.g[i].cout * p.g[i].P;
    p.act_row += p.act[i];
    p.oW[i] = o; o += (int64_t)p.g[i].cout * p.g[i].K;
    p.ob[i] = o; o += p.g[i].cout;
    c = p.g[i].cout; h = p.g[i].ho; w = p.g[i].wo;
  }
  p.flat = p.act[s.n - 1];
  p.nconv = p.oWf = o; o += (int64_t)s.F * p.flat;
  p.obf = o; o += s.F;
  p.total = o;
  p.fused = stem_fused_ok(s, C, H, W);
  return p;
}

// ---- activations: layer i is [rows][act[i]], the layers one behind the other
inline int64_t stem_act_off(const StemPlan& p, int64_t rows, int i) {
  int64_t o = 0;
  for (int j = 0; j < i; ++j) o += rows * p.act[j];
  return o;
}
inline int64_t stem_act_floats(const StemPlan& p, int64_t rows) { return rows * p.act_row; }

// ---- the backward's scratch (floats): one gradient image per activation that
// has a producer, dA_n first, then the weight-gradient partials.  General
// form: every dA_i, and ONE partial region of the largest layer's size (the
// layers' weight gradients run one after another).  Fused form: dA_n (dA2) and
// cnn_bwd_grid(rows) slabs of the conv parameters, the carve of smi_cnn_backward.
struct StemScratch {
  int64_t dA[kStemMaxLayers];          // offset of dA_{i+1}; -1: the form has no such image
  int64_t part, part_floats;
  int64_t total;
};
inline int64_t stem_part_floats(const StemPlan& p, int64_t rows) {
  if (p.fused) return (int64_t)cnn_bwd_grid(rows) * p.nconv;
  int64_t m = 0;
  for (int i = 0; i < p.n; ++i) {
    const int64_t b = conv_scratch_bytes(p.g[i], rows) / 4;
    m = b > m ? b : m;
  }
  return m;
}
inline StemScratch stem_scratch(const StemPlan& p, int64_t rows) {
  StemScratch s{};
  int64_t o = 0;
  for (int i = 0; i < kStemMaxLayers; ++i) s.dA[i] = -1;
  for (int i = p.n - 1; i >= 0; --i) {
    if (p.fused && i != p.n - 1) continue;
    s.dA[i] = o;
    o += rows * p.act[i];
  }
  s.part = o;
  s.part_floats = stem_part_floats(p, rows);
  s.total = o + s.part_floats;
  return s;
}
// a forward without an activation buffer keeps its intermediates in scratch:
// the fused form A_n alone (A1 stays in LDS), the general form every layer
inline int64_t stem_fwd_scratch_floats(const StemPlan& p, int64_t rows) {
  return p.fused ? rows * p.flat : stem_act_floats(p, rows);
}
// what one scratch buffer needs to serve either call
inline int64_t stem_scratch_bytes(const StemPlan& p, int64_t rows) {
  const int64_t b = stem_scratch(p, rows).total, f = stem_fwd_scratch_floats(p, rows);
  return 4 * (b > f ? b : f);
}

}  // namespace smi
