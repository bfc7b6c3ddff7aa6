// smi_shapes.hpp — shape arithmetic shared by the kernels, their launchers and
// the host-only layout code (rnn_layout.hpp): parameter layouts, the pixel
// stem's geometry, the packed policy row, and the grids whose size a scratch
// region depends on.  Plain C++17: compiles without the HIP headers (SMI_HD is
// empty outside hipcc), so every formula here has this one definition.
#pragma once
#include <stdint.h>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SMI_HD __host__ __device__
#else
#define SMI_HD
#endif

namespace smi {

// LDS leading dimension for a K-wide row: >= roundup(K,4) and == 2 (mod 32), so
// the A-operand column reads of a 32-lane half (16 rows at k, 16 rows at k+1)
// land on 32 distinct banks.
SMI_HD inline int pad_ld(int k) {
  const int k4 = (k + 3) & ~3;
  const int r = (k4 - 2) & 31;
  return k4 + (32 - r);
}
SMI_HD inline int round4(int k) { return (k + 3) & ~3; }

// ------------------------------------------------------------ MLP layouts
// Flat (global, torch) layout and padded (LDS) layout of a 3-layer MLP
// in -> h1 -> h2 -> out [+ log_var(out)].
struct MlpLayout {
  int in, h1, h2, out, lv;
  // flat offsets
  int fW1, fb1, fW2, fb2, fW3, fb3, flv, fcount;
  // padded LDS offsets and leading dims
  int ld1, ld2, ld3;
  int pW1, pb1, pW2, pb2, pW3, pb3, plv, pcount;
};

SMI_HD inline MlpLayout mlp_layout(int in, int h1, int h2, int out, int lv) {
  MlpLayout L;
  L.in = in; L.h1 = h1; L.h2 = h2; L.out = out; L.lv = lv;
  L.fW1 = 0;
  L.fb1 = L.fW1 + h1 * in;
  L.fW2 = L.fb1 + h1;
  L.fb2 = L.fW2 + h2 * h1;
  L.fW3 = L.fb2 + h2;
  L.fb3 = L.fW3 + out * h2;
  L.flv = L.fb3 + out;
  L.fcount = L.flv + (lv ? out : 0);
  L.ld1 = pad_ld(in); L.ld2 = pad_ld(h1); L.ld3 = pad_ld(h2);
  L.pW1 = 0;
  L.pb1 = L.pW1 + h1 * L.ld1;
  L.pW2 = round4(L.pb1 + h1);
  L.pb2 = L.pW2 + h2 * L.ld2;
  L.pW3 = round4(L.pb2 + h2);
  L.pb3 = L.pW3 + out * L.ld3;
  L.plv = round4(L.pb3 + out);
  L.pcount = round4(L.plv + (lv ? out : 0));
  return L;
}

// ---- pixel stem (CNNStemNetwork, builders.py:8-33) -------------------------
// Flat parameter layout (torch Conv2d / Linear shapes, in module order):
// [conv1.weight (16,C,8,8) | conv1.bias (16) | conv2.weight (32,16,4,4) |
//  conv2.bias (32) | fc.weight (F, 32*H2*W2) | fc.bias (F)]
struct CnnGeom {
  int C, H, W, H1, W1, P1, H2, W2, P2, K1, flat, F;
  int64_t img;                                  // bytes per uint8 image
  int64_t oW1, ob1, oW2, ob2, oWf, obf, total;  // offsets (floats)
  int64_t nconv;                                // conv parameters = oWf
};
SMI_HD inline CnnGeom cnn_geom(int C, int H, int W, int F) {
  CnnGeom g;
  g.C = C; g.H = H; g.W = W; g.F = F;
  g.H1 = (H - 8) / 4 + 1; g.W1 = (W - 8) / 4 + 1; g.P1 = g.H1 * g.W1;
  g.H2 = (g.H1 - 4) / 2 + 1; g.W2 = (g.W1 - 4) / 2 + 1; g.P2 = g.H2 * g.W2;
  g.K1 = 64 * C; g.flat = 32 * g.P2;
  g.img = (int64_t)C * H * W;
  g.oW1 = 0; g.ob1 = 16 * (int64_t)g.K1; g.oW2 = g.ob1 + 16; g.ob2 = g.oW2 + 32 * 256;
  g.oWf = g.ob2 + 32; g.obf = g.oWf + (int64_t)F * g.flat; g.total = g.obf + F;
  g.nconv = g.oWf;
  return g;
}
constexpr int kCnnPartials = 512;               // max workgroups (partial slabs) of the backward
inline int cnn_bwd_grid(int64_t rows) { return (int)(rows < kCnnPartials ? rows : kCnnPartials); }

// ---- fused head chains (head_kernels.hip) ----------------------------------
constexpr int HC_R = 16;                 // rows per workgroup
// row tiles per workgroup: 2 (32 rows: the weight chunks feed twice the MFMAs)
// once the batch leaves at least ~2 workgroups per CU of them, else 1
inline int hc_rt(int64_t rows) { return rows >= 16384 ? 2 : 1; }
// workgroups of a fused head launch over rows (the policy prologue writes one
// log_var partial per workgroup)
inline int head_bwd_blocks(int64_t rows) {
  const int R = HC_R * hc_rt(rows);
  return (int)((rows + R - 1) / R);
}

// ---- policy rows (pol_rows.hpp) ---------------------------------------------
// device control block (int / float scratch)
enum { CI_STOP = 0, CI_RUNS, CI_NG, CI_NP, CI_COUNT = 8 };
enum { CF_KLCOEF = 0, CF_SURRW, CF_COUNT = 8 };

// fields of a packed row: A actions, 2A behaviour parameters, the advantage,
// then the row's behaviour-policy terms, fixed for the whole learn() (the
// behaviour parameters and the reference policy do not change across epochs):
// the clamped behaviour likelihood and the row's KL(ref || behaviour) term,
// computed once by row_pack_kernel instead of in every epoch's row passes
SMI_HD inline int row_w(int A) { return 3 * A + 3; }

}  // namespace smi
