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
constexpr int kCnnThreads = 256;                // threads of a stem workgroup (== kWG)
// what the fused kernels (cnn_kernels.hip) ask of a frame: nullptr, or the
// reason they refuse it
inline const char* cnn_check_msg(const CnnGeom& g) {
  if (g.C != 3 && g.C != 9) return "cnn: 3 (one RGB frame) or 9 (three stacked RGB frames) channels";
  if (g.H1 < 4 || g.W1 < 4 || g.H2 < 1 || g.W2 < 1) return "cnn: image smaller than the two convolutions";
  if ((g.P2 + 15) / 16 > 6) return "cnn: conv-2 output larger than 96 pixels (84x84 gives 81)";
  if (g.W % 4 != 0 || g.img % 16 != 0 || g.P1 % 4 != 0 || g.W1 % 2 != 0 || g.flat % 4 != 0)
    return "cnn: need W % 4 == 0, C*H*W % 16 == 0, even conv-1 width, "
           "conv-1 pixels % 4 == 0 (84x84 qualifies)";
  if (g.F < 1) return "cnn: feature dim must be >= 1";
  return nullptr;
}
// dynamic LDS of the fused forward / backward: the 16-byte-aligned image and A1;
// + dA2, the reduction space and the two pixel-offset tables
SMI_HD inline int64_t lds_img_bytes(const CnnGeom& g) { return (g.img + 15) & ~(int64_t)15; }
inline int64_t cnn_fwd_lds(const CnnGeom& g) { return lds_img_bytes(g) + (int64_t)64 * g.P1; }
inline int64_t cnn_bwd_lds(const CnnGeom& g) {
  return lds_img_bytes(g) + (int64_t)64 * g.P1 + 4 * (int64_t)round4(g.flat) + 4 * kCnnThreads +
         4 * (int64_t)(g.P1 + g.P2);
}
// per-thread 16-byte chunk counts of an 84 x 84 frame's staging (image, A1,
// dA2), register arrays of the forward's batched image loads and the
// backward's next-image prefetch (larger frames: a tail loop / prefetch off)
template <int C> struct CnnPf {
  static constexpr int KI = C <= 3 ? 6 : 16;     // uint4 of the uint8 image
  static constexpr int KA = 7;                   // float4 of A1 (16 x P1)
  static constexpr int KD = 3;                   // float4 of dA2 (flat)
};
// the backward form: next-image prefetch when the frame's image, A1 and dA2
// fit the prefetch register arrays (84 x 84 does, for 3 and 9 channels), else
// the form that stages each image after the previous one's last pass
inline bool cnn_bwd_prefetch(const CnnGeom& g, int C) {
  const int ki = C == 9 ? CnnPf<9>::KI : CnnPf<3>::KI, ka = C == 9 ? CnnPf<9>::KA : CnnPf<3>::KA,
            kd = C == 9 ? CnnPf<9>::KD : CnnPf<3>::KD;
  return (g.img >> 4) <= (int64_t)ki * kCnnThreads && 4 * g.P1 <= ka * kCnnThreads &&
         (g.flat >> 2) <= kd * kCnnThreads;
}

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
// LDS leading dim of a K-wide activation tile: K rounded up to the 16-k chunk,
// + 4 (an odd multiple of 4 floats: the 16 rows of a chunk read land on 16
// distinct 16-byte bank groups)
SMI_HD inline int hc_ld(int k) { return ((k + 15) & ~15) + 4; }
constexpr int HC_SR = 32 * 33 + 32;     // last-layer partials (1024) / a transpose tile (1056)
// LDS floats of the forward's last-layer partials / transpose tile
SMI_HD constexpr int hc_sr(int RT) { return RT * 1024 > HC_SR ? RT * 1024 : HC_SR; }
// 16-column tiles per wave of an n-wide layer, rounded to an instantiation
inline int hc_nt(int n) {
  const int t = (((n + 15) >> 4) + 3) >> 2;
  return t <= 2 ? 2 : t <= 4 ? t : t <= 5 ? 5 : 8;     // 2, 3, 4, 5, 8
}
constexpr int kCuLdsBytes = 160 * 1024;  // LDS of one CU
constexpr int kCuWgSlots = 8;            // 8 waves per SIMD: 8 four-wave workgroups per CU
constexpr int HC_PG_LDS = 1024;          // bound of the policy prologue's static LDS (PolGradShared)

// The launch shape of the two fused chains over `rows` rows of an
// in -> h1 -> h2 head (dX over dxn input columns): the one place that decides
// the row tiles per workgroup, the kernel forms, the LDS carve and the grid.
// Offsets are in floats from the start of the dynamic LDS.
//   forward:  X [R][ld0] and HA2 [R][ld2] at 0, HA1 [R][ld1] at fwd_o1, the
//             partials / transpose tile at fwd_oR;
//   backward: dH2 [R][ld2], dH1 [R][ld1], dZ [R][16], one behind the other.
// Forward, separate carve: HA1 has LDS of its own beside the X / HA2 region.
// Shared carve (two row tiles only): X, HA1 and HA2 take their turns in ONE
// region of the widest tile's size (fwd_o1 == 0), at the price of a barrier
// between a layer's k loop and its epilogue.  It is chosen only where the
// smaller carve lets more workgroups onto a CU: at the C3 widths 100 -> 300 ->
// 200 and 32 rows, 74,752 -> 47,616 B, two -> three per CU, so the 672
// workgroups of 21,504 rows are one resident round of the 256 CUs (62 -> 59
// us per launch).  The backward keeps dH2 and dH1 apart: sharing them, with
// the register cuts three per CU need, measured no faster (DESIGN.md section
// 9).  *_wgs is what the LDS carve allows (the backward's with the policy
// prologue's static LDS); registers may hold a form below it (the forward's
// 8-tile forms and the two-row-tile backward: two per CU).
struct HeadPlan {
  int rt, grid;                          // row tiles per workgroup, workgroups
  int ld0, ld1, ld2;                     // LDS leading dims of the in / h1 / h2 wide tiles
  int fwd_n1, fwd_n2, bwd_na, bwd_nb;    // tiles per wave of the instantiation launched
  int fwd_shared;                        // forward: the shared carve
  int fwd_o1, fwd_oR;
  int fwd_lds, bwd_lds;                  // dynamic LDS bytes
  int fwd_wgs, bwd_wgs;                  // workgroups per CU
};
inline int hc_wgs(int lds_bytes) {
  const int n = kCuLdsBytes / lds_bytes;
  return n < kCuWgSlots ? n : kCuWgSlots;
}
inline HeadPlan head_plan(int64_t rows, int in, int h1, int h2, int dxn) {
  HeadPlan p;
  p.rt = hc_rt(rows);
  p.grid = head_bwd_blocks(rows);
  p.ld0 = hc_ld(in); p.ld1 = hc_ld(h1); p.ld2 = hc_ld(h2);
  const int n1 = hc_nt(h1), nb = hc_nt(dxn > 0 ? dxn : 1);
  // forward: layer-1 slots {2, 5, 8} x layer-2 slots {2, 3, 4, 5, 8} (C3 / C5:
  // 300 x 200 -> 5, 4); backward: {2, 5, 8} x {2, 5}
  p.fwd_n1 = p.bwd_na = n1 <= 2 ? 2 : n1 <= 5 ? 5 : 8;
  p.fwd_n2 = hc_nt(h2);
  p.bwd_nb = nb <= 2 ? 2 : 5;
  const int R = HC_R * p.rt;
  const int w02 = p.ld0 > p.ld2 ? p.ld0 : p.ld2;
  const int w012 = w02 > p.ld1 ? w02 : p.ld1;
  const int fsep = (R * (w02 + p.ld1) + hc_sr(p.rt)) * 4, fsh = (R * w012 + hc_sr(p.rt)) * 4;
  p.fwd_shared = p.rt == 2 && hc_wgs(fsh) > hc_wgs(fsep);
  p.fwd_o1 = p.fwd_shared ? 0 : R * w02;
  p.fwd_oR = p.fwd_shared ? R * w012 : R * (w02 + p.ld1);
  p.fwd_lds = p.fwd_shared ? fsh : fsep;
  p.bwd_lds = (R * (p.ld2 + p.ld1) + R * 16) * 4;
  p.fwd_wgs = hc_wgs(p.fwd_lds);
  p.bwd_wgs = hc_wgs(p.bwd_lds + HC_PG_LDS);
  return p;
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
