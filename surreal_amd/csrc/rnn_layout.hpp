// rnn_layout.hpp — the LSTM learner's shapes (RnnDims) and its scratch carve
// (RnnScratch) for ppo_rnn.hip: host-only arithmetic, no HIP headers and no
// runtime calls, so tests/rnn_layout_main.cpp sweeps it on the CPU.
#pragma once
#include "smi_shapes.hpp"
#include "stem_plan.hpp"

namespace smi {

struct RnnDims {
  int B, T, Hz, E, S1, D, H, G4, A, h1, h2, c1, c2;
  int L;                              // LSTM layers (nn.LSTM num_layers = rnn_layer)
  int64_t nL0, nLk;                   // parameters of layer 0 / of each layer above it
  int F, Din;                         // pixel features (0: no CNN stem), LSTM input D + F
  int Hin;                            // head input width: H (LSTM) or Din (H == 0: MLP policy)
  int ldx;                            // row stride of the stem input Xz / Xr: Din rounded up to
                                      // 4 (16-byte rows; the padding columns stay zero)
  int Hld;                            // row stride of the head input: H, or ldx (MLP policy)
  int64_t NE, NG;
  int64_t nA_head, nC_head, nL, nCnn, nS;   // parameter counts; stem = [lstm | cnn]
  MlpLayout LA, LC;
  CnnGeom G;
  // the stem behind G (the reference's default layers, ppo_net.py:139 passes
  // none) and the implementation it runs on this camera: the fused kernels, or
  // the general layers (stem_plan.hpp); px_ok: a stem the library accepts
  StemPlan SP;
  bool px_ok, px_fused;
};

inline RnnDims rnn_dims(int B, int T, int Hz, int D, int H, int h1, int h2, int A, int c1, int c2,
                        int pc = 0, int ph = 0, int pw = 0, int F = 0, int L = 1) {
  RnnDims d;
  d.L = L > 1 ? L : 1;
  d.F = F > 0 ? F : 0; d.Din = D + d.F;
  d.G = cnn_geom(pc, ph, pw, d.F);
  d.nCnn = d.F > 0 ? d.G.total : 0;
  d.SP = StemPlan{};
  d.px_ok = d.F > 0 && stem_check(stem_spec_default(d.F), pc, ph, pw) == 0;
  if (d.px_ok) d.SP = stem_plan(stem_spec_default(d.F), pc, ph, pw);
  d.px_fused = d.px_ok && d.SP.fused;
  d.B = B; d.T = T; d.Hz = Hz; d.E = T - Hz + 1; d.S1 = T + 1; d.D = D; d.H = H; d.G4 = 4 * H;
  d.A = A; d.h1 = h1; d.h2 = h2; d.c1 = c1; d.c2 = c2;
  d.NE = (int64_t)d.E * B; d.NG = (int64_t)d.S1 * B;
  d.Hin = H > 0 ? H : d.Din;
  d.ldx = (d.Din + 3) & ~3;
  d.Hld = H > 0 ? H : d.ldx;
  d.LA = mlp_layout(d.Hin, h1, h2, A, 1);
  d.LC = mlp_layout(d.Hin, c1, c2, 1, 0);
  d.nA_head = d.LA.fcount; d.nC_head = d.LC.fcount;
  // nn.LSTM parameter order per layer: W_ih, W_hh, b_ih, b_hh (layer k >= 1 reads
  // layer k-1's h, so its W_ih is 4H x H)
  d.nL0 = H > 0 ? (int64_t)4 * H * d.Din + (int64_t)4 * H * H + 8 * (int64_t)H : 0;
  d.nLk = H > 0 ? (int64_t)8 * H * H + 8 * (int64_t)H : 0;
  d.nL = d.nL0 + (d.L - 1) * d.nLk;
  d.nS = d.nL + d.nCnn;
  return d;
}

// scratch carve (floats, 64-float aligned regions)
struct RnnScratch {
  float *Xz, *Xr, *xproj, *hbuf, *cbuf, *gates, *HA1, *HA2, *OUT, *dOUT, *dH1, *dH2, *dh, *dgates;
  // the PREP phase's own copies (it may run on a second stream beside GAE)
  float *xprojR, *hbufR, *HA1R, *HA2R, *A2R;
  // W1^T | W2^T of the head a phase's fused forward wrote for its backward
  float *wT;
  float *values, *adv, *ret, *refmu, *lvpart;
  // time-major per-row inputs of the row kernels, packed once per learn,
  // field-major within blocks of 64 rows: rowin[rin_idx(W, n, f)], f =
  // {actions (A) | behave mu, sigma (2A) | raw advantage | behaviour
  // likelihood | KL(ref || behaviour) row term}, n = t*B + b;
  // ret_tm[n] the window return
  float *rowin, *ret_tm;
  float *A1, *A2, *dA2, *dF, *cpart;        // pixel stem (empty without one)
  // the general stem's own regions (empty where the fused one runs): its
  // forward keeps A1 in memory (the PREP phase's copy) and its backward dA1
  float *A1R, *dA1;
  double *part, *gaepart;
  int* ci; float* cf;
  // the transposed image of LSTM layer 0's weights, [W_ihT [Din][4H] | W_hhT [H][4H]
  // | 4H zeros] (one-layer stems with H <= 128: the r4 forward loads its
  // columns from it; written by the GAE phase and kept current by both Adam
  // applies).  It lives in the tail of xproj: that region holds S1 steps for the
  // GAE pass, which is done with them before it writes the image, and every
  // later forward of the learn runs E < S1 steps (PREP has xprojR), so rows
  // [E B, S1 B) stay idle.  The carve's total does not change.  Empty
  // (wimg_off == -1) when the shape has no image or the tail cannot hold it.
  float* wimg;
  int64_t wimg_off;
  int64_t total_floats;
};

inline int64_t al64(int64_t n) { return (n + 63) & ~(int64_t)63; }
// floats of the weight image; 0: the shape has none
inline int64_t wimg_floats(const RnnDims& d) {
  return d.L == 1 && d.H >= 1 && d.H <= 128 ? (int64_t)d.G4 * (d.Din + d.H + 1) : 0;
}
// its float offset inside xproj (past the E steps an epoch forward writes, on a
// 64-float boundary), or -1
inline int64_t wimg_in_xproj(const RnnDims& d) {
  const int64_t n = wimg_floats(d), at = al64(d.NE * d.G4);
  return n > 0 && at + n <= d.NG * d.G4 ? at : -1;
}
// doubles of s.part: 65536, or the value statistics' five per head workgroup
inline int64_t part_doubles(const RnnDims& d) {
  const int64_t v = 5 * (int64_t)head_bwd_blocks(d.NE);
  return v > 65536 ? v : 65536;
}
inline RnnScratch rnn_scratch(const RnnDims& d, void* base) {
  RnnScratch s{};
  float* p = static_cast<float*>(base);
  int64_t o = 0;
  auto take = [&](int64_t n) { float* r = p ? p + o : nullptr; o += al64(n); return r; };
  const int hmax1 = d.h1 > d.c1 ? d.h1 : d.c1, hmax2 = d.h2 > d.c2 ? d.h2 : d.c2;
  s.Xz = take(d.NG * d.ldx);
  s.Xr = take(d.NE * d.ldx);
  s.wimg_off = wimg_in_xproj(d) >= 0 ? o + wimg_in_xproj(d) : -1;
  s.xproj = take(d.NG * d.G4);
  s.wimg = s.xproj && s.wimg_off >= 0 ? p + s.wimg_off : nullptr;
  s.hbuf = take((int64_t)d.L * (d.S1 + 1) * d.B * d.H);     // per layer (see hbuf_of)
  s.cbuf = take((int64_t)d.L * (d.E + 1) * d.B * d.H);
  s.gates = take((int64_t)d.L * d.NE * d.G4);
  s.HA1 = take(d.NG * hmax1);
  s.HA2 = take(d.NG * hmax2);
  s.OUT = take(d.NG * (d.A > 1 ? d.A : 1));
  s.dOUT = take(d.NE * (d.A > 1 ? d.A : 1));
  s.dH1 = take(d.NE * hmax1);
  s.dH2 = take(d.NE * hmax2);
  s.dh = take(d.NE * d.H);
  s.dgates = take((int64_t)d.L * d.NE * d.G4);
  s.values = take((int64_t)d.B * d.S1);
  s.adv = take(d.NE);
  s.ret = take(d.NE);
  s.refmu = take(d.NE * d.A);
  s.rowin = take(((d.NE + 63) & ~(int64_t)63) * row_w(d.A));
  s.ret_tm = take(d.NE);
  s.lvpart = take((int64_t)4096 * d.A);
  const bool px = d.F > 0;
  // general stem: also the S1-step forward of the GAE pass writes A1
  const bool gen = px && d.px_ok && !d.px_fused;
  s.A1 = take(px ? (gen ? d.NG : d.NE) * 16 * d.G.P1 : 0);
  s.A2 = take(px ? d.NG * d.G.flat : 0);
  s.xprojR = take(d.NE * d.G4);
  s.hbufR = take((int64_t)d.L * (d.S1 + 1) * d.B * d.H);
  s.HA1R = take(d.NE * hmax1);
  s.HA2R = take(d.NE * hmax2);
  s.A2R = take(px ? d.NE * d.G.flat : 0);
  s.A1R = take(gen ? d.NE * 16 * d.G.P1 : 0);
  {
    const int64_t wa = (int64_t)d.Hin * d.h1 + (int64_t)d.h1 * d.h2;
    const int64_t wc = (int64_t)d.Hin * d.c1 + (int64_t)d.c1 * d.c2;
    s.wT = take(wa > wc ? wa : wc);
  }
  s.dA2 = take(px ? d.NE * d.G.flat : 0);
  s.dF = take(px ? d.NE * d.F : 0);
  s.dA1 = take(gen ? d.NE * 16 * d.G.P1 : 0);
  // conv weight-gradient partials: the fused backward's slabs, or the general
  // layers' shared region (stem_part_floats)
  s.cpart = take(px ? (gen ? stem_part_floats(d.SP, d.NE) : (int64_t)cnn_bwd_grid(d.NE) * d.G.nconv) : 0);
  s.part = reinterpret_cast<double*>(take(2 * part_doubles(d)));   // >= 65536 doubles
  s.gaepart = reinterpret_cast<double*>(take(2 * 2 * 2048));
  s.ci = reinterpret_cast<int*>(take(CI_COUNT));
  s.cf = take(CF_COUNT);
  s.total_floats = o;
  return s;
}

// per-layer regions of the LSTM buffers
inline float* hbuf_of(const RnnDims& d, const RnnScratch& s, int l) {
  return s.hbuf + (int64_t)l * (d.S1 + 1) * d.B * d.H;
}
inline float* cbuf_of(const RnnDims& d, const RnnScratch& s, int l) {
  return s.cbuf + (int64_t)l * (d.E + 1) * d.B * d.H;
}
inline float* gates_of(const RnnDims& d, const RnnScratch& s, int l) {
  return s.gates + (int64_t)l * d.NE * d.G4;
}
inline float* dgates_of(const RnnDims& d, const RnnScratch& s, int l) {
  return s.dgates + (int64_t)l * d.NE * d.G4;
}

struct LstmP { const float *Wih, *Whh, *bih, *bhh; };
inline LstmP lstm_params(const float* p, int D, int H) {
  LstmP l;
  l.Wih = p;
  l.Whh = p + (int64_t)4 * H * D;
  l.bih = l.Whh + (int64_t)4 * H * H;
  l.bhh = l.bih + 4 * H;
  return l;
}
// layer l of a stem buffer [layer 0 (in Din) | layer 1 (in H) | ...]
inline LstmP lstm_layer(const RnnDims& d, const float* p, int l) {
  return l == 0 ? lstm_params(p, d.Din, d.H)
                : lstm_params(p + d.nL0 + (int64_t)(l - 1) * d.nLk, d.H, d.H);
}

}  // namespace smi
