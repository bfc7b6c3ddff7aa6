// ppo_rnn.hip — PPOLearner._optimize with the LSTM policy (if_rnn_policy;
// surreal/learner/ppo.py:487-586 and the RNN branch of _gae_and_return,
// ppo.py:389-406) as a fixed sequence of device phases (see surreal_mi.h).
//
// Rows of every activation are time-major, n = t*B + b (t < S), so the LSTM
// input projection, the heads and all weight gradients are plain GEMMs over
// contiguous matrices; per-row loss kernels map n back to the batch-major
// inputs.  Data-dependent control (KL early stop, adapt penalty branch) is a
// device flag that turns later phases into no-ops: the host issues the same
// launches on every call and every rank, and never waits for the device.
//
// This unit is the host sequencing only: shapes and the scratch carve are
// rnn_layout.hpp, the learner's own kernels and their launchers
// ppo_rnn_kernels.hip (rnn_kernels.hpp).
#include "smi_device.hpp"
#include "smi_internal.hpp"
#include "dw_plan.hpp"
#include "pol_rows.hpp"
#include "lstm_cell.hpp"
#include "rnn_layout.hpp"
#include "rnn_kernels.hpp"

namespace smi {

struct Head {   // one MLP head over rows of an activation matrix
  const float* P; MlpLayout L; int in, h1, h2, out, tanh_out;
};

static bool head_fused(const Head& h, const float* X, int64_t ldx) {
  return head_fused_ok(h.in, ldx, h.h1, h.h2, h.out, X, h.P + h.L.fW1, h.P + h.L.fW2,
                       h.P + h.L.fW3);
}

// what a head forward does beside Y (every field optional)
struct HeadFwdOpts {
  const int* skip = nullptr;    // device stop flag
  float* wT = nullptr;          // the fused launch also writes W1^T | W2^T here, for a
                                // fused backward of the same parameters
  bool keep_act = true;         // false: no backward follows, HA1 / HA2 need not be kept
  // the value-loss gradient written by the fused forward (out == 1), and with
  // vpart its value statistics' partials; *vdone tells whether it was (the
  // layer-GEMM path does not)
  const float* vret = nullptr;
  float* vgrad = nullptr;
  float vscale = 0.f;
  double* vpart = nullptr;
  bool* vdone = nullptr;
};

// forward: X[rows][ldx] -> HA1 -> HA2 -> Y ([rows][out]); one fused launch
// (head_kernels.hip) when the shapes allow
static int head_fwd(const Head& h, const float* X, int64_t ldx, int64_t rows, float* HA1,
                    float* HA2, float* Y, hipStream_t st, const HeadFwdOpts& o) {
  const MlpLayout& L = h.L;
  if (o.vdone) *o.vdone = false;
  if (head_fused(h, X, ldx)) {
    // keep_act false: no backward follows (the GAE critic pass, PREP's
    // reference forward, the KL check after the last policy update), so the
    // fused chain skips the HA1 / HA2 copy-outs (the layer-GEMM path below
    // needs them as its intermediates)
    if (!o.keep_act) HA1 = HA2 = nullptr;
    const bool ve = o.vgrad && h.out == 1;
    if (o.vdone) *o.vdone = ve;
    return launch_head_fwd_fused(X, ldx, rows, h.in, h.P + L.fW1, h.P + L.fb1, h.h1, h.P + L.fW2,
                                 h.P + L.fb2, h.h2, h.P + L.fW3, h.P + L.fb3, h.out, h.tanh_out,
                                 HA1, HA2, Y, h.out, o.wT,
                                 o.wT ? o.wT + (int64_t)h.in * h.h1 : nullptr, st, o.skip,
                                 ve ? o.vret : nullptr, ve ? o.vgrad : nullptr, o.vscale,
                                 ve ? o.vpart : nullptr);
  }
  const int M = (int)rows;
  RC_CHECK(launch_linear_fwd(X, ldx, M, h.in, h.P + h.L.fW1, h.in, h.P + h.L.fb1, h.h1, ACT_RELU,
                             HA1, h.h1, st, o.skip));
  RC_CHECK(launch_linear_fwd(HA1, h.h1, M, h.h1, h.P + h.L.fW2, h.h1, h.P + h.L.fb2, h.h2,
                             ACT_RELU, HA2, h.h2, st, o.skip));
  return launch_linear_fwd(HA2, h.h2, M, h.h2, h.P + h.L.fW3, h.h2, h.P + h.L.fb3, h.out,
                           h.tanh_out ? ACT_TANH : ACT_NONE, Y, h.out, st, o.skip);
}

struct HeadBwdOpts {
  const float* wT = nullptr;        // W1^T | W2^T of the fused forward: the fused chain may run
  const PolRowArgs* pg = nullptr;   // the policy-gradient prologue (dZ computed from the policy
                                    // rows by the fused chain itself); only on the fused path
};

// backward from dZ (gradient at the last layer's pre-activation) into the flat
// gradient image G (same layout as P); input-gradient columns [dx0, dx0+dxn)
// to dXout ([rows][dxn], masked by dxmask > 0 when given; dxn == 0: none).
// Inside a dW group (stem_backward) the weight gradients are queued and run
// as one grouped launch at the flush.
static int head_bwd(const Head& h, const float* dZ, const float* X, int64_t ldx, int64_t rows,
                    const float* HA1, const float* HA2, float* dH1, float* dH2, float* G,
                    int dx0, int dxn, const float* dxmask, int64_t ldm, float* dXout,
                    hipStream_t st, const int* skip, const HeadBwdOpts& o) {
  const int M = (int)rows;
  const MlpLayout& L = h.L;
  const float* wT = o.wT;
  if (wT && dxn <= 320 && head_fused(h, X, ldx)) {
    // the input-gradient chain in one launch (dH2, dH1, dX), then the three
    // weight gradients (queued into the phase's dW group when one is open)
    RC_CHECK(launch_head_bwd_fused(dZ, h.out, rows, h.P + L.fW3, wT + (int64_t)h.in * h.h1, wT,
                                   h.h1, h.h2, dx0, dxn, HA1, HA2, dH2, dH1, dXout, dxn, dxmask,
                                   ldm, st, skip, o.pg));
    RC_CHECK(launch_linear_bwd_dw(dZ, h.out, M, h.out, HA2, h.h2, h.h2, G + L.fW3, h.h2,
                                  G + L.fb3, 0, st, skip));
    RC_CHECK(launch_linear_bwd_dw(dH2, h.h2, M, h.h2, HA1, h.h1, h.h1, G + L.fW2, h.h1,
                                  G + L.fb2, 0, st, skip));
    return launch_linear_bwd_dw(dH1, h.h1, M, h.h1, X, ldx, h.in, G + L.fW1, h.in, G + L.fb1, 0,
                                st, skip);
  }
  if (o.pg) return set_error(SMI_E_ARG, "head_backward: the policy prologue needs the fused chain");
  RC_CHECK(launch_linear_bwd_dw(dZ, h.out, M, h.out, HA2, h.h2, h.h2, G + L.fW3, h.h2, G + L.fb3,
                                0, st, skip));
  RC_CHECK(launch_linear_bwd_dx(dZ, h.out, M, h.out, h.P + L.fW3, h.h2, h.h2, HA2, h.h2, dH2,
                                h.h2, st, skip));
  RC_CHECK(launch_linear_bwd_dw(dH2, h.h2, M, h.h2, HA1, h.h1, h.h1, G + L.fW2, h.h1, G + L.fb2,
                                0, st, skip));
  RC_CHECK(launch_linear_bwd_dx(dH2, h.h2, M, h.h2, h.P + L.fW2, h.h1, h.h1, HA1, h.h1, dH1,
                                h.h1, st, skip));
  RC_CHECK(launch_linear_bwd_dw(dH1, h.h1, M, h.h1, X, ldx, h.in, G + L.fW1, h.in, G + L.fb1, 0,
                                st, skip));
  if (dxn <= 0) return SMI_OK;
  return launch_linear_bwd_dx(dH1, h.h1, M, h.h1, h.P + L.fW1 + dx0, h.in, dxn, dxmask, ldm, dXout,
                              dxn, st, skip);
}

// the stacked LSTM over S steps from (h0, c0) ([L][B][H] each): layer 0 reads X
// (fused input projection when it fits, else xproj GEMM + recurrence), layer
// l >= 1 reads layer l-1's outputs hbuf_l-1[1..S]; keep: store the cell states
// and gate activations of every layer for a backward
// keep_steps: with keep, the cell states / gates are stored for the first
// keep_steps steps only (0: all S; the GAE pass over S1 steps keeps E)
// wimg: the transposed image of P's layer-0 weights (Ctx::wimg; one layer): the
// recurrence loads its weight columns from it (the xproj GEMM of the unfused
// form still reads W_ih's rows)
static int lstm_forward(const RnnDims& d, const float* P, const float* X, int S, const float* h0,
                        const float* c0, const RnnScratch& s, bool keep, hipStream_t st,
                        const int* skip, int keep_steps = 0, const float* wimg = nullptr) {
  const int64_t BH = (int64_t)d.B * d.H;
  for (int l = 0; l < d.L; ++l) {
    const LstmP lp = lstm_layer(d, P, l);
    const bool img = wimg && l == 0;
    const float* rWih = img ? wimg : lp.Wih;
    const float* rWhh = img ? wimg + (int64_t)d.G4 * d.Din : lp.Whh;
    const float* Xl = l == 0 ? X : hbuf_of(d, s, l - 1) + BH;
    const int64_t ldx = l == 0 ? d.ldx : d.H;
    const int din = l == 0 ? d.Din : d.H;
    float* hb = hbuf_of(d, s, l);
    float* cb = keep ? cbuf_of(d, s, l) : nullptr;
    float* gt = keep ? gates_of(d, s, l) : nullptr;
    const int rf = launch_lstm_fwd_x(Xl, ldx, din, rWih, lp.bih, rWhh, lp.bhh, h0 + l * BH,
                                     c0 + l * BH, S, d.B, d.H, hb, cb, gt, st, skip, keep_steps,
                                     img);
    if (rf == SMI_E_NOFIT) {
      const int64_t rows = (int64_t)S * d.B;
      RC_CHECK(launch_linear_fwd(Xl, ldx, (int)rows, din, lp.Wih, din, lp.bih, d.G4, ACT_NONE,
                                 s.xproj, d.G4, st, skip));
      RC_CHECK(launch_lstm_fwd(s.xproj, rWhh, lp.bhh, h0 + l * BH, c0 + l * BH, S, d.B, d.H, hb,
                               cb, gt, st, skip, keep_steps, img));
    } else if (rf) {
      return rf;
    }
  }
  return SMI_OK;
}

// gradients of the stacked LSTM's parameters (flat layout) from dh [E][B][H] at
// the top layer's outputs: BPTT layer by layer downwards, each layer's input
// gradient dgates_l W_ih_l (no activation between layers) the dh of the layer
// below; the weight gradients over [x_t | h_{t-1}] join the phase's dW group
static int lstm_backward(const RnnDims& d, const float* P, float* G, const RnnScratch& s,
                         hipStream_t st, const int* skip) {
  const int64_t BH = (int64_t)d.B * d.H;
  const int M = (int)d.NE;
  for (int l = d.L - 1; l >= 0; --l) {
    const LstmP lp = lstm_layer(d, P, l);
    float* dg = dgates_of(d, s, l);
    float* hb = hbuf_of(d, s, l);
    // one layer, no pixel stem: the BPTT shares its launch with the heads'
    // weight gradients queued so far (their partials stay reserved in the
    // workspace until the group's flush: workspace_reserve; one layer, so the
    // pre entries (<= 6 after tail splits) and this layer's (<= 2) fit the
    // reducer's 8)
    int rb = SMI_E_NOFIT;
    if (d.L == 1 && d.F == 0)
      rb = launch_lstm_bwd_dw(s.dh, gates_of(d, s, l), cbuf_of(d, s, l), lp.Whh, d.E, d.B, d.H, dg,
                              st, skip);
    if (rb == SMI_E_NOFIT)
      RC_CHECK(launch_lstm_bwd(s.dh, gates_of(d, s, l), cbuf_of(d, s, l), lp.Whh, d.E, d.B, d.H, dg,
                               st, skip));
    else if (rb)
      return rb;
    const int din = l == 0 ? d.Din : d.H;
    const float* Xl = l == 0 ? s.Xz : hbuf_of(d, s, l - 1) + BH;
    const int64_t ldx = l == 0 ? d.ldx : d.H;
    float* gWih = G + (l == 0 ? 0 : d.nL0 + (int64_t)(l - 1) * d.nLk);
    float* gWhh = gWih + (int64_t)4 * d.H * din;
    float* gbih = gWhh + (int64_t)4 * d.H * d.H;
    float* gbhh = gbih + d.G4;
    // W_ih over x_t, W_hh over h_{t-1} (hbuf[0..E-1], hbuf[0] = h0) and the
    // shared bias gradient in ONE launch over [x_t | h_{t-1}]
    RC_CHECK(launch_linear_bwd_dw2(dg, d.G4, M, d.G4, Xl, ldx, din, hb, d.H, d.H, gWih, din, gWhh,
                             d.H, gbih, gbhh, st, skip));
    if (l > 0)        // dh of layer l-1's outputs (steps 1..E) = dgates_l W_ih_l
      RC_CHECK(launch_linear_bwd_dx(dg, d.G4, M, d.G4, lp.Wih, d.H, d.H, nullptr, 0, s.dh, d.H, st,
                                    skip));
  }
  return SMI_OK;
}

static PixRows pix_rows(const smi_ppo_rnn_args& a, const RnnDims& d) {
  return PixRows{a.pixels, a.pixels_next, d.B, d.T, d.G.img};
}

// CNN features of the first S time steps into X[:, D:] (ldx = Din); A1 kept
// for a backward when non-null
static int cnn_features(const smi_ppo_rnn_args& a, const RnnDims& d, const float* cnn, int S,
                        float* X, float* A1, const RnnScratch& s, hipStream_t st,
                        const int* skip) {
  if (d.F == 0) return SMI_OK;
  // (the general stem keeps A1 in memory whether or not a backward follows)
  float* A[kStemMaxLayers] = {A1 || d.px_fused ? A1 : s.A1, s.A2, nullptr, nullptr};
  return stem_forward(d.SP, cnn, pix_rows(a, d), (int64_t)S * d.B, A, X + d.D, d.ldx, st, skip);
}

// CNN backward from dF = dL/d(features) * relu'(features) in s.dF
static int cnn_bwd_from_dF(const smi_ppo_rnn_args& a, const RnnDims& d, const float* cnn,
                           float* Gc, const RnnScratch& s, hipStream_t st, const int* skip) {
  const float* A[kStemMaxLayers] = {s.A1, s.A2, nullptr, nullptr};
  float* dA[kStemMaxLayers] = {s.dA1, s.dA2, nullptr, nullptr};
  return stem_backward(d.SP, cnn, pix_rows(a, d), d.NE, A, s.dF, d.F, Gc, dA, s.cpart, st, skip);
}

// pixel-stem gradient (into Gc) from the LSTM gate gradients of the E steps:
// dF = relu'(F) * (dgates W_ih[:, D:]), then the CNN backward
static int cnn_grad(const smi_ppo_rnn_args& a, const RnnDims& d, const LstmP& l, const float* cnn,
                    float* Gc, const RnnScratch& s, hipStream_t st, const int* skip) {
  if (d.F == 0) return SMI_OK;
  RC_CHECK(launch_linear_bwd_dx(dgates_of(d, s, 0), d.G4, (int)d.NE, d.G4, l.Wih + d.D, d.Din, d.F,
                          s.Xz + d.D, d.ldx, s.dF, d.F, st, skip));
  return cnn_bwd_from_dF(a, d, cnn, Gc, s, st, skip);
}

// the policy / value features the heads read: LSTM outputs hbuf[1..] ([S][B][H])
// or, without the LSTM (MLP policy), the stem input itself ([S][B][Din])
static const float* head_in(const RnnDims& d, const RnnScratch& s, const float* X) {
  return d.H > 0 ? hbuf_of(d, s, d.L - 1) + (int64_t)d.B * d.H : X;
}

// backward of one head into G (+ the stem below it): LSTM BPTT and/or CNN
static int stem_backward_chain(const smi_ppo_rnn_args& a, const RnnDims& d, const Head& hd,
                               const LstmP& lm, const float* cnn, float* G, const RnnScratch& s,
                               int64_t n_head, hipStream_t st, const int* skip,
                               const PolRowArgs* pg) {
  const float* X = head_in(d, s, s.Xz);
  HeadBwdOpts o;
  o.wT = s.wT;
  if (d.H > 0) {
    o.pg = pg;
    RC_CHECK(head_bwd(hd, s.dOUT, X, d.Hld, d.NE, s.HA1, s.HA2, s.dH1, s.dH2, G, 0, d.H, nullptr,
                      0, s.dh, st, skip, o));
    RC_CHECK(lstm_backward(d, a.lstm, G + n_head, s, st, skip));
    return cnn_grad(a, d, lm, cnn, G + n_head + d.nL, s, st, skip);
  }
  if (pg) return set_error(SMI_E_ARG, "ppo_rnn: the policy prologue needs the LSTM stem");
  // MLP policy: the first head layer's input gradient over the CNN columns only
  RC_CHECK(head_bwd(hd, s.dOUT, X, d.Hld, d.NE, s.HA1, s.HA2, s.dH1, s.dH2, G, d.D, d.F,
                    s.Xz + d.D, d.ldx, s.dF, st, skip, o));
  if (d.F == 0) return SMI_OK;
  return cnn_bwd_from_dF(a, d, cnn, G + n_head, s, st, skip);
}

// every weight gradient of the phase (head layers + LSTM) queued and run as
// one grouped launch after the input-gradient chain and BPTT
// ex: the reducer's epilogue task (the log_var gradient, the clip-norm partials)
static int stem_backward(const smi_ppo_rnn_args& a, const RnnDims& d, const Head& hd,
                         const LstmP& lm, const float* cnn, float* G, const RnnScratch& s,
                         int64_t n_head, hipStream_t st, const int* skip,
                         const DwEpilogue* ex = nullptr, const PolRowArgs* pg = nullptr) {
  dw_group_begin();
  if (ex) RC_CHECK(dw_group_epilogue(*ex));
  const int rc = stem_backward_chain(a, d, hd, lm, cnn, G, s, n_head, st, skip, pg);
  const int rf = dw_group_flush(st);     // always flush: nothing stays queued after an error
  return rc ? rc : rf;
}

static float c_loglik_of(int A) { return (float)(0.5 * log(2.0 * 3.141592653589793) * (double)A); }
static float c_entropy_of(int A) {
  return (float)(0.5 * log(2.0 * 3.141592653589793 * 2.718281828459045) * (double)A);
}

int64_t ppo_rnn_scratch_bytes(int B, int T, int Hz, int D, int H, int L, int h1, int h2, int A, int c1,
                              int c2, int pc, int ph, int pw, int F) {
  return 4 * rnn_scratch(rnn_dims(B, T, Hz, D, H, h1, h2, A, c1, c2, pc, ph, pw, F, L), nullptr)
                 .total_floats;
}

int64_t ppo_rnn_wimage_offset(int B, int T, int Hz, int D, int H, int L, int h1, int h2, int A, int c1,
                              int c2, int pc, int ph, int pw, int F) {
  return rnn_scratch(rnn_dims(B, T, Hz, D, H, h1, h2, A, c1, c2, pc, ph, pw, F, L), nullptr)
      .wimg_off;
}

static PolRowArgs pol_rows(const smi_ppo_rnn_args& a, const RnnDims& d, const RnnScratch& s) {
  PolRowArgs p{};
  p.B = d.B; p.T = d.T; p.E = d.E; p.A = d.A; p.mode = a.mode;
  p.mu = s.OUT; p.lv = a.actor + d.LA.flv; p.refmu = s.refmu; p.ref_lv = a.ref_actor + d.LA.flv;
  p.actions = a.actions; p.behave = a.behave; p.adv = s.adv; p.ret = s.ret;
  p.rowin = s.rowin; p.ret_tm = s.ret_tm;
  p.moments = a.moments; p.norm_adv = a.norm_adv; p.c_ll = c_loglik_of(d.A);
  p.hyper = a.hyper; p.skip = s.ci + CI_STOP;
  p.part = s.part; p.dz = s.dOUT; p.lvpart = s.lvpart; p.cf = s.cf;
  return p;
}

// ----------------------------------------------------------- context, rules
// what every phase needs, built once per ppo_rnn_phase call
struct Ctx {
  const smi_ppo_rnn_args& a;
  RnnDims d;
  RnnScratch s;
  const int* stop;              // the device stop flag (KL early stop)
  LstmP lm;                     // layer 0 of the trained stem
  const float* cnn;             // stem = [lstm | cnn]
  Head actor, critic;
  float *gA, *gC;               // [actor head | lstm | cnn], [critic head | lstm | cnn]
  int64_t NEg;                  // training rows of all ranks
  hipStream_t st;
  // the transposed image of the trained stem's layer-0 weights (s.wimg) when
  // the epoch forwards load from it (the r4 form runs at this batch), else
  // null: nobody writes or reads the region
  float* wimg;
};

static Ctx make_ctx(const smi_ppo_rnn_args& a, hipStream_t st) {
  const RnnDims d = rnn_dims(a.B, a.T, a.horizon, a.obs_dim, a.rnn_hidden, a.h1, a.h2, a.act_dim,
                             a.critic_h1, a.critic_h2, a.pix_c, a.pix_h, a.pix_w, a.cnn_feat,
                             a.rnn_layer);
  const RnnScratch s = rnn_scratch(d, a.scratch);
  return Ctx{a, d, s, s.ci + CI_STOP, lstm_params(a.lstm, d.Din, d.H), a.lstm + d.nL,
             Head{a.actor, d.LA, d.Hin, d.h1, d.h2, d.A, 1},
             Head{a.critic, d.LC, d.Hin, d.c1, d.c2, 1, 0},
             a.xbuf, a.xbuf + d.nA_head + d.nS, (int64_t)d.E * a.B_global, st,
             s.wimg && lstm_fwd_image_ok(d.B, d.H) ? s.wimg : nullptr};
}

// The choices more than one phase depends on.  Each is a function of
// (a, d, s) alone, so every phase of a learn() gets the same answer; the
// phases that must agree read it here and nowhere else:
//
//   rule             read by                     what the readers must agree on
//   gae_prep_dual    GAE, PREP                   GAE formed PREP's input and ran its recurrence
//                                                exactly when PREP leaves them out
//   pol_stats_nb     POLICY_FWD, POLICY_BWD      FWD's statistics grid is the partial count BWD's
//                                                decision reduces (dec_nb) and, in clip mode,
//                                                the log_var partial count of its epilogue
//   fused_decide(e)  POLICY_FWD, POLICY_BWD      FWD leaves the decision out exactly when BWD's
//                                                gradient pass takes it
//   pol_head_grad    POLICY_BWD (row pass, dW    the row pass is left out exactly when the head
//                    epilogue, head chain)       chain's prologue runs it, and the epilogue
//                                                reduces that chain's log_var partials
//   fused_clip_norm  POLICY_BWD, POLICY_APPLY,   the dW reducer wrote the sums of squares and
//                    VALUE_GRAD, VALUE_APPLY     bumped the step exactly when APPLY does not
//   vstats(e)        VALUE_GRAD (head forward,   who summed the last epoch's value statistics,
//                    value rows, reduction)      and over how many partials
//   Ctx::wimg        GAE, POLICY_FWD,            GAE built the weight image and every Adam that
//                    VALUE_GRAD, both APPLYs     ran kept it current exactly when the epoch
//                                                forwards load from it
struct Rules {
  const smi_ppo_rnn_args& a;
  const RnnDims& d;
  const RnnScratch& s;
  const Head& actor;

  // One rank with no pixel stem: the optimizer's clip_grad_norm_ partials come
  // from the dW group's reducer (every gradient of [head | lstm] but log_var is a
  // reducer output, log_var is the reducer's epilogue task), so the APPLY phases
  // run Adam alone.  Data parallel: the norm is of the all-reduced gradient, so
  // the sums of squares stay in APPLY (sumsq_part_kernel); with the pixel stem
  // the CNN gradient is not a reducer output.
  // Every weight gradient of both optimizers must join the group for that
  // (dw_group_takes: heads wider than 511 or 4H > 512 run outside it); the flush
  // also fails loudly if one ran outside an open bracket with the fused norm.
  bool fused_clip_norm() const {
    if (a.B_global != a.B || d.F != 0 || d.L > 3 || fault() != 0) return false;
    const bool heads = dw_group_takes(d.h1, d.Hin + 1) && dw_group_takes(d.h2, d.h1 + 1) &&
                       dw_group_takes(d.A, d.h2 + 1) && dw_group_takes(d.c1, d.Hin + 1) &&
                       dw_group_takes(d.c2, d.c1 + 1) && dw_group_takes(1, d.c2 + 1);
    const bool stem = d.H == 0 || (dw_group_takes(d.G4, d.ldx + d.H + 1) &&
                                   (d.L == 1 || dw_group_takes(d.G4, d.H + d.H + 1)));
    return heads && stem;
  }

  // the GAE critic pass (T + 1 steps) and PREP's reference-policy forward (E
  // steps) as ONE recurrence launch (two weight sets over two inputs, B
  // workgroups each): one LSTM layer, no pixel stem, the one-segment form for 2B
  // segments, PREP issued after GAE on the same stream (a.prep_independent == 0:
  // the caller's explicit statement, no environment read here); GAE then also
  // forms PREP's z-filtered input and PREP runs the reference head only.
  bool gae_prep_dual() const {
    return a.prep_independent == 0 && d.H > 0 && d.L == 1 && d.F == 0 &&
           lstm_fwd_x_dual_fits(d.B, d.B, d.S1 > d.E ? d.S1 : d.E, d.H, d.Din);
  }

  // adapt mode with the LSTM stem, 8 actions and the fused head chain at a
  // rank's batch (< 16384 rows: one row tile per workgroup): the policy-gradient
  // row pass runs as that chain's prologue (head_kernels.hip, pol_rows.hpp); one log_var
  // partial per chain workgroup (<= the 4096 of s.lvpart).  Measured: 128
  // segments 2.947 -> 2.929 ms per learn; 1024 segments 6.98 -> 7.05 ms (the
  // 32-row workgroups' serial prologue costs more than the launch it saves)
  bool pol_head_grad() const {
    return a.mode != 0 && d.H > 0 && d.A == 8 && d.H <= 320 && d.NE < 16384 &&
           head_fused(actor, head_in(d, s, s.Xz), d.Hld) && head_bwd_blocks(d.NE) <= 4096;
  }

  // the partials the policy statistics pass wrote (its grid)
  int pol_stats_nb() const { return pol_stats_blocks(a.mode == 0, d.A, d.NE); }

  // adapt mode, one rank, a policy epoch that trains: the decision of POLICY_FWD
  // (early stop, KL coefficient, statistics) is taken by the gradient pass of
  // POLICY_BWD itself (policy_rows_grad_kernel, dec_part)
  bool fused_decide(int e) const {
    // every gradient workgroup re-reduces the statistics pass's partials: only
    // while they are few (at 65536 segments, ~3000 partials per workgroup over
    // ~4000 workgroups took the gradient pass from 47 to 103 us)
    return a.mode != 0 && a.B_global == a.B && e < a.epoch_policy && fault() == 0 &&
           pol_stats_nb() <= 512;
  }

  // the last value epoch's statistics of ppo.py:324-331 summed by the head
  // forward's epilogue, one 5-double partial per head workgroup, when the
  // fused head runs (vdone) and the partials fit s.part
  bool vstats(int e) const {
    const bool last = e == a.epoch_baseline - 1;
    return last && 5 * (int64_t)head_bwd_blocks(d.NE) <= part_doubles(d);
  }
};

static DecideArgs decide_args(const Ctx& c, int e) {
  const smi_ppo_rnn_args& a = c.a;
  return DecideArgs{a.pstat, e, a.epoch_policy, a.mode,
                    a.kl_target, a.kl_cutoff_coeff, c.NEg, a.hyper, a.actor + c.d.LA.flv, c.d.A,
                    c_entropy_of(c.d.A), c.s.ci, c.s.cf, a.stats};
}

// a head forward no backward follows: activations and weight transposes not kept
static HeadFwdOpts fwd_only() {
  HeadFwdOpts o;
  o.keep_act = false;
  return o;
}

// ------------------------------------------------------------------- phases
static int phase_gae(const Ctx& c, const Rules& r) {
  const smi_ppo_rnn_args& a = c.a;
  const RnnDims& d = c.d;
  const RnnScratch& s = c.s;
  hipStream_t st = c.st;
  int kt = ktime_begin(st);
  const int zrc = launch_zf_tmajor(a.obs, a.obs_next, d.B, d.T, d.S1, d.D, a.use_zf, a.zf_sum,
                                   a.zf_sumsq, a.zf_count, a.zf_eps, s.Xz, d.ldx, st, 0,
                                   d.F == 0);
  ktime_end(kt, KT_ZF_TMAJOR, 8.0 * (double)d.NG * d.D, st);      // read x, write z(x)
  RC_CHECK(zrc);
  RC_CHECK(cnn_features(a, d, c.cnn, d.S1, s.Xz, nullptr, s, st, nullptr));
  // the critic's LSTM pass over T + 1 steps (ppo.py:385) with the cell
  // states and gates of its first E steps kept: the first policy forward
  // (ppo.py:253-262 at epoch 0) is the same recurrence over the same
  // inputs from the same (h0, c0) with the same parameters, so
  // POLICY_FWD(0) reads these instead of recomputing them
  if (r.gae_prep_dual()) {
    // PREP's input (the reference z-filter over obs_iter), then both
    // recurrences in one launch: the critic's over T + 1 steps keeping E
    // steps' cells / gates, the reference policy's over E steps
    RC_CHECK(launch_zf_tmajor(a.obs, a.obs_next, d.B, d.T, d.E, d.D, a.use_zf, a.rzf_sum,
                              a.rzf_sumsq, a.rzf_count, a.zf_eps, s.Xr, d.ldx, st, 0,
                              d.F == 0));
    const LstmP lc = lstm_layer(d, a.lstm, 0), lr = lstm_layer(d, a.ref_lstm, 0);
    LstmFwdArgs g0{nullptr, lc.Whh, lc.bhh, a.h0, a.c0, d.S1, d.B, d.H, hbuf_of(d, s, 0),
                   cbuf_of(d, s, 0), gates_of(d, s, 0), nullptr, s.Xz, d.ldx, d.Din, lc.Wih,
                   lc.bih, d.E};
    LstmFwdArgs g1{nullptr, lr.Whh, lr.bhh, a.h0, a.c0, d.E, d.B, d.H, s.hbufR, nullptr, nullptr,
                   nullptr, s.Xr, d.ldx, d.Din, lr.Wih, lr.bih, 0};
    RC_CHECK(launch_lstm_fwd_x_dual(g0, g1, st));
  } else if (d.H > 0) {
    RC_CHECK(lstm_forward(d, a.lstm, s.Xz, d.S1, a.h0, a.c0, s, true, st, nullptr, d.E));
  }
  // the parameters may have been replaced since the last learn (checkpoint
  // load, DP broadcast): the weight image the epoch forwards load from is
  // rebuilt from them once per learn, by a launch of its own (57 K floats at
  // C3); the Adam applies keep it current from here on.  After the recurrence
  // above: the image lives in the tail of s.xproj (rnn_layout.hpp), which that
  // pass over S1 steps is the only one to use
  if (c.wimg) RC_CHECK(launch_lstm_weight_image(c.lm.Wih, c.lm.Whh, d.Din, d.H, c.wimg, st));
  RC_CHECK(head_fwd(c.critic, head_in(d, s, s.Xz), d.Hld, d.NG, s.HA1, s.HA2, s.OUT, st,
                    fwd_only()));
  // (also zeroes the learn()'s device control state)
  RC_CHECK(launch_tmajor_to_bmajor(s.OUT, d.S1, d.B, s.values, s.ci, s.cf, st));
  int np = 0;
  kt = ktime_begin(st);
  RC_CHECK(launch_gae_windows(s.values, nullptr, a.rewards, a.dones, d.B, d.T, d.Hz, a.gamma_tab,
                              a.lam_tab, a.gamma, a.gamma_H, s.adv, s.ret, s.gaepart, &np, st));
  // r, d (8 B) + V (4 (T+1)/T B) per env-step, adv + ret (8 B) per window
  ktime_end(kt, KT_GAE, (double)d.B * (8.0 * d.T + 4.0 * d.S1 + 8.0 * d.E), st);
  return launch_reduce_partials(s.gaepart, np, 2, a.moments, nullptr, a.moments + 2,
                                (double)d.NE, st);
}

static int phase_prep(const Ctx& c, const Rules& r) {
  const smi_ppo_rnn_args& a = c.a;
  const RnnDims& d = c.d;
  const RnnScratch& s = c.s;
  hipStream_t st = c.st;
  // ref_pol (ppo.py:539): the reference model's forward over obs_iter.
  // With a.prep_independent != 0 it reads only the batch and the reference
  // parameters and writes only its own buffers (sp) and refmu, so the host
  // may run it on a second stream beside GAE (with its own smi_context).
  // With a.prep_independent == 0 it must follow GAE on the same stream: GAE
  // may have run its input transpose and recurrence (gae_prep_dual).
  RnnScratch sp = s;
  sp.xproj = s.xprojR; sp.hbuf = s.hbufR; sp.HA1 = s.HA1R; sp.HA2 = s.HA2R; sp.A2 = s.A2R;
  sp.A1 = s.A1R;
  const float* X = s.Xr;
  if (!r.gae_prep_dual()) {   // (else the GAE phase ran this input and recurrence)
    RC_CHECK(launch_zf_tmajor(a.obs, a.obs_next, d.B, d.T, d.E, d.D, a.use_zf, a.rzf_sum,
                              a.rzf_sumsq, a.rzf_count, a.zf_eps, s.Xr, d.ldx, st, 0,
                              d.F == 0));
    RC_CHECK(cnn_features(a, d, a.ref_lstm + d.nL, d.E, s.Xr, nullptr, sp, st, nullptr));
    if (d.H > 0)
      RC_CHECK(lstm_forward(d, a.ref_lstm, X, d.E, a.h0, a.c0, sp, false, st, nullptr));
  }
  const Head ref{a.ref_actor, d.LA, d.Hin, d.h1, d.h2, d.A, 1};
  return head_fwd(ref, head_in(d, sp, X), d.Hld, d.NE, sp.HA1, sp.HA2, s.refmu, st, fwd_only());
}

static int phase_policy_fwd(const Ctx& c, const Rules& r, int e) {
  const smi_ppo_rnn_args& a = c.a;
  const RnnDims& d = c.d;
  const RnnScratch& s = c.s;
  hipStream_t st = c.st;
  if (e == 0) RC_CHECK(launch_row_pack(d.A, d.NE, pol_rows(a, d, s), s.rowin, s.ret_tm, st));
  if (e == 0 && (a.adv_out || a.ret_out))
    RC_CHECK(launch_adv_export(pol_rows(a, d, s), d.NE, a.adv_out, a.ret_out, st));
  RC_CHECK(cnn_features(a, d, c.cnn, d.E, s.Xz, s.A1, s, st, c.stop));
  if (d.H > 0 && e > 0)
    RC_CHECK(lstm_forward(d, a.lstm, s.Xz, d.E, a.h0, a.c0, s, true, st, c.stop, 0, c.wimg));
  PolRowArgs p = pol_rows(a, d, s);
  p.invN = (float)(1.0 / (double)c.NEg);
  // (the KL check after the last update, e == epoch_policy, has no backward:
  // neither the activations nor the weight transposes are kept)
  const bool bwd_next = e < a.epoch_policy;
  HeadFwdOpts o;
  o.skip = c.stop;
  o.wT = bwd_next ? s.wT : nullptr;
  o.keep_act = bwd_next;
  RC_CHECK(head_fwd(c.actor, head_in(d, s, s.Xz), d.Hld, d.NE, s.HA1, s.HA2, s.OUT, st, o));
  const int nb = r.pol_stats_nb();
  RC_CHECK(launch_pol_stats(a.mode == 0, nb, p, st));     // clip: + the clip gradient
  if (r.fused_decide(e)) return SMI_OK;     // decided by POLICY_BWD's gradient pass
  if (a.B_global == a.B)           // one rank: nothing to exchange before the decision
    return launch_reduce_decide(s.part, nb, decide_args(c, e), c.stop, st);
  return launch_reduce_partials(s.part, nb, PS_N, a.pstat, c.stop, nullptr, 0.0, st);
}

static int phase_policy_decide(const Ctx& c, int e) {   // after the pstat all-reduce
  if (c.a.B_global == c.a.B) return SMI_OK;     // decided by POLICY_FWD's reduce_decide_kernel
  return launch_policy_decide(decide_args(c, e), c.st);
}

static int phase_policy_bwd(const Ctx& c, const Rules& r, int e) {
  const smi_ppo_rnn_args& a = c.a;
  const RnnDims& d = c.d;
  const RnnScratch& s = c.s;
  if (fault() == SMI_FAULT_POLICY_EPOCH_SHORT && e == a.epoch_policy - 1) return SMI_OK;
  PolRowArgs p = pol_rows(a, d, s);
  // clip: the log_var partials came from POLICY_FWD's fused pass, over its grid
  const int nb = a.mode == 0 ? r.pol_stats_nb() : rnn_nblk(d.NE, kRowNT);
  if (r.fused_decide(e)) {
    p.dec_part = s.part;
    p.dec_nb = r.pol_stats_nb();
    p.dec = decide_args(c, e);
  }
  // adapt: the gradient row pass as the fused head chain's prologue (one
  // launch fewer), or its own launch
  const bool pgh = r.pol_head_grad();
  const int nb_pg = pgh ? head_bwd_blocks(d.NE) : nb;
  // (clip: dz and the log_var partials came with POLICY_FWD's pass)
  if (a.mode != 0 && !pgh) RC_CHECK(launch_pol_grad(nb, p, c.st));
  // the log_var gradient (and, fused, the clip-norm partials and the step
  // bump) as the dW reducer's epilogue task
  DwEpilogue ex{};
  ex.lvpart = s.lvpart; ex.lv_nb = nb_pg; ex.lv_A = d.A;
  ex.lv = a.actor + d.LA.flv; ex.lv_out = c.gA + d.LA.flv;
  ex.skip = c.stop;
  if (r.fused_clip_norm()) {
    ex.sq = s.part; ex.np = s.ci + CI_NP;
    ex.step = a.actor_step; ex.runs = s.ci + CI_RUNS;
  }
  return stem_backward(a, d, c.actor, c.lm, c.cnn, c.gA, s, d.nA_head, c.st, c.stop, &ex,
                       pgh ? &p : nullptr);
}

// torch.optim.Adam over one optimizer's list [head | stem] after its
// clip_grad_norm_ (ppo.py:243-247, 348-352); the policy's apply obeys the stop
// flag and counts the epochs that ran
static int adam_apply(const Ctx& c, const Rules& r, bool policy) {
  const smi_ppo_rnn_args& a = c.a;
  const RnnDims& d = c.d;
  const int64_t nS = !policy && fault() == SMI_FAULT_CRITIC_STEM_OMIT ? 0 : d.nS;
  const int64_t n_head = policy ? d.nA_head : d.nC_head;
  const int g = grid_of(n_head + nS, 1024);
  const bool fn = r.fused_clip_norm();
  const bool clip = policy ? a.clip_actor_grad : a.clip_critic_grad;
  const float max_norm = policy ? a.actor_max_norm : a.critic_max_norm;
  float* norm_out = a.stats + (policy ? SMI_ST_GRAD_NORM_ACTOR : SMI_ST_GRAD_NORM_CRITIC);
  AdamSplitArgs aa{policy ? a.actor : a.critic, n_head, a.lstm, nS, policy ? c.gA : c.gC,
                   policy ? a.actor_m : a.critic_m, policy ? a.actor_v : a.critic_v,
                   policy ? a.actor_step : a.critic_step,
                   a.hyper + (policy ? SMI_HYP_LR_ACTOR : SMI_HYP_LR_CRITIC), a.beta1, a.beta2,
                   a.adam_eps, policy ? a.actor_wd : a.critic_wd, clip ? max_norm : 0.f,
                   c.s.part, g, policy ? c.stop : nullptr, clip ? norm_out : nullptr, nullptr,
                   fn ? c.s.ci + CI_NP : nullptr, c.wimg, d.Din, d.H,
                   lstm_fwd_x_fuses(d.Din, d.H) ? 1 : 0};
  return launch_adam_split(aa, g, fn ? nullptr : c.s.part, policy ? c.s.ci + CI_RUNS : nullptr,
                           c.st);
}

static int phase_policy_apply(const Ctx& c, const Rules& r, int e) {
  if (fault() == SMI_FAULT_POLICY_EPOCH_SHORT && e == c.a.epoch_policy - 1) return SMI_OK;
  return adam_apply(c, r, true);
}

static int phase_value_grad(const Ctx& c, const Rules& r, int e) {
  const smi_ppo_rnn_args& a = c.a;
  const RnnDims& d = c.d;
  const RnnScratch& s = c.s;
  hipStream_t st = c.st;
  // value epoch 0: the last policy forward that ran (the KL check after
  // the last policy update, ppo.py:553-556, or the epoch-0 forward with
  // no update) left the stem's outputs, cell states, gates and conv
  // activations of exactly the current parameters: reused, not recomputed
  if (e > 0) {
    RC_CHECK(cnn_features(a, d, c.cnn, d.E, s.Xz, s.A1, s, st, nullptr));
    if (d.H > 0)
      RC_CHECK(lstm_forward(d, a.lstm, s.Xz, d.E, a.h0, a.c0, s, true, st, nullptr, 0, c.wimg));
  }
  // dV = 2 (V - R) / N: written by the head forward's epilogue, except in
  // the last epoch, whose value_rows pass also sums the statistics of
  // ppo.py:324-331 (and on the layer-GEMM path)
  // (round 6: the last epoch's statistics too, one 5-double partial per
  // head workgroup, when the fused head runs and the partials fit s.part)
  const bool last = e == a.epoch_baseline - 1;
  const float vscale = (float)(2.0 / (double)c.NEg);
  bool vdone = false;
  const bool vstats = r.vstats(e);
  HeadFwdOpts o;
  o.wT = s.wT;
  o.vret = last && !vstats ? nullptr : s.ret_tm;
  o.vgrad = last && !vstats ? nullptr : s.dOUT;
  o.vscale = vscale;
  o.vpart = vstats ? s.part : nullptr;
  o.vdone = &vdone;
  RC_CHECK(head_fwd(c.critic, head_in(d, s, s.Xz), d.Hld, d.NE, s.HA1, s.HA2, s.OUT, st, o));
  int nb = rnn_nblk((d.NE + 3) / 4, kRowNT);           // 4 rows per thread
  if (vdone && vstats) nb = head_bwd_blocks(d.NE);     // the head forward's partials
  if (!vdone)
    RC_CHECK(launch_value_rows(s.OUT, s.ret_tm, d.B, d.E, vscale, s.dOUT, last ? s.part : nullptr,
                               nb, st));
  if (last) RC_CHECK(launch_reduce_partials(s.part, nb, 5, a.zbuf, nullptr, nullptr, 0.0, st));
  if (!r.fused_clip_norm())
    return stem_backward(a, d, c.critic, c.lm, c.cnn, c.gC, s, d.nC_head, st, nullptr);
  DwEpilogue ex{};                // the clip-norm partials and the step bump
  ex.sq = s.part; ex.np = s.ci + CI_NP;
  ex.step = a.critic_step;
  return stem_backward(a, d, c.critic, c.lm, c.cnn, c.gC, s, d.nC_head, st, nullptr, &ex);
}

static int phase_value_apply(const Ctx& c, const Rules& r) {
  if (fault() == SMI_FAULT_CRITIC_ADAM_SKIP) return SMI_OK;
  return adam_apply(c, r, false);
}

static int phase_zstats(const Ctx& c) {
  const smi_ppo_rnn_args& a = c.a;
  const RnnDims& d = c.d;
  // zbuf (double) = [value sums (5) | column sums (D) | sums of squares (D)]
  if (!a.use_zf) return SMI_OK;
  // >= 64 rows per block (16 per wave, four in flight), at most 256 blocks
  const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(256, (d.NE + 63) / 64));
  double* part = c.s.part;     // [nb][2][D] <= 65536 doubles for D <= 128
  if ((int64_t)nb * 2 * d.D > 4096 * 16) return set_error(SMI_E_ARG, "ppo_rnn: obs_dim too large");
  RC_CHECK(launch_obs_iter_colsum(a.obs, d.B, d.T, d.E, d.D, part, nb, c.st));
  return launch_reduce_partials(part, nb, 2 * d.D, a.zbuf + FS_Z, nullptr, nullptr, 0.0, c.st);
}

static int phase_zapply(const Ctx& c) {
  const smi_ppo_rnn_args& a = c.a;
  const FinalArgs fa{a.zbuf, c.d.D, c.NEg, a.actor + c.d.LA.flv, c.d.A,
                     a.clip_critic_grad, a.zf_sum, a.zf_sumsq, a.zf_count, a.use_zf, a.stats,
                     c.s.ci, a.kl_record, a.kl_count, a.kl_capacity, a.epoch_policy};
  return launch_rnn_final(fa, c.st);
}

int ppo_rnn_phase(const smi_ppo_rnn_args& a, int phase, int e, hipStream_t st) {
  const Ctx c = make_ctx(a, st);
  if (c.s.total_floats * 4 > a.scratch_bytes)
    return set_error(SMI_E_ARG, "ppo_rnn: scratch too small");
  const Rules r{a, c.d, c.s, c.actor};
  switch (phase) {
    case SMI_RNN_PH_GAE: return phase_gae(c, r);
    case SMI_RNN_PH_PREP: return phase_prep(c, r);
    case SMI_RNN_PH_POLICY_FWD: return phase_policy_fwd(c, r, e);
    case SMI_RNN_PH_POLICY_DECIDE: return phase_policy_decide(c, e);
    case SMI_RNN_PH_POLICY_BWD: return phase_policy_bwd(c, r, e);
    case SMI_RNN_PH_POLICY_APPLY: return phase_policy_apply(c, r, e);
    case SMI_RNN_PH_VALUE_GRAD: return phase_value_grad(c, r, e);
    case SMI_RNN_PH_VALUE_APPLY: return phase_value_apply(c, r);
    case SMI_RNN_PH_ZSTATS: return phase_zstats(c);
    case SMI_RNN_PH_ZAPPLY: return phase_zapply(c);
    default: return set_error(SMI_E_ARG, "ppo_rnn: unknown phase");
  }
}

}  // namespace smi
