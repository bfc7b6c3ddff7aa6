// rnn_kernels.hpp — launchers of the LSTM learner's own kernels
// (ppo_rnn_kernels.hip) for the host sequencing in ppo_rnn.hip.  Each launcher
// is one function: the grid rule that belongs to the kernel, the kernel-timing
// bracket where the launch has one, and check_launch.
#pragma once
#include "smi_internal.hpp"
#include "pol_rows.hpp"

namespace smi {

// final sums (fstat, double): value statistics of the last value epoch, then
// the ZFilter column sums of obs_iter
enum { FS_SE = 0, FS_D, FS_D2, FS_R, FS_R2, FS_Z = 5 };

inline int rnn_nblk(int64_t rows, int nt = kWG) {
  // at most 1024 four-wave blocks' worth of waves (4096 one-wave blocks)
  const int64_t cap = (int64_t)1024 * kWG / nt;
  const int64_t b = (rows + nt - 1) / nt;
  return (int)(b < cap ? (b < 1 ? 1 : b) : cap);
}
// per-row loss kernels (a thread per row, ~100 dependent VALU / transcendental
// ops each): one-wave blocks so the rows of a C3 batch (21504) spread over
// 336 CUs' worth of blocks instead of 84 four-wave blocks
constexpr int kRowNT = 64;
inline int grid_of(int64_t n, int cap = 1024) {
  int64_t g = (n + kWG - 1) / kWG;
  if (g < 1) g = 1;
  return (int)(g < cap ? g : cap);
}

// the time-major z-filtered copy of the batch's low-dim observations (forms:
// ppo_rnn_kernels.hip)
int launch_zf_tmajor(const float* obs, const float* obs_next, int B, int T, int S, int D,
                     int use_zf, const float* zs, const float* zq, const float* zc, float eps,
                     float* out, int ldo, hipStream_t st, int form = 0, bool pad_ok = false);
// values[b][t] = vt[t*B + b]; ci / cf (non-null) zeroed
int launch_tmajor_to_bmajor(const float* vt, int S, int B, float* v, int* ci, float* cf,
                            hipStream_t st);
int launch_reduce_partials(const double* part, int nb, int w, double* out, const int* skip,
                           double* cnt, double n, hipStream_t st);
int launch_adv_export(const PolRowArgs& p, int64_t rows, float* adv_out, float* ret_out,
                      hipStream_t st);
int launch_row_pack(int A, int64_t rows, const PolRowArgs& p, float* rowin, float* ret_tm,
                    hipStream_t st);
// workgroups of the statistics pass (fuse: with the clip gradient), and the pass
int pol_stats_blocks(bool fuse, int A, int64_t rows);
int launch_pol_stats(bool fuse, int nb, const PolRowArgs& p, hipStream_t st);
int launch_pol_grad(int nb, const PolRowArgs& p, hipStream_t st);
int launch_policy_decide(const DecideArgs& da, hipStream_t st);
int launch_reduce_decide(const double* part, int nb, const DecideArgs& da, const int* skip,
                         hipStream_t st);
// dV (and, part non-null, the value statistics' partials) over nb one-wave blocks
int launch_value_rows(const float* V, const float* ret_tm, int B, int E, float invN2, float* dV,
                      double* part, int nb, hipStream_t st);
int launch_obs_iter_colsum(const float* obs, int B, int T, int E, int D, double* part, int nb,
                           hipStream_t st);

// torch.optim.Adam over one optimizer's parameter list [head | lstm] (two
// parameter buffers, one gradient / moment buffer), after clip_grad_norm_
// over the same list (ppo.py:243-247, 348-352).
struct AdamSplitArgs {
  float* p0; int64_t n0; float* p1; int64_t n1;
  const float* g; float* m; float* v;
  int* step; const float* lr_ptr; float beta1, beta2, eps, wd, max_norm;
  const double* part; int np;
  const int* skip; float* norm_out; int* runs;
  const int* np_dev;     // non-null: the partial count on the device (a fused sum of squares)
  // non-null: p1 starts with LSTM layer 0's W_ih [4 wH][wdin] | W_hh [4 wH][wH], and
  // every new value of those is also stored at its transposed position in wimg
  // ([W_ihT [wdin][4 wH] | W_hhT [wH][4 wH] | zeros], the r4 forward's weight image)
  // wih == 0: W_ihT is left as it is (no forward reads it: the unfused form's
  // xproj GEMM takes W_ih's rows)
  float* wimg; int wdin, wH, wih;
};
// clip_grad_norm_ + Adam over grid workgroups.  sumsq_part non-null: the sums
// of squares of a.g are formed here first (into sumsq_part == a.part, with the
// step / runs bump); null: a fused reducer already wrote them (a.np_dev)
int launch_adam_split(const AdamSplitArgs& a, int grid, double* sumsq_part, int* runs,
                      hipStream_t st);

struct FinalArgs {
  const double* fs; int D; int64_t N; const float* lv; int A; int clip_critic;
  float* zs; float* zq; float* zc; int use_zf;
  float* stats; const int* ci; float* kl_record; int* kl_count; int kl_capacity; int Ep;
};
int launch_rnn_final(const FinalArgs& a, hipStream_t st);

}  // namespace smi
