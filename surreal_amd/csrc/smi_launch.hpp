// smi_launch.hpp — the one declaration of every host function that one .hip
// unit defines and another calls (beyond the plumbing of smi_internal.hpp,
// which includes this file, so the defining unit sees it too).  Parameter names
// are the definitions'; default arguments appear only here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace smi {

struct PolRowArgs;     // pol_rows.hpp
struct LstmFwdArgs;    // lstm_cell.hpp
struct ConvGeom;       // conv_plan.hpp
struct PixRows;        // smi_internal.hpp
struct StemPlan;       // stem_plan.hpp

// ---- ops_kernels.hip
int launch_zfilter_apply(const float* x, float* out, int64_t rows, int dim, const float* s,
                         const float* sq, const float* cnt, float eps, hipStream_t st);
int launch_colstats(const float* x, int64_t rows, int dim, int64_t stride, int mode,
                    float* osum, float* osq, float* cnt, hipStream_t st);
int launch_reward_filter(float* r, int64_t n, float scale, int use, float* s, float* sq,
                         float* c, float eps, double* out3, hipStream_t st);
int launch_reward_filter_commit(const double* s3, float* s, float* sq, float* c, hipStream_t st);
int launch_diag_gauss(const float* a, const float* p0, const float* p1, int64_t rows, int A,
                      float* ll, float* lik, float* kl, float* ent, hipStream_t st);
int launch_mlp_forward(const float* params, int in, int h1, int h2, int out, int act, int lv,
                       const float* x, int64_t rows, int64_t stride, int use_zf,
                       const float* zs, const float* zsq, const float* zc, float zeps,
                       float* y, hipStream_t st);
int launch_moments(const float* x, int64_t n, const double* part, int np, double* out,
                   hipStream_t st);
int launch_adam_clip(float* p, const float* g, float* m, float* v, int64_t n, int* step,
                     const float* lr, float b1, float b2, float eps, float wd, float max_norm,
                     float clip_value, const int* skip, float* norm_out, hipStream_t st);
int launch_zfilter_accumulate(const float* s, const float* s2, int dim, float rows, float* rs,
                              float* rsq, float* cnt, hipStream_t st);
int launch_ddpg_target(const float* r, const float* d, const float* q, const float* q2,
                       int64_t n, float gn, float* y, hipStream_t st);
// ---- ddpg_kernels.hip
int launch_mse_grad(const float* q, int64_t qs, const float* y, int64_t n, float* dq, float* loss,
                    hipStream_t st);
int launch_mse_grad_weighted(const float* q, int64_t qs, const float* y, const float* w, int64_t n,
                             int64_t n_global, int64_t row0, float* dq, float* loss, float* td,
                             hipStream_t st);
int launch_neg_mean_grad(const float* q, int64_t qs, int64_t n, float* dq, float* loss,
                         hipStream_t st);
int launch_tanh_backward(const float* dy, int64_t ldg, const float* y, int64_t ldy, int64_t rows,
                         int cols, float* dz, int64_t ldz, hipStream_t st);
int launch_copy_cols(const float* src, int64_t lds, int64_t rows, int cols, float* dst,
                     int64_t ldd, hipStream_t st);
int launch_copy_bytes16(const void* src, void* dst, int64_t n16, hipStream_t st);
int launch_copy_gather(void* dst, const void* const* srcs, const int64_t* offs,
                       const int64_t* nbytes, int n, hipStream_t st);
int launch_soft_update(float* t, const float* s, int64_t n, float tau, hipStream_t st);
int launch_ddpg_stats(const float* a, int64_t lda, int A, const float* r, int64_t rs,
                      const float* y, const float* q, int64_t qs, int64_t n, float* stats,
                      hipStream_t st);
int launch_layernorm_fwd(const float* x, int64_t ldx, int64_t rows, int n, const float* gamma,
                         const float* beta, float eps, float* y, int64_t ldy, float* mean,
                         float* rstd, hipStream_t st);
int launch_layernorm_bwd(const float* dy, int64_t ldg, const float* x, int64_t ldx,
                         const float* mean, const float* rstd, const float* gamma, int64_t rows,
                         int n, int relu, float* dx, int64_t lddx, float* dgamma, float* dbeta,
                         hipStream_t st);
int launch_mlp3_stacked(const float* P, int64_t pstride, const int64_t* o6, int in, int h1, int h2,
                        int out, int act_out, const float* x, int64_t ldx, int n, float* y,
                        int64_t ldy, hipStream_t st);
// ---- dqn_kernels.hip
int launch_dqn_td(const float* adv, int64_t lda, const float* adv_n, int64_t ldn,
                  const float* adv_t, int64_t ldt, const float* val, int64_t vs,
                  const float* val_n, int64_t vns, const float* val_t, int64_t vts,
                  const float* actions, int64_t as, const float* rewards, int64_t rs,
                  const float* dones, int64_t ds, const float* w, int64_t B, int64_t B_global,
                  int64_t row0, int A, float gamma, int dueling, int double_q, float* dadv,
                  int64_t ldd, float* dval, float* td_all, float* y_out, float* stats,
                  hipStream_t st);
int launch_dqn_greedy(const float* adv, int64_t lda, const float* val, int64_t vs, int64_t rows,
                      int A, int dueling, int32_t* out, hipStream_t st);
// ---- conv_kernels.hip (one general convolution layer; arguments checked by the caller)
// skip: device stop flag (a launch whose flag is set writes nothing; NULL: run).
// rows: the uint8 images come through the learners' time-major row map
// (row n = t B + b: pix[b][t] | pix_next[b]) and x is ignored.
int conv2d_forward(const void* x, int x_u8, int div255, int64_t n, const ConvGeom& g,
                   const float* wgt, const float* bias, int act, float* y, hipStream_t st,
                   const int* skip = nullptr, const PixRows* rows = nullptr);
int conv2d_backward_input(const float* dy, int64_t n, const ConvGeom& g, const float* wgt,
                          const float* mask, float* dx, hipStream_t st, const int* skip = nullptr);
// part: conv_scratch_bytes(g, n) of scratch, written before it is read
int conv2d_backward_weight(const float* dy, const void* x, int x_u8, int div255, int64_t n,
                           const ConvGeom& g, float* dw, float* db, float* part, hipStream_t st,
                           const int* skip = nullptr, const PixRows* rows = nullptr);
// ---- stem.hip (the pixel stem of free shape: fused or general, stem_plan.hpp)
// A[i]: activation of layer i, [rows][act[i]] (the fused form takes A[0] == NULL
// when no backward follows); feat [rows][F] at ldf
int stem_forward(const StemPlan& p, const float* prm, const PixRows& pr, int64_t rows,
                 float* const* A, float* feat, int64_t ldf, hipStream_t st, const int* skip);
// dz: gradient at the Linear pre-activation (ReLU mask applied), rows x F at
// lddz; writes the whole gradient (not accumulated) into grad in the planner's
// layout; dA[i] ([rows][act[i]]; the fused form reads dA[n - 1] alone) and part
// (stem_part_floats) are scratch, written before they are read
int stem_backward(const StemPlan& p, const float* prm, const PixRows& pr, int64_t rows,
                  const float* const* A, const float* dz, int64_t lddz, float* grad,
                  float* const* dA, float* part, hipStream_t st, const int* skip);
// ---- linear_kernels.hip
int launch_linear_fwd_cat(const float* X, int64_t ldx, int M, int K, const float* W, int64_t ldw,
                          const float* b, int N, int act, float* Y, int64_t ldy, const float* S,
                          int64_t lds, int xcols, hipStream_t st);
// ---- head_kernels.hip
bool head_fused_ok(int in, int64_t ldx, int h1, int h2, int out, const float* X,
                   const float* W1, const float* W2, const float* W3);
int launch_head_fwd_fused(const float* X, int64_t ldx, int64_t rows, int in, const float* W1,
                          const float* b1, int h1, const float* W2, const float* b2, int h2,
                          const float* W3, const float* b3, int out, int tanh_out, float* HA1,
                          float* HA2, float* Y, int64_t ldy, float* W1T, float* W2T,
                          hipStream_t st, const int* skip, const float* vret = nullptr,
                          float* vgrad = nullptr, float vscale = 0.f, double* vpart = nullptr);
int launch_head_bwd_fused(const float* dZ, int out, int64_t rows, const float* W3,
                          const float* W2T, const float* W1T, int h1, int h2, int dx0, int dxn,
                          const float* HA1, const float* HA2, float* dH2, float* dH1, float* dX,
                          int64_t lddx, const float* mask, int64_t ldm, hipStream_t st,
                          const int* skip, const PolRowArgs* pg = nullptr);
// ---- lstm_mfma.hip
bool lstm_fwd_x_dual_fits(int B0, int B1, int S, int H, int din);
int launch_lstm_fwd_x_dual(const LstmFwdArgs& a0, const LstmFwdArgs& a1, hipStream_t st);
// ---- ppo_rnn_kernels.hip
int launch_zfilter_tmajor(const float* obs, const float* obs_next, int B, int T, int S, int D,
                          int use_zf, const float* zs, const float* zq, const float* zc, float eps,
                          float* out, int ldo, int form, hipStream_t st);
// ---- sampler_kernels.hip
void mt_seed_host(uint64_t seed, uint32_t* st);
int mt_randint_host(uint32_t* st, int64_t n, int64_t batch, int64_t* out);
int launch_mt_randint(uint32_t* st, int64_t n, int64_t batch, int64_t* out, hipStream_t s);
int launch_gather_rows(const float* table, int64_t cols, const int64_t* idx, int64_t batch,
                       float* out, hipStream_t s);
int launch_replay_gather(const float* table, int64_t cols, const uint8_t* frames,
                         const uint8_t* frames_next, int64_t frame_bytes, const int64_t* idx,
                         int64_t batch, float* rows_out, uint8_t* pix_out, uint8_t* pix_next_out,
                         hipStream_t s);
int launch_replay_gather_shared(const float* table, int64_t cols, const uint8_t* store,
                                const int32_t* fid, int stack, int64_t fbytes, const int64_t* idx,
                                int64_t batch, float* rows_out, uint8_t* pix_out,
                                uint8_t* pix_next_out, hipStream_t s);
int launch_replay_insert_shared(float* table, int64_t cols, int32_t* fid, int stack, uint8_t* store,
                                int64_t fbytes, int64_t memory_size, int64_t first_slot,
                                const float* rows, const int32_t* ids, int64_t n,
                                const uint8_t* frames, const int32_t* fslots, int64_t m,
                                hipStream_t s);
// ---- per_kernels.hip
int per_init_host(double* tree, int64_t cap);
int per_set_host(double* tree, int64_t cap, const int64_t* idx, const double* leaf, int64_t n);
int per_sample_host(const double* tree, int64_t cap, int64_t len, uint32_t* st, int64_t batch,
                    double beta, int64_t* idx_out, float* w_out);
int launch_per_init(double* tree, int64_t cap, hipStream_t s);
int launch_per_set(double* tree, int64_t cap, const int64_t* idx, const double* leaf, int64_t n,
                   hipStream_t s);
int launch_per_insert(double* tree, int64_t cap, int64_t first_slot, int64_t n, int64_t memory_size,
                      double alpha, hipStream_t s);
int launch_per_update_td(double* tree, int64_t cap, const int64_t* idx, const float* td,
                         int64_t td_stride, int64_t n, double eps, double alpha, hipStream_t s);
int launch_per_sample(const double* tree, int64_t cap, int64_t len, uint32_t* st, int64_t batch,
                      double beta, int64_t* idx_out, float* w_out, hipStream_t s);

}  // namespace smi
