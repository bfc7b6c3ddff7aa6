// dqn_kernels.hip — the DQN-specific part of DQNLearner._optimize
// (surreal/learner/dqn.py:50-71) and of QAgent.act (surreal/agent/q_agent.py:
// 42-46); the dense layers run on linear_kernels.hip.
//
//   dqn_td<DUELING, DOUBLE_Q>   dueling combination of the three score matrices
//                   (q_net.py:55-63), double-Q arg-max and gather (dqn.py:53-61),
//                   Bellman target (dqn.py:63-67), TD error, Huber loss and its
//                   gradient w.r.t. the online net's outputs, in ONE launch
//                   smi_dqn_td_shard runs the SAME kernel on one rank's rows
//                   [row0, row0 + B) of a global batch of B_global rows
//                   (data-parallel DQN); smi_dqn_td is B_global = B, row0 = 0
//   dqn_greedy<DUELING>   the same combination and arg-max rule over one score
//                   matrix: int32 action per row (the agent's acting)
//
// Per row, fp32, in this operation order (no contraction into fma):
//   dueling   m = (a_0 + a_1 + ... + a_{A-1}) / A   summed left to right
//             q_j = (a_j - m) + v                    (action_scores -= mean;
//                                                     action_scores + state_score)
//   otherwise q_j = a_j
//   j*  = the FIRST index of the maximum (left-to-right scan with >) of the
//         online net's q(s') with DOUBLE_Q, of the target net's otherwise
//         (torch.max(1) returns the first maximal index on the CPU)
//   q'  = q_target(s')[j*]
//   y   = r + gamma * ((1 - d) * q')
//   td  = q(s)[a] - y
//   l   = 0.5 td^2 if |td| < 1 else |td| - 0.5
//   g   = (w * clamp(td, -1, 1)) / B                 (w == NULL: w = 1, same bits)
//   dadv[j] = g * ([j == a] - 1/A) (dueling) | g * [j == a];  dval = g
//   stats = { mean(w l), mean |td| }, fixed-order fp64 block sums
// A shard (B rows of B_global) differs in three places only:
//   g     = (w * clamp(td)) / B_global: the plain SUM of the ranks' gradients is
//           the gradient of mean(w * l) over the global batch.
//   td    goes to td_all[row0 + i]; every other entry of td_all[0, B_global) is
//           written +0.0f by the same launch.  A SUM all-reduce of the ranks'
//           td_all is then an exact all-gather: each entry is x + 0 + ... + 0 in
//           some order, which is x in IEEE arithmetic for every x (NaN and Inf
//           included) except x = -0.0, which comes out +0.0 (priorities read
//           |td|, so they do not see it).
//   stats = the shard's fixed-order fp64 sums / B_global: the ranks' values sum
//           to the global means.
// dadv, dval and y_out stay shard-local ([B] rows).
//
// Decisions where the reference's text does not settle it:
//   1. U.huber_loss_per_element is not defined in the reference; it is read as
//      the openai/baselines huber_loss with delta 1 (above).
//   2. q_func.clip_grad_norm is torch.nn.utils.clip_grad_norm_ (L2 over all
//      q_func parameters): smi_adam_clip's max_norm.
//   3. An action value outside [0, A) is a caller error; the index is clamped
//      into [0, A) (NaN -> 0, fractions truncated), so nothing outside the A
//      columns is read or written.
// One workgroup loops over the rows (as mse_grad_weighted_kernel): the batch is
// a few hundred rows of A <= ~20 scores, and the statistics need one fixed-order
// sum; the launch is latency bound.
#include "smi_device.hpp"
#include "smi_internal.hpp"

namespace smi {

struct DqnTdArgs {
  const float* adv; int64_t lda;
  const float* adv_n; int64_t ldn;
  const float* adv_t; int64_t ldt;
  const float* val; int64_t vs;
  const float* val_n; int64_t vns;
  const float* val_t; int64_t vts;
  const float* act; int64_t as;
  const float* rew; int64_t rs;
  const float* done; int64_t ds;
  const float* w;
  int64_t B; int A; float gamma;
  int64_t Bg, row0;        // the global batch and the shard's first row in it (whole batch: B, 0)
  float* dadv; int64_t ldd;
  float* dval; float* td; float* y; float* stats;
};

// mean of one score row, summed left to right
__device__ __forceinline__ float dqn_row_mean(const float* __restrict__ a, int A) {
#pragma clang fp contract(off)
  float s = a[0];
  for (int j = 1; j < A; ++j) s = s + a[j];
  return s / (float)A;
}

template <bool DUELING>
__device__ __forceinline__ float dqn_q(const float* __restrict__ a, int j, float m, float v) {
#pragma clang fp contract(off)
  return DUELING ? (a[j] - m) + v : a[j];
}

// first index of the maximum of q_j over one row
template <bool DUELING>
__device__ __forceinline__ int dqn_argmax(const float* __restrict__ a, int A, float m, float v) {
  int best = 0;
  float qb = dqn_q<DUELING>(a, 0, m, v);
  for (int j = 1; j < A; ++j) {
    const float q = dqn_q<DUELING>(a, j, m, v);
    if (q > qb) { qb = q; best = j; }
  }
  return best;
}

__device__ __forceinline__ int dqn_action_index(float af, int A) {
  if (!(af >= 0.f)) return 0;                     // negative or NaN
  return af < (float)A ? (int)af : A - 1;
}

template <bool DUELING, bool DOUBLE_Q>
__global__ void __launch_bounds__(kWG) dqn_td_kernel(DqnTdArgs p) {
#pragma clang fp contract(off)
  __shared__ double scr[kNW];
  const int A = p.A;
  const float Bf = (float)p.Bg, invA = 1.f / (float)A;
  double sl = 0.0, st = 0.0;
  // the other ranks' entries of td_all (none for the whole batch): disjoint from
  // the rows written below
  for (int64_t i = threadIdx.x; i < p.Bg - p.B; i += kWG)
    p.td[i < p.row0 ? i : i + p.B] = 0.f;
  for (int64_t i = threadIdx.x; i < p.B; i += kWG) {
    const float* a = p.adv + i * p.lda;
    const float* at = p.adv_t + i * p.ldt;
    const int ai = dqn_action_index(p.act[i * p.as], A);
    float m = 0.f, v = 0.f, mt = 0.f, vt = 0.f;
    if (DUELING) {
      m = dqn_row_mean(a, A);
      v = p.val[i * p.vs];
      mt = dqn_row_mean(at, A);
      vt = p.val_t[i * p.vts];
    }
    const float q_sa = dqn_q<DUELING>(a, ai, m, v);
    int js;
    if (DOUBLE_Q) {
      const float* an = p.adv_n + i * p.ldn;
      float mn = 0.f, vn = 0.f;
      if (DUELING) {
        mn = dqn_row_mean(an, A);
        vn = p.val_n[i * p.vns];
      }
      js = dqn_argmax<DUELING>(an, A, mn, vn);
    } else {
      js = dqn_argmax<DUELING>(at, A, mt, vt);
    }
    const float qn = dqn_q<DUELING>(at, js, mt, vt);
    const float y = p.rew[i * p.rs] + p.gamma * ((1.f - p.done[i * p.ds]) * qn);
    const float td = q_sa - y;
    const float ab = fabsf(td);
    const float l = ab < 1.f ? 0.5f * (td * td) : ab - 0.5f;
    const float c = td > 1.f ? 1.f : (td < -1.f ? -1.f : td);
    const float wi = p.w ? p.w[i] : 1.f;
    const float g = (wi * c) / Bf;
    float* da = p.dadv + i * p.ldd;
    for (int j = 0; j < A; ++j) {
      const float e = j == ai ? 1.f : 0.f;
      da[j] = DUELING ? g * (e - invA) : g * e;
    }
    if (DUELING) p.dval[i] = g;
    p.td[p.row0 + i] = td;
    if (p.y) p.y[i] = y;
    sl += (double)(wi * l);
    st += (double)ab;
  }
  sl = block_sum_d(sl, scr);
  st = block_sum_d(st, scr);
  if (threadIdx.x == 0) {
    p.stats[0] = (float)(sl / (double)p.Bg);
    p.stats[1] = (float)(st / (double)p.Bg);
  }
}

template <bool DUELING>
__global__ void __launch_bounds__(kWG)
dqn_greedy_kernel(const float* __restrict__ adv, int64_t lda, const float* __restrict__ val,
                  int64_t vs, int64_t rows, int A, int32_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * kWG + threadIdx.x; i < rows;
       i += (int64_t)gridDim.x * kWG) {
    const float* a = adv + i * lda;
    float m = 0.f, v = 0.f;
    if (DUELING) {
      m = dqn_row_mean(a, A);
      v = val[i * vs];
    }
    out[i] = dqn_argmax<DUELING>(a, A, m, v);
  }
}

int launch_dqn_td(const float* adv, int64_t lda, const float* adv_n, int64_t ldn,
                  const float* adv_t, int64_t ldt, const float* val, int64_t vs,
                  const float* val_n, int64_t vns, const float* val_t, int64_t vts,
                  const float* actions, int64_t as, const float* rewards, int64_t rs,
                  const float* dones, int64_t ds, const float* w, int64_t B, int64_t B_global,
                  int64_t row0, int A, float gamma, int dueling, int double_q, float* dadv,
                  int64_t ldd, float* dval, float* td_all, float* y_out, float* stats,
                  hipStream_t st) {
  const DqnTdArgs p{adv, lda, adv_n, ldn, adv_t, ldt, val, vs, val_n, vns, val_t, vts, actions, as,
                    rewards, rs, dones, ds, w, B, A, gamma, B_global, row0, dadv, ldd, dval,
                    td_all, y_out, stats};
  if (dueling && double_q) {
    hipLaunchKernelGGL((dqn_td_kernel<true, true>), dim3(1), dim3(kWG), 0, st, p);
    return check_launch("dqn_td_kernel<1,1>");
  }
  if (dueling) {
    hipLaunchKernelGGL((dqn_td_kernel<true, false>), dim3(1), dim3(kWG), 0, st, p);
    return check_launch("dqn_td_kernel<1,0>");
  }
  if (double_q) {
    hipLaunchKernelGGL((dqn_td_kernel<false, true>), dim3(1), dim3(kWG), 0, st, p);
    return check_launch("dqn_td_kernel<0,1>");
  }
  hipLaunchKernelGGL((dqn_td_kernel<false, false>), dim3(1), dim3(kWG), 0, st, p);
  return check_launch("dqn_td_kernel<0,0>");
}

int launch_dqn_greedy(const float* adv, int64_t lda, const float* val, int64_t vs, int64_t rows,
                      int A, int dueling, int32_t* out, hipStream_t st) {
  int64_t g = (rows + kWG - 1) / kWG;
  g = g < 1 ? 1 : (g > 1024 ? 1024 : g);
  if (dueling) {
    hipLaunchKernelGGL((dqn_greedy_kernel<true>), dim3((unsigned)g), dim3(kWG), 0, st, adv, lda,
                       val, vs, rows, A, out);
    return check_launch("dqn_greedy_kernel<1>");
  }
  hipLaunchKernelGGL((dqn_greedy_kernel<false>), dim3((unsigned)g), dim3(kWG), 0, st, adv, lda,
                     val, vs, rows, A, out);
  return check_launch("dqn_greedy_kernel<0>");
}

}  // namespace smi
