// dqn_quant_kernels.hip — the quantile-regression head (QR-DQN, Dabney et al.
// 2018) of DQNLearner / QAgentBatch: what dqn_dist_kernels.hip does for a
// categorical distribution on a fixed support, for N quantile values per
// action and no support at all.  The reference has no distributional DQN; the
// specification below is this project's own.
//
//   qr_td<DUELING, DOUBLE_Q, HUBER>   dueling quantiles of the three head slabs,
//                   their means Q, the (double-Q) arg-max, the Bellman targets
//                   T, the pairwise quantile-Huber loss over every (online
//                   quantile i, target quantile j) and its gradient w.r.t. the
//                   online net's outputs, in ONE launch, in one of two forms
//                   (below); smi_dqn_qr_td_shard runs the SAME kernels on one
//                   rank's rows [row0, row0 + B) of a global batch of B_global
//   qr_q<DUELING>   Q [rows][A] = the mean quantiles and (optionally) the first
//                   arg-max per row (FFQfunc.forward, the agent's acting), in
//                   the same two forms and with the same device functions
//   the statistics launch is the categorical unit's (launch_dqn_dist_stats)
//
// Shapes: A actions, N quantiles, 1 <= N <= 256, A N <= 4096.  A head slab is
// [rows][ld >= A N], action major: column a N + i is quantile i of action a; a
// state slab is [rows][ld >= N].  Per row, fp32, in this operation order (no
// contraction into fma):
//   dueling   mean_i = (adv[0,i] + ... + adv[A-1,i]) / A   left to right, per quantile
//             theta[a,i] = (adv[a,i] - mean_i) + val[i]
//   otherwise theta = adv
//   Q[a]    = (sum_i theta[a,i]) / N.  The sum: lane l (0..63) adds, starting
//             from +0, the quantiles i = l, l + 64, l + 128, l + 192 below N in
//             ascending order (one term for N <= 64); the 64 lane sums (0 for a
//             lane without a quantile) then go through the xor butterfly
//             (offsets 32, 16, ..., 1)
//   a*      = the FIRST index of the maximum of Q(s') (left-to-right scan with >),
//             of the online net with DOUBLE_Q, of the target net otherwise
//   T_j     = r + gamma * ((1 - d) * theta_target(s')[a*, j])
//   tau_i   = (float)(2 i + 1) / (float)(2 N);   1 - tau_i = 1.f - tau_i
//   u_ij    = T_j - theta(s)[a_taken, i]          a_taken through dqn_action_index
//   c_ij    = u_ij < 0 ? 1 - tau_i : tau_i        (= |tau_i - [u_ij < 0]|, exactly)
//   kappa > 0 (HUBER):
//     h_ij  = |u_ij| <= kappa ? 0.5 * (u_ij * u_ij) : kappa * (|u_ij| - 0.5 * kappa)
//     k_ij  = u_ij < -kappa ? -kappa : (u_ij > kappa ? kappa : u_ij)      (the clamp)
//     S_i   = (sum_j c_ij * h_ij) / kappa,  G_i = (sum_j c_ij * k_ij) / kappa
//             (the division by kappa is taken out of the sums: once per i)
//   kappa == 0 (the pinball loss, QR-DQN-0):
//     S_i   = sum_j c_ij * |u_ij|,  G_i = sum_j c_ij * sign(u_ij), sign(0) = 0
//   both inner sums run j = 0, 1, ..., N - 1 (ascending) in two levels: each
//   run of 8 consecutive targets (the last one shorter) is added in fp32 from
//   +0, the run sums are added in fp64 from +0 in ascending order, and the
//   result is rounded to fp32 once.  (One fp32 chain over 200 targets of a
//   clipped row adds the same c_ij 200 times: its rounding bias grows with N
//   and was measured at 2.5e-6 of the gradient's scale, outside the test bar.)
//   loss    = (W_0 + W_1 + W_2 + W_3) / N, left to right, where W_k is the xor
//             butterfly (offsets 32, ..., 1) over the 64 values S_i, i = 64 k ..
//             64 k + 63 (0 for i >= N): sum over the online quantiles, mean
//             over the target ones.  (N <= 64: loss = W_0 / N, the same bits)
//   td[row] = loss   (>= 0; what PrioritizedReplay.update_priorities_from_td reads)
//   g_i     = (w * (-(G_i / N))) / B               (w == NULL: w = 1, same bits)
//             no gradient flows through the indicator or through T
//   dadv[a',i] = g_i * ([a' == a_taken] - 1/A), dval[i] = g_i     (dueling)
//   dadv[a_taken,i] = g_i, 0 for the other actions                (otherwise)
//   stats = { mean(w loss), mean(loss) }, fixed-order fp64 sums
// NaN and inf: every select above keeps a NaN u (both compares are false, the
// last operand is u or a product with it), so a NaN reward or done makes every
// T_j, every u_ij and with them the row's td, all its gradients and the stats
// NaN, never a finite priority; a NaN target quantile at a* does the same; a
// NaN online quantile i of the action taken reaches td and g_i (with dueling a
// NaN anywhere in column i does); a NaN weight reaches the row's gradients and
// stats[0] only.  An infinite reward gives td = +inf (not finite either) and,
// with kappa > 0, the clamped finite gradient.  A NaN Q never compares
// greater, so the arg-max scan steps over it (and keeps it when it is action
// 0); what a* is then is not specified.  A shard differs in the three places
// smi_dqn_td_shard documents: g divides by B_global, td goes to
// td_all[row0 + i] with +0.0f written to every other entry of td_all, and the
// statistics are the shard's sums / B_global; its rows have the whole batch's
// bits.
//
// Work split (reasoning from the code; measured figures: DESIGN.md §6).  The
// pair loop is a subtract, three compares with selects, and four multiplies
// and two adds written out (contraction off) on one u per lane: there is no
// GEMM in it, so no MFMA.  The host picks one of two forms from N alone:
//   N <= 64  one WAVE per row, four rows per workgroup, one LANE per online
//            quantile.  Each wave stages one net's A N slab of its row in its
//            own LDS region (dqn_copy_slab<64>, wave-scope ordering), reuses it
//            for the three nets, and reads it twice (the dueling mean, then
//            theta).  T_j sits in one register per lane and reaches the j loop
//            by a wave-uniform v_readlane.  A workgroup owns a fixed block of
//            rows (dqn_rows_per_block) and writes one statistics slot.
//   N > 64   one WORKGROUP per row.  The four waves stage the slab once per
//            net (dqn_copy_slab<256>, workgroup barriers), thread t holds the
//            dueling mean and val of quantile t, wave k computes Q[a] for the
//            actions a = k, k + 4, ... from LDS, every thread scans the A
//            values for a*, and thread j writes T_j to LDS behind one barrier.
//            Wave k then owns the online quantiles 64 k .. 64 k + 63, one per
//            lane, and runs the j loop over all N targets, reading T_j with
//            the same address in every lane (an LDS broadcast).  One
//            statistics slot per row.
// In both the staging form is ONE decision per launch, made on the host: 16
// byte loads (and dwords for the last A N % 4 outputs) when every head slab
// the form reads (adv, adv_target, and adv_next with DOUBLE_Q) has a 16-byte
// aligned base and a leading dimension that is a multiple of 4, dword loads
// for all of them otherwise.  Lanes past N carry neutral values (theta 0, S 0)
// and never store.
#include <math.h>
#include <stdio.h>
#include "smi_device.hpp"
#include "smi_internal.hpp"
#include "dqn_rows.hpp"

namespace smi {

constexpr int kQrMaxN = 256;                     // one thread of a workgroup per quantile
constexpr int kQrMaxSlab = 4096;                 // A N: 4 wave slabs of 16 KiB in the first form
constexpr int kQrWaveN = 64;                     // N up to here: one wave per row

struct QrTdArgs {
  const float* adv; int64_t lda;
  const float* adv_n; int64_t ldn;
  const float* adv_t; int64_t ldt;
  const float* val; int64_t ldv;
  const float* val_n; int64_t ldvn;
  const float* val_t; int64_t ldvt;
  const float* act; int64_t as;
  const float* rew; int64_t rs;
  const float* done; int64_t ds;
  const float* w;
  int64_t B; int A, N; float kappa, gamma;
  int64_t Bg, row0;        // the global batch and the shard's first row in it (whole batch: B, 0)
  int rpb;                 // first form: rows per workgroup, a multiple of kNW
  int vec;                 // every slab row is 16-byte aligned
  float* dadv; int64_t ldd;
  float* dval; int64_t lddv;
  float* td; float* t_out; int32_t* astar; double* partials;
};

// theta[a, i] of a staged slab (i < N)
template <bool DUELING>
__device__ __forceinline__ float qr_theta(const float* __restrict__ slab, int a, int N, int i,
                                          float mean, float v) {
#pragma clang fp contract(off)
  const float x = slab[a * N + i];
  return DUELING ? (x - mean) + v : x;
}

// ---- first form: a wave per row.  First index of the maximum of Q[a] over the
// wave's staged slab; q_out (may be NULL) receives the A means
template <bool DUELING>
__device__ __forceinline__ int qr_wave_argmax(const float* __restrict__ slab, int A, int N,
                                              int lane, float mean, float v,
                                              float* __restrict__ q_out) {
#pragma clang fp contract(off)
  const float fN = (float)N;
  int best = 0;
  float qb = 0.f;
  for (int a = 0; a < A; ++a) {
    const float th = lane < N ? 0.f + qr_theta<DUELING>(slab, a, N, lane, mean, v) : 0.f;
    const float q = wave_sum(th) / fN;
    if (q_out && lane == 0) q_out[a] = q;
    if (a == 0) qb = q;
    else if (q > qb) { qb = q; best = a; }
  }
  return best;
}

// ---- second form: a workgroup per row.  What its kernels keep in LDS next to
// the slab: the dueling means and vals of the N quantiles, the targets, the A
// means and the waves' loss sums
struct QrRowLds {
  float mean[kQrMaxN], val[kQrMaxN], T[kQrMaxN], Q[kQrWaveN], W[kNW];
};

// stage one net's row; thread t leaves with the dueling mean and val of
// quantile t (0, 0 without dueling or past N)
template <bool DUELING>
__device__ __forceinline__ void qr_row_stage(const float* __restrict__ adv_row,
                                             const float* __restrict__ val_row, int A, int N,
                                             int vec, float* __restrict__ slab, int t, float& mean,
                                             float& v) {
  __syncthreads();                               // the previous net's reads are done
  dqn_copy_slab<kWG>(adv_row, A * N, vec, slab, t);
  __syncthreads();
  mean = dqn_col_mean<DUELING>(slab, A, N, t);
  v = DUELING && t < N ? val_row[t] : 0.f;
}

// Q[0..A) of the staged row into L.Q (wave k: the actions k, k + 4, ...) and
// the first index of their maximum, in every thread
template <bool DUELING>
__device__ __forceinline__ int qr_row_argmax(const float* __restrict__ slab, int A, int N, int t,
                                             float mean, float v, QrRowLds& L,
                                             float* __restrict__ q_out) {
#pragma clang fp contract(off)
  const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const float fN = (float)N;
  if (DUELING) { L.mean[t] = mean; L.val[t] = v; }
  __syncthreads();
  for (int a = wave; a < A; a += kNW) {
    float part = 0.f;
    for (int i = lane; i < N; i += 64)
      part = part + qr_theta<DUELING>(slab, a, N, i, DUELING ? L.mean[i] : 0.f,
                                      DUELING ? L.val[i] : 0.f);
    const float q = wave_sum(part) / fN;
    if (lane == 0) {
      L.Q[a] = q;
      if (q_out) q_out[a] = q;
    }
  }
  __syncthreads();
  int best = 0;
  float qb = L.Q[0];
  for (int a = 1; a < A; ++a) {
    const float q = L.Q[a];
    if (q > qb) { qb = q; best = a; }
  }
  return best;
}

// (qr_pairs, the sums of one online quantile over the targets: dqn_rows.hpp)

// one quantile's gradient into the row's dadv / dval
template <bool DUELING>
__device__ __forceinline__ void qr_store_grad(const QrTdArgs& p, int64_t row, int i, int ai,
                                              float G, float wi) {
#pragma clang fp contract(off)
  const int A = p.A, N = p.N;
  const float invA = 1.f / (float)A;
  const float g = (wi * (-(G / (float)N))) / (float)p.Bg;
  float* da = p.dadv + row * p.ldd + i;
  for (int a = 0; a < A; ++a) {
    const float e = a == ai ? 1.f : 0.f;
    da[a * N] = DUELING ? g * (e - invA) : (a == ai ? g : 0.f);
  }
  if (DUELING) p.dval[row * p.lddv + i] = g;
}

// the other ranks' entries of td_all (none for the whole batch): disjoint from
// the rows the launch writes
__device__ __forceinline__ void qr_zero_other_td(const QrTdArgs& p) {
  for (int64_t i = (int64_t)blockIdx.x * kWG + threadIdx.x; i < p.Bg - p.B;
       i += (int64_t)gridDim.x * kWG)
    p.td[i < p.row0 ? i : i + p.B] = 0.f;
}

template <bool DUELING, bool DOUBLE_Q, bool HUBER>
__global__ void __launch_bounds__(kWG) qr_td_wave_kernel(QrTdArgs p) {
#pragma clang fp contract(off)
  extern __shared__ float4 qr_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int A = p.A, N = p.N, AN = A * N, region = round4(AN);
  float* slab = reinterpret_cast<float*>(qr_lds) + wave * region;
  const bool on = lane < N;
  const float tau = (float)(2 * lane + 1) / (float)(2 * N);
  qr_zero_other_td(p);
  const int64_t r0 = (int64_t)blockIdx.x * p.rpb;
  double sl = 0.0, st = 0.0;                     // thread 0: this block's sums, rows ascending
  for (int it = 0; it < p.rpb / kNW; ++it) {
    const int64_t row = r0 + (int64_t)it * kNW + wave;
    double rl = 0.0, rt = 0.0;
    if (row < p.B) {
      // ---- a* : first maximum of Q(s') of the selecting net
      int astar = 0;
      if (DOUBLE_Q) {
        dqn_wave_sync();                         // the previous row's reads are done
        dqn_copy_slab<64>(p.adv_n + row * p.ldn, AN, p.vec, slab, lane);
        dqn_wave_sync();
        const float vn = DUELING && on ? p.val_n[row * p.ldvn + lane] : 0.f;
        const float mn = dqn_col_mean<DUELING>(slab, A, N, lane);
        astar = qr_wave_argmax<DUELING>(slab, A, N, lane, mn, vn, nullptr);
      }
      // ---- T = r + gamma (1 - d) theta_target(s')[a*, .], one target per lane
      dqn_wave_sync();
      dqn_copy_slab<64>(p.adv_t + row * p.ldt, AN, p.vec, slab, lane);
      dqn_wave_sync();
      const float vt = DUELING && on ? p.val_t[row * p.ldvt + lane] : 0.f;
      const float mt = dqn_col_mean<DUELING>(slab, A, N, lane);
      if (!DOUBLE_Q) astar = qr_wave_argmax<DUELING>(slab, A, N, lane, mt, vt, nullptr);
      const float r = p.rew[row * p.rs], d = p.done[row * p.ds];
      const float tt = on ? qr_theta<DUELING>(slab, astar, N, lane, mt, vt) : 0.f;
      const float T = r + p.gamma * ((1.f - d) * tt);
      // ---- the pairs against the online net's quantiles of the action taken
      dqn_wave_sync();
      dqn_copy_slab<64>(p.adv + row * p.lda, AN, p.vec, slab, lane);
      dqn_wave_sync();
      const float v = DUELING && on ? p.val[row * p.ldv + lane] : 0.f;
      const float mean = dqn_col_mean<DUELING>(slab, A, N, lane);
      const int ai = dqn_action_index(p.act[row * p.as], A);
      const float th = on ? qr_theta<DUELING>(slab, ai, N, lane, mean, v) : 0.f;
      const QrSums s = qr_pairs<HUBER>(th, tau, p.kappa, N, [&](int j) { return dqn_lane(T, j); });
      const float loss = wave_sum(on ? s.S : 0.f) / (float)N;
      const float wi = p.w ? p.w[row] : 1.f;
      if (on) {
        qr_store_grad<DUELING>(p, row, lane, ai, s.G, wi);
        if (p.t_out) p.t_out[row * N + lane] = T;
      }
      if (lane == 0) {
        p.td[p.row0 + row] = loss;
        if (p.astar) p.astar[row] = astar;
      }
      rl = (double)(wi * loss);
      rt = (double)loss;
    }
    // the waves' {w loss, loss} meet in the first 16 bytes of their slab regions
    // (the LDS of a workgroup is the four slabs and nothing else: 64 KiB at A N
    // = 4096): a barrier before thread 0 reads them, one before they are staged over
    dqn_wave_sync();
    if (lane == 0) {
      double* s = reinterpret_cast<double*>(slab);
      s[0] = rl;
      s[1] = rt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int w = 0; w < kNW; ++w) {
        const double* s = reinterpret_cast<const double*>(reinterpret_cast<float*>(qr_lds) + w * region);
        sl += s[0];
        st += s[1];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    p.partials[2 * blockIdx.x] = sl;
    p.partials[2 * blockIdx.x + 1] = st;
  }
}

template <bool DUELING, bool DOUBLE_Q, bool HUBER>
__global__ void __launch_bounds__(kWG) qr_td_row_kernel(QrTdArgs p) {
#pragma clang fp contract(off)
  extern __shared__ float4 qr_lds[];
  __shared__ QrRowLds L;
  float* slab = reinterpret_cast<float*>(qr_lds);
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int A = p.A, N = p.N;
  const bool on = t < N;
  const float tau = (float)(2 * t + 1) / (float)(2 * N);
  qr_zero_other_td(p);
  const int64_t row = blockIdx.x;                // grid = B
  float mean, v;
  // ---- a* : first maximum of Q(s') of the selecting net
  int astar = 0;
  if (DOUBLE_Q) {
    qr_row_stage<DUELING>(p.adv_n + row * p.ldn, DUELING ? p.val_n + row * p.ldvn : nullptr, A, N,
                          p.vec, slab, t, mean, v);
    astar = qr_row_argmax<DUELING>(slab, A, N, t, mean, v, L, nullptr);
  }
  // ---- T_j into LDS, one target per thread
  qr_row_stage<DUELING>(p.adv_t + row * p.ldt, DUELING ? p.val_t + row * p.ldvt : nullptr, A, N,
                        p.vec, slab, t, mean, v);
  if (!DOUBLE_Q) astar = qr_row_argmax<DUELING>(slab, A, N, t, mean, v, L, nullptr);
  const float r = p.rew[row * p.rs], d = p.done[row * p.ds];
  if (on) {
    const float T = r + p.gamma * ((1.f - d) * qr_theta<DUELING>(slab, astar, N, t, mean, v));
    L.T[t] = T;
    if (p.t_out) p.t_out[row * N + t] = T;
  }
  // ---- the pairs: wave k's lanes hold the online quantiles 64 k .. 64 k + 63
  // (the barriers of the staging put T behind them)
  qr_row_stage<DUELING>(p.adv + row * p.lda, DUELING ? p.val + row * p.ldv : nullptr, A, N, p.vec,
                        slab, t, mean, v);
  const int ai = dqn_action_index(p.act[row * p.as], A);
  const float th = on ? qr_theta<DUELING>(slab, ai, N, t, mean, v) : 0.f;
  const float* Tl = L.T;
  const QrSums s = qr_pairs<HUBER>(th, tau, p.kappa, N, [&](int j) { return Tl[j]; });
  const float ws = wave_sum(on ? s.S : 0.f);
  if (lane == 0) L.W[wave] = ws;
  const float wi = p.w ? p.w[row] : 1.f;
  if (on) qr_store_grad<DUELING>(p, row, t, ai, s.G, wi);
  __syncthreads();
  if (t == 0) {
    const float loss = (((L.W[0] + L.W[1]) + L.W[2]) + L.W[3]) / (float)N;
    p.td[p.row0 + row] = loss;
    if (p.astar) p.astar[row] = astar;
    p.partials[2 * row] = (double)(wi * loss);
    p.partials[2 * row + 1] = (double)loss;
  }
}

template <bool DUELING>
__global__ void __launch_bounds__(kWG)
qr_q_wave_kernel(const float* __restrict__ adv, int64_t lda, const float* __restrict__ val,
                 int64_t ldv, int64_t rows, int A, int N, int vec, float* __restrict__ q,
                 int64_t ldq, int32_t* __restrict__ greedy) {
  extern __shared__ float4 qr_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int AN = A * N;
  float* slab = reinterpret_cast<float*>(qr_lds) + wave * round4(AN);
  for (int64_t row = (int64_t)blockIdx.x * kNW + wave; row < rows;
       row += (int64_t)gridDim.x * kNW) {
    dqn_wave_sync();
    dqn_copy_slab<64>(adv + row * lda, AN, vec, slab, lane);
    dqn_wave_sync();
    const float v = DUELING && lane < N ? val[row * ldv + lane] : 0.f;
    const float mean = dqn_col_mean<DUELING>(slab, A, N, lane);
    const int best = qr_wave_argmax<DUELING>(slab, A, N, lane, mean, v, q + row * ldq);
    if (greedy && lane == 0) greedy[row] = best;
  }
}

template <bool DUELING>
__global__ void __launch_bounds__(kWG)
qr_q_row_kernel(const float* __restrict__ adv, int64_t lda, const float* __restrict__ val,
                int64_t ldv, int64_t rows, int A, int N, int vec, float* __restrict__ q,
                int64_t ldq, int32_t* __restrict__ greedy) {
  extern __shared__ float4 qr_lds[];
  __shared__ QrRowLds L;
  float* slab = reinterpret_cast<float*>(qr_lds);
  const int t = threadIdx.x;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    float mean, v;
    qr_row_stage<DUELING>(adv + row * lda, DUELING ? val + row * ldv : nullptr, A, N, vec, slab, t,
                          mean, v);
    const int best = qr_row_argmax<DUELING>(slab, A, N, t, mean, v, L, q + row * ldq);
    if (greedy && t == 0) greedy[row] = best;
  }
}

// ------------------------------------------------------------------- host
// one slot per row covers both forms (the first uses one per block of rows)
int64_t qr_partials_bytes(int64_t B) { return B < 1 ? 0 : B * 2 * (int64_t)sizeof(double); }

// the checks both launchers share; 0 or SMI_E_ARG with the message set
static int qr_check_shape(const char* who, int A, int N) {
  char msg[160];
  const char* why = nullptr;
  if (N < 1 || N > kQrMaxN) why = "quantiles outside [1, 256]";
  else if (A < 1) why = "A < 1";
  else if ((int64_t)A * N > kQrMaxSlab) why = "A * quantiles over 4096 (the LDS slabs of a workgroup)";
  if (!why) return SMI_OK;
  snprintf(msg, sizeof(msg), "%s: %s", who, why);
  return set_error(SMI_E_ARG, msg);
}

template <bool HUBER>
static const char* qr_td_launch(const QrTdArgs& p, bool rowform, int dueling, int double_q,
                                dim3 grid, size_t lds, hipStream_t st) {
#define QR_TD_FORM(D, Q)                                                                      \
  do {                                                                                        \
    if (rowform) {                                                                            \
      hipLaunchKernelGGL((qr_td_row_kernel<D, Q, HUBER>), grid, dim3(kWG), lds, st, p);       \
      return HUBER ? "qr_td_row_kernel<" #D "," #Q ",1>" : "qr_td_row_kernel<" #D "," #Q ",0>"; \
    }                                                                                         \
    hipLaunchKernelGGL((qr_td_wave_kernel<D, Q, HUBER>), grid, dim3(kWG), lds, st, p);        \
    return HUBER ? "qr_td_wave_kernel<" #D "," #Q ",1>" : "qr_td_wave_kernel<" #D "," #Q ",0>"; \
  } while (0)
  if (dueling && double_q) QR_TD_FORM(1, 1);
  if (dueling) QR_TD_FORM(1, 0);
  if (double_q) QR_TD_FORM(0, 1);
  QR_TD_FORM(0, 0);
#undef QR_TD_FORM
}

int launch_qr_td(const float* adv, int64_t lda, const float* adv_n, int64_t ldn,
                 const float* adv_t, int64_t ldt, const float* val, int64_t ldv,
                 const float* val_n, int64_t ldvn, const float* val_t, int64_t ldvt,
                 const float* actions, int64_t as, const float* rewards, int64_t rs,
                 const float* dones, int64_t ds, const float* w, int64_t B, int64_t B_global,
                 int64_t row0, int A, int N, float kappa, float gamma, int dueling, int double_q,
                 float* dadv, int64_t ldd, float* dval, int64_t lddv, float* td_all, float* t_out,
                 int32_t* astar_out, double* partials, int64_t partials_bytes, float* stats,
                 hipStream_t st) {
  RC_CHECK(qr_check_shape("dqn_qr_td", A, N));
  if (!(kappa >= 0.f)) return set_error(SMI_E_ARG, "dqn_qr_td: kappa < 0 or NaN");
  const int64_t AN = (int64_t)A * N;
  if (lda < AN || ldt < AN || ldd < AN || (double_q && ldn < AN) ||
      (dueling && (ldv < N || ldvt < N || lddv < N || (double_q && ldvn < N))))
    return set_error(SMI_E_ARG, "dqn_qr_td: leading dims too small");
  const bool rowform = N > kQrWaveN;
  const int64_t rpb = rowform ? 1 : dqn_rows_per_block(B, dqn_cus());
  const int64_t nb = (B + rpb - 1) / rpb;
  if (rpb > INT32_MAX || nb > INT32_MAX)
    return set_error(SMI_E_ARG, "dqn_qr_td: B over the launch grid");
  if (partials_bytes < nb * 2 * (int64_t)sizeof(double))
    return set_error(SMI_E_ARG, "dqn_qr_td: partials workspace too small "
                                "(smi_dqn_qr_partials_bytes)");
  const int vec = dqn_aligned16(adv, lda) && dqn_aligned16(adv_t, ldt) &&
                  (!double_q || dqn_aligned16(adv_n, ldn));
  const QrTdArgs p{adv, lda, adv_n, ldn, adv_t, ldt, val, ldv, val_n, ldvn, val_t, ldvt,
                   actions, as, rewards, rs, dones, ds, w, B, A, N, kappa, gamma,
                   B_global, row0, (int)rpb, vec, dadv, ldd, dval, lddv, td_all, t_out,
                   astar_out, partials};
  const size_t lds = (size_t)(rowform ? 1 : kNW) * round4((int)AN) * sizeof(float);
  const dim3 grid((unsigned)nb);
  const char* what = kappa > 0.f ? qr_td_launch<true>(p, rowform, dueling, double_q, grid, lds, st)
                                 : qr_td_launch<false>(p, rowform, dueling, double_q, grid, lds, st);
  RC_CHECK(check_launch(what));
  RC_CHECK(launch_dqn_dist_stats(partials, (int)nb, (double)B_global, stats, st));
  return check_launch(what);                     // smi_last_launch names the TD form
}

int launch_qr_q(const float* adv, int64_t lda, const float* val, int64_t ldv, int64_t rows, int A,
                int N, int dueling, float* q, int64_t ldq, int32_t* greedy, hipStream_t st) {
  RC_CHECK(qr_check_shape("dqn_qr_q", A, N));
  const int64_t AN = (int64_t)A * N;
  if (lda < AN || ldq < A || (dueling && ldv < N))
    return set_error(SMI_E_ARG, "dqn_qr_q: leading dims too small");
  const bool rowform = N > kQrWaveN;
  const int64_t cap = (int64_t)kDistBlocksPerCU * dqn_cus();
  int64_t g = rowform ? rows : (rows + kNW - 1) / kNW;
  g = g < 1 ? 1 : (g > cap ? cap : g);
  const int vec = dqn_aligned16(adv, lda);
  const size_t lds = (size_t)(rowform ? 1 : kNW) * round4((int)AN) * sizeof(float);
  const dim3 grid((unsigned)g), wg(kWG);
#define QR_Q_FORM(K, D, NAME)                                                                  \
  do {                                                                                         \
    hipLaunchKernelGGL((K<D>), grid, wg, lds, st, adv, lda, val, ldv, rows, A, N, vec, q, ldq, \
                       greedy);                                                                \
    return check_launch(NAME);                                                                 \
  } while (0)
  if (rowform && dueling) QR_Q_FORM(qr_q_row_kernel, true, "qr_q_row_kernel<1>");
  if (rowform) QR_Q_FORM(qr_q_row_kernel, false, "qr_q_row_kernel<0>");
  if (dueling) QR_Q_FORM(qr_q_wave_kernel, true, "qr_q_wave_kernel<1>");
  QR_Q_FORM(qr_q_wave_kernel, false, "qr_q_wave_kernel<0>");
#undef QR_Q_FORM
}

}  // namespace smi
