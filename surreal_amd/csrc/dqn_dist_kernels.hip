// dqn_dist_kernels.hip — the categorical (C51, Bellemare et al. 2017) head of
// DQNLearner / QAgentBatch: what dqn_kernels.hip does for one number per action,
// for a distribution over N atoms per action.  The reference has no
// distributional DQN; the specification below is this project's own.
//
//   c51_td<DUELING, DOUBLE_Q>   dueling logits of the three score slabs, softmax
//                   and expected values, (double-Q) arg-max, the projected
//                   target distribution, cross-entropy and its gradient
//                   w.r.t. the online net's outputs, in ONE launch;
//                   smi_dqn_c51_td_shard runs the SAME kernel on one rank's rows
//                   [row0, row0 + B) of a global batch of B_global rows
//   c51_stats       sums the workgroups' fp64 partials of c51_td into stats[2]
//   c51_q<DUELING>  expected values q [rows][A] and (optionally) the first
//                   arg-max action per row (FFQfunc.forward, the agent's acting)
//
// Shapes: A actions, N atoms (2 <= N <= 64), support z_i = v_min + i D,
// D = (v_max - v_min) / (N - 1).  A score slab is [rows][ld >= A N], action
// major: column a N + i is atom i of action a; a state slab is [rows][ld >= N].
// Per row, fp32, in this operation order (no contraction into fma):
//   dueling   mean_i = (adv[0,i] + ... + adv[A-1,i]) / A   left to right, per atom
//             l[a,i] = (adv[a,i] - mean_i) + val[i]
//   otherwise l = adv
//   softmax   mx_a = max_i l[a,i];  e[a,i] = exp(l[a,i] - mx_a);  S_a = sum_i e[a,i]
//             p[a,i] = e[a,i] / S_a
//   Q[a]    = (sum_i z_i e[a,i]) / S_a                 (both sums: xor butterfly)
//   a*      = the FIRST index of the maximum of Q(s') (left-to-right scan with >),
//             of the online net with DOUBLE_Q, of the target net otherwise
//   p'      = p_target(s')[a*, .]
//   Tz_j    = clamp(r + gamma * ((1 - d) * z_j), v_min, v_max);  b_j = (Tz_j - v_min) / D
//             (torch.clamp: +-inf go to the bounds, a NaN stays NaN)
//   m_i     = sum_{j = 0..N-1} p'_j * max(0, 1 - |b_j - i|)      j ascending
//             (the gather form of the textbook floor / ceil scatter, its l == u
//             corner included: no atomics, continuous in b, the same bits on
//             every rank)
//   logp_i  = (l[a_taken,i] - mx) - log(S)             (log-softmax, not log(softmax))
//   loss    = -(sum_i m_i * logp_i)                    i ascending
//   td[row] = loss   (>= 0; what PrioritizedReplay.update_priorities_from_td reads)
//   g_i     = (w * (p[a_taken,i] - m_i)) / B           (w == NULL: w = 1, same bits)
//   dadv[a',i] = g_i * ([a' == a_taken] - 1/A), dval[i] = g_i     (dueling)
//   dadv[a_taken,i] = g_i, 0 for the other actions                (otherwise)
//   stats = { mean(w loss), mean(loss) }, fixed-order fp64 sums
// NaN: a NaN reward or done makes every Tz_j, b_j and with them the whole row
// of m, its loss (td) and its gradients NaN, as the reference's torch.clamp
// does (fminf(fmaxf()) alone would return v_min and hand the sum tree a finite
// priority); a NaN weight reaches the row's gradients and stats[0] only; a NaN
// logit of the action taken reaches td and that action's gradients.  A NaN
// expected value never compares greater, so the arg-max scan steps over it
// (and keeps it when it is action 0); what a* is then is not specified.
// The action index is clamped as dqn_action_index does.  A shard differs in the
// three places smi_dqn_td_shard documents: g divides by B_global, td goes to
// td_all[row0 + i] with +0.0f written to every other entry of td_all, and the
// statistics are the shard's sums / B_global.
//
// Work split (reasoning from the code; measured figures: DESIGN.md §6): one
// WAVE per row, one LANE per atom.  A workgroup of kWG threads holds 4 rows at
// a time and owns a fixed contiguous block of rows (dqn_rows_per_block: from B
// and the CU count only; one quad of rows up to B = 16 CUs, then 2, 3, ...).
// Each wave stages one net's A N slab of its row in its own LDS region, reuses
// the region for the three nets in turn, and reads it twice.  The staging form
// is ONE decision per launch, made on the host: 16-byte loads (and dwords for
// the last A N % 4 scores) when every score slab the form reads (adv,
// adv_target, and adv_next with DOUBLE_Q) has a 16-byte aligned base and a
// leading dimension that is a multiple of 4, dword loads for all of them
// otherwise; val rows, outputs and an adv_next the form does not read have no
// say.  The two reads: the dueling mean over a, then the per-action
// softmax.  val rows, p', b and m live in one register per lane; the projection
// is N steps of a wave-uniform lane broadcast (v_readlane) and 4-5 VALU ops.
// Lanes i >= N carry -inf / 0 and never store.  Each workgroup writes
// {sum w loss, sum loss} of its rows (ascending) as fp64 into its slot of the
// caller's partials; c51_stats, a second launch of one wave, adds the slots.
#include <math.h>
#include <stdio.h>
#include "smi_device.hpp"
#include "smi_internal.hpp"
#include "dqn_rows.hpp"

namespace smi {

constexpr int kC51MaxAtoms = 64;                 // one lane per atom
constexpr int kC51LdsBytes = 48 * 1024;          // the kNW slabs of a workgroup: A N <= 3072

struct C51TdArgs {
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
  int64_t B; int A, N; float v_min, v_max, gamma;
  int64_t Bg, row0;        // the global batch and the shard's first row in it (whole batch: B, 0)
  int rpb;                 // rows per workgroup, a multiple of kNW
  int vec;                 // every slab row is 16-byte aligned
  float* dadv; int64_t ldd;
  float* dval; int64_t lddv;
  float* td; float* m_out; int32_t* astar; double* partials;
};

__device__ __forceinline__ float c51_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// torch.clamp(y, lo, hi): a NaN stays NaN (fmaxf / fminf return their other
// operand); every other input has the bits of fminf(fmaxf(y, lo), hi)
// (clamp5 of smi_device.hpp with the bounds as arguments)
__device__ __forceinline__ float c51_clamp(float y, float lo, float hi) {
  return y != y ? y : fminf(fmaxf(y, lo), hi);
}

// one row's A N scores into the wave's LDS region (dqn_copy_slab, ordered
// against the wave's reads of the previous net)
__device__ __forceinline__ void c51_stage(const float* __restrict__ src, int AN, int vec,
                                          float* __restrict__ slab, int lane) {
  dqn_wave_sync();                               // the previous net's reads are done
  dqn_copy_slab<64>(src, AN, vec, slab, lane);
  dqn_wave_sync();
}

// l[a, lane]; -inf in the lanes past the last atom
template <bool DUELING>
__device__ __forceinline__ float c51_logit(const float* __restrict__ slab, int a, int N, int lane,
                                           float mean, float v) {
#pragma clang fp contract(off)
  if (lane >= N) return -INFINITY;
  const float x = slab[a * N + lane];
  return DUELING ? (x - mean) + v : x;
}

// softmax moments of one action's logits: the row maximum, this lane's
// exp(l - mx) (0 past the last atom), their sum and the expected value
struct C51Moments { float mx, e, S, Q; };
__device__ __forceinline__ C51Moments c51_moments(float l, float z) {
#pragma clang fp contract(off)
  C51Moments o;
  o.mx = c51_wave_max(l);
  o.e = expf(l - o.mx);
  o.S = wave_sum(o.e);
  o.Q = wave_sum(z * o.e) / o.S;
  return o;
}

// first index of the maximum of Q[a] over the staged slab; q_out (may be NULL)
// receives the A expected values
template <bool DUELING>
__device__ __forceinline__ int c51_first_argmax(const float* __restrict__ slab, int A, int N,
                                                int lane, float mean, float v, float z,
                                                float* __restrict__ q_out) {
  int best = 0;
  float qb = 0.f;
  for (int a = 0; a < A; ++a) {
    const float q = c51_moments(c51_logit<DUELING>(slab, a, N, lane, mean, v), z).Q;
    if (q_out && lane == 0) q_out[a] = q;
    if (a == 0) qb = q;
    else if (q > qb) { qb = q; best = a; }
  }
  return best;
}

template <bool DUELING, bool DOUBLE_Q>
__global__ void __launch_bounds__(kWG) c51_td_kernel(C51TdArgs p) {
#pragma clang fp contract(off)
  extern __shared__ float4 c51_lds[];
  __shared__ double slot[2][kNW][2];             // per quad of rows: {w loss, loss} of each wave
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int A = p.A, N = p.N, AN = A * N;
  float* slab = reinterpret_cast<float*>(c51_lds) + wave * round4(AN);
  const bool on = lane < N;
  const float delta = (p.v_max - p.v_min) / (float)(N - 1);
  const float z = p.v_min + (float)lane * delta;
  const float Bf = (float)p.Bg, invA = 1.f / (float)A;
  // the other ranks' entries of td_all (none for the whole batch): disjoint from
  // the rows written below
  for (int64_t i = (int64_t)blockIdx.x * kWG + threadIdx.x; i < p.Bg - p.B;
       i += (int64_t)gridDim.x * kWG)
    p.td[i < p.row0 ? i : i + p.B] = 0.f;
  const int64_t r0 = (int64_t)blockIdx.x * p.rpb;
  double sl = 0.0, st = 0.0;                     // thread 0: this block's sums, rows ascending
  for (int it = 0; it < p.rpb / kNW; ++it) {
    const int64_t row = r0 + (int64_t)it * kNW + wave;
    double rl = 0.0, rt = 0.0;
    if (row < p.B) {
      // ---- a* : first maximum of Q(s') of the selecting net
      int astar = 0;
      if (DOUBLE_Q) {
        c51_stage(p.adv_n + row * p.ldn, AN, p.vec, slab, lane);
        const float vn = DUELING && on ? p.val_n[row * p.ldvn + lane] : 0.f;
        const float mn = dqn_col_mean<DUELING>(slab, A, N, lane);
        astar = c51_first_argmax<DUELING>(slab, A, N, lane, mn, vn, z, nullptr);
      }
      // ---- p' = p_target(s')[a*, .]
      c51_stage(p.adv_t + row * p.ldt, AN, p.vec, slab, lane);
      const float vt = DUELING && on ? p.val_t[row * p.ldvt + lane] : 0.f;
      const float mt = dqn_col_mean<DUELING>(slab, A, N, lane);
      if (!DOUBLE_Q) astar = c51_first_argmax<DUELING>(slab, A, N, lane, mt, vt, z, nullptr);
      const C51Moments t = c51_moments(c51_logit<DUELING>(slab, astar, N, lane, mt, vt), z);
      const float pp = t.e / t.S;
      // ---- projection onto the support, gather form
      const float r = p.rew[row * p.rs], d = p.done[row * p.ds];
      float tz = r + p.gamma * ((1.f - d) * z);
      tz = c51_clamp(tz, p.v_min, p.v_max);
      const float b = (tz - p.v_min) / delta;
      const float fi = (float)lane;
      float m = 0.f;
      for (int j = 0; j < N; ++j) {
        const float pj = dqn_lane(pp, j), bj = dqn_lane(b, j);
        const float wgt = 1.f - fabsf(bj - fi);
        // a NaN b_j stays (as act_f's relu).  One wave-wide test of b after the
        // loop with the old max here was measured and is no gain: DESIGN.md §6
        m = m + pj * (wgt <= 0.f ? 0.f : wgt);
      }
      // ---- cross-entropy against the online net's log-softmax at the action taken
      c51_stage(p.adv + row * p.lda, AN, p.vec, slab, lane);
      const float v = DUELING && on ? p.val[row * p.ldv + lane] : 0.f;
      const float mean = dqn_col_mean<DUELING>(slab, A, N, lane);
      const int ai = dqn_action_index(p.act[row * p.as], A);
      const float l = c51_logit<DUELING>(slab, ai, N, lane, mean, v);
      const C51Moments o = c51_moments(l, z);
      const float term = on ? m * ((l - o.mx) - logf(o.S)) : 0.f;
      float s = dqn_lane(term, 0);
      for (int i = 1; i < N; ++i) s = s + dqn_lane(term, i);
      const float loss = -s;
      const float wi = p.w ? p.w[row] : 1.f;
      if (on) {
        const float g = (wi * (o.e / o.S - m)) / Bf;
        float* da = p.dadv + row * p.ldd + lane;
        for (int a = 0; a < A; ++a) {
          const float e = a == ai ? 1.f : 0.f;
          da[a * N] = DUELING ? g * (e - invA) : (a == ai ? g : 0.f);
        }
        if (DUELING) p.dval[row * p.lddv + lane] = g;
        if (p.m_out) p.m_out[row * N + lane] = m;
      }
      if (lane == 0) {
        p.td[p.row0 + row] = loss;
        if (p.astar) p.astar[row] = astar;
      }
      rl = (double)(wi * loss);
      rt = (double)loss;
    }
    if (lane == 0) { slot[it & 1][wave][0] = rl; slot[it & 1][wave][1] = rt; }
    // one barrier per quad: the slots alternate, and thread 0 has read quad
    // it - 1's before it arrives here
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int w = 0; w < kNW; ++w) { sl += slot[it & 1][w][0]; st += slot[it & 1][w][1]; }
    }
  }
  if (threadIdx.x == 0) {
    p.partials[2 * blockIdx.x] = sl;
    p.partials[2 * blockIdx.x + 1] = st;
  }
}

// one wave: the slots l, l + 64, ... per lane, then the xor butterfly
__global__ void __launch_bounds__(64) c51_stats_kernel(const double* __restrict__ partials, int nb,
                                                       double Bg, float* __restrict__ stats) {
  double sl = 0.0, st = 0.0;
  for (int i = threadIdx.x; i < nb; i += 64) { sl += partials[2 * i]; st += partials[2 * i + 1]; }
  sl = wave_sum_d(sl);
  st = wave_sum_d(st);
  if (threadIdx.x == 0) {
    stats[0] = (float)(sl / Bg);
    stats[1] = (float)(st / Bg);
  }
}

template <bool DUELING>
__global__ void __launch_bounds__(kWG)
c51_q_kernel(const float* __restrict__ adv, int64_t lda, const float* __restrict__ val, int64_t ldv,
             int64_t rows, int A, int N, float v_min, float v_max, int vec, float* __restrict__ q,
             int64_t ldq, int32_t* __restrict__ greedy) {
#pragma clang fp contract(off)
  extern __shared__ float4 c51_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int AN = A * N;
  float* slab = reinterpret_cast<float*>(c51_lds) + wave * round4(AN);
  const float delta = (v_max - v_min) / (float)(N - 1);
  const float z = v_min + (float)lane * delta;
  for (int64_t row = (int64_t)blockIdx.x * kNW + wave; row < rows;
       row += (int64_t)gridDim.x * kNW) {
    c51_stage(adv + row * lda, AN, vec, slab, lane);
    const float v = DUELING && lane < N ? val[row * ldv + lane] : 0.f;
    const float mean = dqn_col_mean<DUELING>(slab, A, N, lane);
    const int best = c51_first_argmax<DUELING>(slab, A, N, lane, mean, v, z, q + row * ldq);
    if (greedy && lane == 0) greedy[row] = best;
  }
}

// ------------------------------------------------------------------- host
// the statistics launch of both distributional units: nb slots of {sum w loss,
// sum loss} into stats[2] = the sums / Bg
int launch_dqn_dist_stats(const double* partials, int nb, double Bg, float* stats, hipStream_t st) {
  hipLaunchKernelGGL(c51_stats_kernel, dim3(1), dim3(64), 0, st, partials, nb, Bg, stats);
  return check_launch("c51_stats_kernel");
}

// an upper bound of the row blocks of any device: one per quad of rows
int64_t c51_partials_bytes(int64_t B) {
  return B < 1 ? 0 : (B + kNW - 1) / kNW * 2 * (int64_t)sizeof(double);
}

// the checks both launchers share; 0 or SMI_E_ARG with the message set
static int c51_check_shape(const char* who, int A, int N, float v_min, float v_max) {
  char msg[160];
  const char* why = nullptr;
  if (N < 2 || N > kC51MaxAtoms) why = "atoms outside [2, 64]";
  else if (A < 1) why = "A < 1";
  else if ((int64_t)A * N > kC51LdsBytes / 4 / kNW) why = "A * atoms over 3072 (the LDS slabs of a workgroup)";
  else if (!(v_max > v_min)) why = "v_max <= v_min";
  if (!why) return SMI_OK;
  snprintf(msg, sizeof(msg), "%s: %s", who, why);
  return set_error(SMI_E_ARG, msg);
}

int launch_c51_td(const float* adv, int64_t lda, const float* adv_n, int64_t ldn,
                  const float* adv_t, int64_t ldt, const float* val, int64_t ldv,
                  const float* val_n, int64_t ldvn, const float* val_t, int64_t ldvt,
                  const float* actions, int64_t as, const float* rewards, int64_t rs,
                  const float* dones, int64_t ds, const float* w, int64_t B, int64_t B_global,
                  int64_t row0, int A, int N, float v_min, float v_max, float gamma, int dueling,
                  int double_q, float* dadv, int64_t ldd, float* dval, int64_t lddv, float* td_all,
                  float* m_out, int32_t* astar_out, double* partials, int64_t partials_bytes,
                  float* stats, hipStream_t st) {
  RC_CHECK(c51_check_shape("dqn_c51_td", A, N, v_min, v_max));
  const int64_t AN = (int64_t)A * N;
  if (lda < AN || ldt < AN || ldd < AN || (double_q && ldn < AN) ||
      (dueling && (ldv < N || ldvt < N || lddv < N || (double_q && ldvn < N))))
    return set_error(SMI_E_ARG, "dqn_c51_td: leading dims too small");
  const int64_t rpb = dqn_rows_per_block(B, dqn_cus());
  const int64_t nb = (B + rpb - 1) / rpb;
  if (rpb > INT32_MAX || partials_bytes < nb * 2 * (int64_t)sizeof(double))
    return set_error(SMI_E_ARG, "dqn_c51_td: partials workspace too small "
                                "(smi_dqn_c51_partials_bytes)");
  const int vec = dqn_aligned16(adv, lda) && dqn_aligned16(adv_t, ldt) &&
                  (!double_q || dqn_aligned16(adv_n, ldn));
  const C51TdArgs p{adv, lda, adv_n, ldn, adv_t, ldt, val, ldv, val_n, ldvn, val_t, ldvt,
                    actions, as, rewards, rs, dones, ds, w, B, A, N, v_min, v_max, gamma,
                    B_global, row0, (int)rpb, vec, dadv, ldd, dval, lddv, td_all, m_out,
                    astar_out, partials};
  const size_t lds = (size_t)kNW * round4((int)AN) * sizeof(float);
  const dim3 grid((unsigned)nb), wg(kWG);
  const char* what;
  if (dueling && double_q) {
    hipLaunchKernelGGL((c51_td_kernel<true, true>), grid, wg, lds, st, p);
    what = "c51_td_kernel<1,1>";
  } else if (dueling) {
    hipLaunchKernelGGL((c51_td_kernel<true, false>), grid, wg, lds, st, p);
    what = "c51_td_kernel<1,0>";
  } else if (double_q) {
    hipLaunchKernelGGL((c51_td_kernel<false, true>), grid, wg, lds, st, p);
    what = "c51_td_kernel<0,1>";
  } else {
    hipLaunchKernelGGL((c51_td_kernel<false, false>), grid, wg, lds, st, p);
    what = "c51_td_kernel<0,0>";
  }
  RC_CHECK(check_launch(what));
  RC_CHECK(launch_dqn_dist_stats(partials, (int)nb, (double)B_global, stats, st));
  return check_launch(what);                     // smi_last_launch names the TD form
}

int launch_c51_q(const float* adv, int64_t lda, const float* val, int64_t ldv, int64_t rows, int A,
                 int N, float v_min, float v_max, int dueling, float* q, int64_t ldq,
                 int32_t* greedy, hipStream_t st) {
  RC_CHECK(c51_check_shape("dqn_c51_q", A, N, v_min, v_max));
  const int64_t AN = (int64_t)A * N;
  if (lda < AN || ldq < A || (dueling && ldv < N))
    return set_error(SMI_E_ARG, "dqn_c51_q: leading dims too small");
  const int64_t cap = (int64_t)kDistBlocksPerCU * dqn_cus();
  int64_t g = (rows + kNW - 1) / kNW;
  g = g < 1 ? 1 : (g > cap ? cap : g);
  const int vec = dqn_aligned16(adv, lda);
  const size_t lds = (size_t)kNW * round4((int)AN) * sizeof(float);
  if (dueling) {
    hipLaunchKernelGGL((c51_q_kernel<true>), dim3((unsigned)g), dim3(kWG), lds, st, adv, lda, val,
                       ldv, rows, A, N, v_min, v_max, vec, q, ldq, greedy);
    return check_launch("c51_q_kernel<1>");
  }
  hipLaunchKernelGGL((c51_q_kernel<false>), dim3((unsigned)g), dim3(kWG), lds, st, adv, lda, val,
                     ldv, rows, A, N, v_min, v_max, vec, q, ldq, greedy);
  return check_launch("c51_q_kernel<0>");
}

}  // namespace smi
