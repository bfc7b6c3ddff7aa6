// dqn_iqn_kernels.hip — the implicit quantile head (IQN, Dabney et al. 2018b) of
// DQNLearner / QAgentBatch / FFQfunc: the network takes a sampled quantile
// fraction tau per sample row and the loss is the quantile pair loss of
// dqn_quant_kernels.hip with per-sample tau.  The reference has no
// distributional DQN; the specification below is this project's own.
//
//   iqn_taus          the fractions: a stateless counter-based draw
//   iqn_embed_fwd     Z = H1 (.) relu(bias + cos(pi i tau) W^T): an fp32-MFMA GEMM
//                     whose cosine operand is generated in registers
//   iqn_embed_dh1 / iqn_embed_dw / iqn_embed_dw_sum   its backward
//   iqn_td<DUELING, DOUBLE_Q, HUBER>   the TD step, smi_iqn_td_shard the same
//                     kernel on one rank's rows of a global batch
//   iqn_q<DUELING>    Q [rows][A] = the mean over K samples, the first arg-max
//
// Sample rows.  An observation b has N sample rows r = b N + n (n < N); the head
// outputs of a net are adv [B N][ld >= A] and val [B N] (dueling), so a row's
// head block is SAMPLE major: [N][A].  fp32 throughout, no contraction into
// fma except where fmaf is written.
//
// Fractions (iqn_taus).  Sample g = (row0 + row) N + n of stream `stream_id`
// at step *step: x = word 0 of Philox4x32-10(key = {seed lo, seed hi}, counter
// = {g lo, g hi, (uint32)*step, stream_id}); tau = ((x >> 9) + 0.5) 2^-23,
// exact in fp32 and strictly inside (0, 1).  (24 random bits, (k + 0.5) 2^-24,
// need 25 significand bits: the largest one rounds to 1.0f.)  *step is read on
// the device, so a replayed graph draws new fractions; a shard passes its row0
// and draws the whole batch's fractions of its rows.
//
// Cosine.  c_i(tau) = cos(pi i tau), i < n_cos <= 64, is cospif(s) of
//   s = fmaf((float)i, tau, -2 rint(0.5 ((float)i tau)))
// For a tau on the 2^-23 grid s is exact (a multiple of 2^-23 in [-1, 1]); for
// any tau it is the correctly rounded i tau - 2 m.  cospif is the device
// library's (its own reduction is exact, its polynomial within a few ulp), so
// the error of c_i does not grow with i.  Chosen over the hardware cosine
// (v_cos_f32 on i tau / 2 revolutions: its absolute error is not documented
// to fp32 precision and the product i tau / 2 rounds before the reduction:
// 4e-6 revolutions at i = 63) and over a Chebyshev recurrence from cos(pi tau)
// (its error grows like i^2 ulp, 1e-4 at i = 63 near tau = 0 and 1).  The
// kernels are bound by their stores and loads, not by the
// cosine; that is reasoning from the code, the alternatives were not timed.
//
// Embedding forward.  M = B N rows, d columns, K = n_cos (a multiple of 4):
//   phi[r][j] = relu(bias[j] + sum_i c_i(tau_r) W[j][i])    the sum is the MFMA's
//               k-ordered chain starting from bias[j], i ascending
//   Z[r][j]   = H1[r / N][j] * phi[r][j];  phi is stored only when asked for
// relu is torch's (a NaN stays).  Work split: the product is computed
// TRANSPOSED, D^T = W C^T (v_mfma_f32_16x16x4_f32: A = W[j][i], B = C[r][i]),
// so a lane leaves the MFMA with FOUR CONSECUTIVE COLUMNS of one row and the
// epilogue is one 16-byte load of H1 and one 16-byte store of Z (and phi) per
// lane: a wave writes 16 rows x 64 columns with four stores per lane.  A
// workgroup stages its chunk of up to 128 columns of W (<= 34 KiB, leading
// dimension n_cos + 4) in LDS once and its four waves walk 16-row tiles
// (persistent grid sized from the CU count); a lane computes the 16 cosines of
// its (row, i) slots once per tile and reuses them for every column of the
// chunk; the cosine matrix exists in registers only.  16-byte accesses are
// one decision per launch and operand (Z, phi, H1: base 16-byte aligned and
// leading dimension a multiple of 4), dwords otherwise and for the last d % 4
// columns.
//
// Embedding backward.
//   dH1[b][j] = H1[b][j] > 0 ? sum_n dZ[b N + n][j] * phi[b N + n][j] : 0
//               n ascending from +0; one thread per (b, j)
//   dpre[r][j] = phi[r][j] > 0 ? dZ[r][j] * H1[r / N][j] : 0
//   dW[j][i]  = sum_r dpre[r][j] c_i(tau_r),  db[j] = dW[j][0]   (c_0 = 1: the
//               same sum, term by term)
// dW is an MFMA GEMM over the rows (A = dpre, B = the regenerated cosines): the
// rows are cut into ns = min(64, ceil(M / 256)) contiguous ranges, a workgroup
// owns (64 columns, one range), wave w the cosines 16 w .. 16 w + 15, and adds
// its range 4 rows per MFMA, rows ascending.  ns == 1 writes dW / db; otherwise
// every partial goes to the caller's scratch [ns][d][n_cos] and a second launch
// adds them s ascending: no atomics, the same bits on every run, dW / db are
// WRITTEN.  A caller may pass dZ already masked by Z > 0 (the layer above
// masks by its input Z = H1 phi): every result above is unchanged, since
// Z > 0 exactly where H1 > 0 and phi > 0.
//
// TD step (iqn_td).  One wave per row b, four rows per workgroup, one lane per
// online sample; N online samples, N' samples of the selecting and target nets
// (both in [1, 64], A max(N, N') <= 4096).  Per row:
//   dueling   mean_n = (adv[n][0] + ... + adv[n][A-1]) / A   left to right
//             theta[n][a] = (adv[n][a] - mean_n) + val[n];   otherwise theta = adv
//   Q[a]    = (xor butterfly (32, ..., 1) over lanes of theta[lane][a], 0 for
//             lane >= the net's samples) / samples
//   a*      = first maximum of Q(s') (scan with >): online net at s' on its own
//             N' samples with DOUBLE_Q, the target net otherwise
//   T_j     = r + gamma * ((1 - d) * theta_target(s')[j][a*])        j < N'
//   u_ij    = T_j - theta(s)[i][a_taken],  tau_i = tau[b N + i]
//   S_i, G_i  qr_pairs (dqn_rows.hpp; the pair terms, the Huber / pinball
//             branches and the 8-run fp32 / fp64 sums of dqn_quant_kernels.hip)
//             over the N' targets
//   loss    = (butterfly over S_i, 0 for i >= N) / N';  td[b] = loss
//   g_i     = (w * (-(G_i / N'))) / B
//   dadv[b N + i][a'] = g_i ([a' == a_taken] - 1/A), dval[b N + i] = g_i (dueling)
//   dadv[b N + i][a_taken] = g_i, 0 elsewhere (otherwise); every entry written
//   stats   = { mean(w loss), mean(loss) } through launch_dqn_dist_stats
// NaN / inf and the shard form: dqn_quant_kernels.hip's rules, unchanged.
// A wave stages one net's [samples][A] block in its own LDS region
// (dqn_copy_slab<64>: 16-byte loads when every block read is contiguous, ld ==
// A, and 16-byte aligned, dwords when contiguous, a strided dword copy
// otherwise: one decision per launch), reuses the region for the three nets
// and at the end for g_i, so that dadv is written with consecutive lanes on
// consecutive addresses.
#include <math.h>
#include <stdio.h>
#include "smi_device.hpp"
#include "smi_internal.hpp"
#include "dqn_rows.hpp"
#include "philox.hpp"

namespace smi {

constexpr int kIqnMaxN = 64;                     // one lane per sample
constexpr int kIqnMaxSlab = 4096;                // A max(N, N'): 4 wave regions of 16 KiB
constexpr int kIqnMaxCos = 64;
constexpr int kIqnChunk = 128;                   // columns of W a forward workgroup stages
constexpr int kIqnDwCols = 64;                   // columns of a weight-gradient workgroup
constexpr int kIqnDwRows = 256;                  // rows per range of the weight gradient, at least
constexpr int kIqnDwMaxSplit = 64;

// ------------------------------------------------------------------ fractions
// (iqn_philox: philox.hpp, shared with noisy_kernels.hip)
__global__ void __launch_bounds__(kWG)
iqn_taus_kernel(uint64_t seed, const int32_t* __restrict__ step, uint32_t stream_id, int64_t row0,
                int64_t count, int N, float* __restrict__ tau) {
  const uint32_t s = (uint32_t)step[0];
  for (int64_t e = (int64_t)blockIdx.x * kWG + threadIdx.x; e < count;
       e += (int64_t)gridDim.x * kWG) {
    const uint64_t g = (uint64_t)(row0 * N + e);
    const uint32_t x = iqn_philox((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)g,
                                  (uint32_t)(g >> 32), s, stream_id);
    tau[e] = ((float)(x >> 9) + 0.5f) * 0x1p-23f;
  }
}

// --------------------------------------------------------------------- cosine
__device__ __forceinline__ float iqn_cos(int i, float tau) {
#pragma clang fp contract(off)
  const float fi = (float)i;
  const float m = rintf(0.5f * (fi * tau));
  return cospif(fmaf(fi, tau, -2.f * m));
}

// ---------------------------------------------------------- embedding forward
struct IqnFwdArgs {
  const float* tau; const float* H1; int64_t ldh;
  int64_t M; int N;
  const float* W; const float* bias; int K, d;
  float* Z; int64_t ldz; float* phi; int64_t ldp;
  int vz, vp, vh;
};

__global__ void __launch_bounds__(kWG) iqn_embed_fwd_kernel(IqnFwdArgs p) {
  extern __shared__ float4 iqn_lds[];
  float* Ws = reinterpret_cast<float*>(iqn_lds);
  const int K = p.K, ldw = K + 4, K4 = K >> 2;
  const int c0 = blockIdx.y * kIqnChunk;
  const int nc = p.d - c0 < kIqnChunk ? p.d - c0 : kIqnChunk;        // columns of this chunk
  const int ncr = (nc + 15) & ~15;                                  // staged, zero past nc
  float* bs = Ws + kIqnChunk * ldw;
  for (int e = threadIdx.x; e < ncr * K; e += kWG) {
    const int c = e / K, k = e - c * K;
    Ws[c * ldw + k] = c < nc ? p.W[(int64_t)(c0 + c) * K + k] : 0.f;
  }
  for (int c = threadIdx.x; c < ncr; c += kWG) bs[c] = c < nc ? p.bias[c0 + c] : 0.f;
  __syncthreads();
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t tiles = (p.M + 15) >> 4;
  for (int64_t t = (int64_t)blockIdx.x * kNW + wave; t < tiles; t += (int64_t)gridDim.x * kNW) {
    const int64_t row = t * 16 + li;
    const bool rv = row < p.M;
    const float tr = rv ? p.tau[row] : 0.5f;
    float c[kIqnMaxCos / 4];
#pragma unroll
    for (int u = 0; u < kIqnMaxCos / 4; ++u) c[u] = u < K4 ? iqn_cos(4 * u + lk, tr) : 0.f;
    const float* hrow = p.H1 + (rv ? row / p.N : 0) * p.ldh + c0;
    for (int cg = 0; cg < nc; cg += 64) {
      const int nq = (nc - cg + 15) >> 4 < 4 ? (nc - cg + 15) >> 4 : 4;  // 16-column tiles here
      f32x4 acc[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float* b4 = bs + (q < nq ? cg + q * 16 + lk * 4 : 0);
        acc[q] = f32x4{b4[0], b4[1], b4[2], b4[3]};
      }
#pragma unroll
      for (int u = 0; u < kIqnMaxCos / 4; ++u) {
        if (u < K4) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (q < nq) acc[q] = mfma4(Ws[(cg + q * 16 + li) * ldw + 4 * u + lk], c[u], acc[q]);
          }
        }
      }
      if (rv) {                                  // no lane leaves the loop: MFMAs follow
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int col = cg + q * 16 + lk * 4;                      // in the chunk
          if (q >= nq || col >= nc) continue;
          float ph[4], h[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) ph[i] = act_f<ACT_RELU>(acc[q][i]);
          const bool full = col + 4 <= nc;
          if (full && p.vh) {
            const float4 v = *reinterpret_cast<const float4*>(hrow + col);
            h[0] = v.x; h[1] = v.y; h[2] = v.z; h[3] = v.w;
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) h[i] = col + i < nc ? hrow[col + i] : 0.f;
          }
          float* zr = p.Z + row * p.ldz + c0 + col;
          if (full && p.vz) {
            *reinterpret_cast<float4*>(zr) = make_float4(h[0] * ph[0], h[1] * ph[1], h[2] * ph[2],
                                                         h[3] * ph[3]);
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (col + i < nc) zr[i] = h[i] * ph[i];
          }
          if (p.phi) {
            float* pr = p.phi + row * p.ldp + c0 + col;
            if (full && p.vp) {
              *reinterpret_cast<float4*>(pr) = make_float4(ph[0], ph[1], ph[2], ph[3]);
            } else {
#pragma unroll
              for (int i = 0; i < 4; ++i)
                if (col + i < nc) pr[i] = ph[i];
            }
          }
        }
      }
    }
  }
}

// --------------------------------------------------------- embedding backward
struct IqnBwdArgs {
  const float* dZ; int64_t ldz; const float* tau; const float* H1; int64_t ldh;
  const float* phi; int64_t ldp; int64_t B; int N; int64_t M; int K, d;
  float* dW; float* db; float* dH1; int64_t lddh;
  float* part; int ns; int64_t rps;              // ranges and rows per range (a multiple of 4)
};

__global__ void __launch_bounds__(kWG) iqn_embed_dh1_kernel(IqnBwdArgs p) {
#pragma clang fp contract(off)
  const int64_t total = p.B * p.d;
  for (int64_t e = (int64_t)blockIdx.x * kWG + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * kWG) {
    const int64_t b = e / p.d;
    const int j = (int)(e - b * p.d);
    const float* dz = p.dZ + b * p.N * p.ldz + j;
    const float* ph = p.phi + b * p.N * p.ldp + j;
    float s = 0.f;
    for (int n = 0; n < p.N; ++n) s = s + dz[n * p.ldz] * ph[n * p.ldp];
    p.dH1[b * p.lddh + j] = p.H1[b * p.ldh + j] > 0.f ? s : 0.f;
  }
}

// grid (column blocks of 64, ns); wave w: the cosines 16 w .. 16 w + 15
__global__ void __launch_bounds__(kWG) iqn_embed_dw_kernel(IqnBwdArgs p) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (wave * 16 >= p.K) return;                  // no barrier below
  const int j0 = blockIdx.x * kIqnDwCols, ic = wave * 16 + li;
  const int64_t ra = (int64_t)blockIdx.y * p.rps;
  const int64_t rb = ra + p.rps < p.M ? ra + p.rps : p.M;
  f32x4 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int64_t r0 = ra; r0 < rb; r0 += 4) {
    const int64_t r = r0 + lk;
    const bool rv = r < rb;
    const float cs = rv && ic < p.K ? iqn_cos(ic, p.tau[r]) : 0.f;
    const int64_t b = rv ? r / p.N : 0;
    float a[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = j0 + q * 16 + li;
      float v = 0.f;
      if (rv && j < p.d) {
        const float ph = p.phi[r * p.ldp + j];
        v = ph > 0.f ? p.dZ[r * p.ldz + j] * p.H1[b * p.ldh + j] : 0.f;
      }
      a[q] = v;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = mfma4(a[q], cs, acc[q]);
  }
  if (ic >= p.K) return;
  float* dw = p.ns > 1 ? p.part + (int64_t)blockIdx.y * p.d * p.K : p.dW;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = j0 + q * 16 + lk * 4 + i;
      if (j >= p.d) continue;
      dw[(int64_t)j * p.K + ic] = acc[q][i];
      if (p.ns == 1 && ic == 0) p.db[j] = acc[q][i];
    }
  }
}

__global__ void __launch_bounds__(kWG) iqn_embed_dw_sum_kernel(IqnBwdArgs p) {
#pragma clang fp contract(off)
  const int64_t total = (int64_t)p.d * p.K;
  for (int64_t e = (int64_t)blockIdx.x * kWG + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * kWG) {
    float s = p.part[e];
    for (int k = 1; k < p.ns; ++k) s = s + p.part[k * total + e];
    p.dW[e] = s;
    if (e % p.K == 0) p.db[e / p.K] = s;
  }
}

// -------------------------------------------------------------------- TD step
struct IqnTdArgs {
  const float* adv; int64_t lda;
  const float* adv_n; int64_t ldn;
  const float* adv_t; int64_t ldt;
  const float *val, *val_n, *val_t;
  const float* tau;
  const float* act; int64_t as;
  const float* rew; int64_t rs;
  const float* done; int64_t ds;
  const float* w;
  int64_t B; int A, N, Nt; float kappa, gamma;
  int64_t Bg, row0;
  int rpb;                 // rows per workgroup, a multiple of kNW
  int mode;                // staging: 2 16-byte loads, 1 contiguous dwords, 0 strided dwords
  float* dadv; int64_t ldd;
  float* dval;
  float* td; float* t_out; int32_t* astar; double* partials;
};

// one net's [n][A] block of a row into the wave's region
__device__ __forceinline__ void iqn_stage(const float* __restrict__ src, int64_t ld, int n, int A,
                                          int mode, float* __restrict__ slab, int lane) {
  if (mode) {
    dqn_copy_slab<64>(src, n * A, mode == 2, slab, lane);
    return;
  }
  for (int e = lane; e < n * A; e += 64) {
    const int s = e / A;
    slab[e] = src[s * ld + (e - s * A)];
  }
}

// the dueling mean of sample `lane` over the actions, left to right
template <bool DUELING>
__device__ __forceinline__ float iqn_row_mean(const float* __restrict__ slab, int A, int n, int lane) {
#pragma clang fp contract(off)
  if (!DUELING || lane >= n) return 0.f;
  const float* x = slab + lane * A;
  float s = x[0];
  for (int a = 1; a < A; ++a) s = s + x[a];
  return s / (float)A;
}

template <bool DUELING>
__device__ __forceinline__ float iqn_theta(const float* __restrict__ slab, int A, int s, int a,
                                           float mean, float v) {
#pragma clang fp contract(off)
  const float x = slab[s * A + a];
  return DUELING ? (x - mean) + v : x;
}

// first index of the maximum of Q[a] = mean over the n staged samples
template <bool DUELING>
__device__ __forceinline__ int iqn_argmax(const float* __restrict__ slab, int A, int n, int lane,
                                          float mean, float v, float* __restrict__ q_out) {
#pragma clang fp contract(off)
  const float fn = (float)n;
  int best = 0;
  float qb = 0.f;
  for (int a = 0; a < A; ++a) {
    const float th = lane < n ? 0.f + iqn_theta<DUELING>(slab, A, lane, a, mean, v) : 0.f;
    const float q = wave_sum(th) / fn;
    if (q_out && lane == 0) q_out[a] = q;
    if (a == 0) qb = q;
    else if (q > qb) { qb = q; best = a; }
  }
  return best;
}

template <bool DUELING, bool DOUBLE_Q, bool HUBER>
__global__ void __launch_bounds__(kWG) iqn_td_kernel(IqnTdArgs p) {
#pragma clang fp contract(off)
  extern __shared__ float4 iqn_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int A = p.A, N = p.N, Nt = p.Nt;
  const int region = round4(A * (N > Nt ? N : Nt));
  float* slab = reinterpret_cast<float*>(iqn_lds) + wave * region;
  const bool on = lane < N, ont = lane < Nt;
  for (int64_t i = (int64_t)blockIdx.x * kWG + threadIdx.x; i < p.Bg - p.B;
       i += (int64_t)gridDim.x * kWG)
    p.td[i < p.row0 ? i : i + p.B] = 0.f;        // the other ranks' entries of td_all
  const int64_t r0 = (int64_t)blockIdx.x * p.rpb;
  double sl = 0.0, st = 0.0;                     // thread 0: this block's sums, rows ascending
  for (int it = 0; it < p.rpb / kNW; ++it) {
    const int64_t row = r0 + (int64_t)it * kNW + wave;
    double rl = 0.0, rt = 0.0;
    if (row < p.B) {
      int astar = 0;
      if (DOUBLE_Q) {
        dqn_wave_sync();                         // the previous row's reads are done
        iqn_stage(p.adv_n + row * Nt * p.ldn, p.ldn, Nt, A, p.mode, slab, lane);
        dqn_wave_sync();
        const float vn = DUELING && ont ? p.val_n[row * Nt + lane] : 0.f;
        const float mn = iqn_row_mean<DUELING>(slab, A, Nt, lane);
        astar = iqn_argmax<DUELING>(slab, A, Nt, lane, mn, vn, nullptr);
      }
      dqn_wave_sync();
      iqn_stage(p.adv_t + row * Nt * p.ldt, p.ldt, Nt, A, p.mode, slab, lane);
      dqn_wave_sync();
      const float vt = DUELING && ont ? p.val_t[row * Nt + lane] : 0.f;
      const float mt = iqn_row_mean<DUELING>(slab, A, Nt, lane);
      if (!DOUBLE_Q) astar = iqn_argmax<DUELING>(slab, A, Nt, lane, mt, vt, nullptr);
      const float r = p.rew[row * p.rs], d = p.done[row * p.ds];
      const float tt = ont ? iqn_theta<DUELING>(slab, A, lane, astar, mt, vt) : 0.f;
      const float T = r + p.gamma * ((1.f - d) * tt);
      dqn_wave_sync();
      iqn_stage(p.adv + row * N * p.lda, p.lda, N, A, p.mode, slab, lane);
      dqn_wave_sync();
      const float v = DUELING && on ? p.val[row * N + lane] : 0.f;
      const float mean = iqn_row_mean<DUELING>(slab, A, N, lane);
      const int ai = dqn_action_index(p.act[row * p.as], A);
      const float th = on ? iqn_theta<DUELING>(slab, A, lane, ai, mean, v) : 0.f;
      const float tau = on ? p.tau[row * N + lane] : 0.5f;
      const QrSums s = qr_pairs<HUBER>(th, tau, p.kappa, Nt, [&](int j) { return dqn_lane(T, j); });
      const float loss = wave_sum(on ? s.S : 0.f) / (float)Nt;
      const float wi = p.w ? p.w[row] : 1.f;
      const float g = (wi * (-(s.G / (float)Nt))) / (float)p.Bg;
      // g_i through the region, so that dadv leaves with consecutive lanes on
      // consecutive addresses
      dqn_wave_sync();
      if (on) slab[lane] = g;
      dqn_wave_sync();
      const float invA = 1.f / (float)A;
      float* da = p.dadv + row * N * p.ldd;
      for (int e = lane; e < N * A; e += 64) {
        const int i = e / A, a = e - i * A;
        const float gi = slab[i];
        const float ea = a == ai ? 1.f : 0.f;
        da[i * p.ldd + a] = DUELING ? gi * (ea - invA) : (a == ai ? gi : 0.f);
      }
      if (DUELING && on) p.dval[row * N + lane] = g;
      if (ont && p.t_out) p.t_out[row * Nt + lane] = T;
      if (lane == 0) {
        p.td[p.row0 + row] = loss;
        if (p.astar) p.astar[row] = astar;
      }
      rl = (double)(wi * loss);
      rt = (double)loss;
    }
    // the waves' {w loss, loss} meet in the first 16 bytes of their regions
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
        const double* s =
            reinterpret_cast<const double*>(reinterpret_cast<float*>(iqn_lds) + w * region);
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

template <bool DUELING>
__global__ void __launch_bounds__(kWG)
iqn_q_kernel(const float* __restrict__ adv, int64_t lda, const float* __restrict__ val,
             int64_t rows, int A, int K, int mode, float* __restrict__ q, int64_t ldq,
             int32_t* __restrict__ greedy) {
  extern __shared__ float4 iqn_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* slab = reinterpret_cast<float*>(iqn_lds) + wave * round4(A * K);
  for (int64_t row = (int64_t)blockIdx.x * kNW + wave; row < rows;
       row += (int64_t)gridDim.x * kNW) {
    dqn_wave_sync();
    iqn_stage(adv + row * K * lda, lda, K, A, mode, slab, lane);
    dqn_wave_sync();
    const float v = DUELING && lane < K ? val[row * K + lane] : 0.f;
    const float mean = iqn_row_mean<DUELING>(slab, A, K, lane);
    const int best = iqn_argmax<DUELING>(slab, A, K, lane, mean, v, q + row * ldq);
    if (greedy && lane == 0) greedy[row] = best;
  }
}

// ------------------------------------------------------------------- host
int64_t iqn_partials_bytes(int64_t B) { return B < 1 ? 0 : B * 2 * (int64_t)sizeof(double); }

static int iqn_dw_split(int64_t M) {
  const int64_t ns = (M + kIqnDwRows - 1) / kIqnDwRows;
  return (int)(ns < 1 ? 1 : (ns > kIqnDwMaxSplit ? kIqnDwMaxSplit : ns));
}

int64_t iqn_embed_scratch_bytes(int64_t B, int N, int n_cos, int d) {
  if (B < 1 || N < 1 || n_cos < 1 || d < 1) return 0;
  const int ns = iqn_dw_split(B * N);
  return ns > 1 ? (int64_t)ns * d * n_cos * (int64_t)sizeof(float) : 0;
}

static int iqn_check(const char* who, int A, int N, int Nt) {
  char msg[160];
  const char* why = nullptr;
  if (N < 1 || N > kIqnMaxN || Nt < 1 || Nt > kIqnMaxN) why = "samples outside [1, 64]";
  else if (A < 1) why = "A < 1";
  else if ((int64_t)A * (N > Nt ? N : Nt) > kIqnMaxSlab)
    why = "A * samples over 4096 (the LDS regions of a workgroup)";
  if (!why) return SMI_OK;
  snprintf(msg, sizeof(msg), "%s: %s", who, why);
  return set_error(SMI_E_ARG, msg);
}

static int iqn_check_embed(const char* who, int64_t B, int N, int n_cos, int d) {
  char msg[160];
  const char* why = nullptr;
  if (B < 1) why = "B < 1";
  else if (N < 1 || N > kIqnMaxN) why = "samples outside [1, 64]";
  else if (n_cos < 4 || n_cos > kIqnMaxCos || (n_cos & 3)) why = "n_cos not a multiple of 4 in [4, 64]";
  else if (d < 1) why = "d < 1";
  else if (B * N > (int64_t)INT32_MAX * 16) why = "B * N over the launch grid";
  if (!why) return SMI_OK;
  snprintf(msg, sizeof(msg), "%s: %s", who, why);
  return set_error(SMI_E_ARG, msg);
}

// the staging form of a launch: every block read is [n][A] at its leading dimension
static int iqn_stage_mode(const float* const* slabs, const int64_t* lds, const int* ns, int count,
                          int A) {
  int mode = 2;
  for (int i = 0; i < count; ++i) {
    if (!slabs[i]) continue;
    if (lds[i] != A) return 0;
    if ((reinterpret_cast<uintptr_t>(slabs[i]) & 15) || ((ns[i] * A) & 3)) mode = 1;
  }
  return mode;
}

int launch_iqn_taus(uint64_t seed, const int32_t* step, int stream_id, int64_t row0, int64_t rows,
                    int N, float* tau, hipStream_t st) {
  if (rows < 1 || N < 1 || N > kIqnMaxN || row0 < 0 || stream_id < 0)
    return set_error(SMI_E_ARG, "iqn_taus: rows < 1, samples outside [1, 64], row0 < 0 or stream_id < 0");
  const int64_t count = rows * N;
  int64_t g = (count + kWG - 1) / kWG;
  g = g > 4096 ? 4096 : g;
  hipLaunchKernelGGL(iqn_taus_kernel, dim3((unsigned)g), dim3(kWG), 0, st, seed, step,
                     (uint32_t)stream_id, row0, count, N, tau);
  return check_launch("iqn_taus_kernel");
}

int launch_iqn_embed_fwd(const float* tau, const float* H1, int64_t ldh, int64_t B, int N,
                         const float* W, const float* bias, int n_cos, int d, float* Z,
                         int64_t ldz, float* phi, int64_t ldp, hipStream_t st) {
  RC_CHECK(iqn_check_embed("iqn_embed_forward", B, N, n_cos, d));
  if (ldh < d || ldz < d || (phi && ldp < d))
    return set_error(SMI_E_ARG, "iqn_embed_forward: leading dims too small");
  const int64_t M = B * N;
  const IqnFwdArgs p{tau, H1, ldh, M, N, W, bias, n_cos, d, Z, ldz, phi, ldp,
                     dqn_aligned16(Z, ldz), phi && dqn_aligned16(phi, ldp), dqn_aligned16(H1, ldh)};
  const int chunks = (d + kIqnChunk - 1) / kIqnChunk;
  const int64_t groups = ((M + 15) / 16 + kNW - 1) / kNW;          // of four row tiles
  int64_t cap = (int64_t)kDistBlocksPerCU * dqn_cus() / chunks;
  cap = cap < 1 ? 1 : cap;
  if (chunks > 65535) return set_error(SMI_E_ARG, "iqn_embed_forward: d over the launch grid");
  const dim3 grid((unsigned)(groups < cap ? groups : cap), (unsigned)chunks);
  const size_t lds = (size_t)(kIqnChunk * (n_cos + 4) + kIqnChunk) * sizeof(float);
  hipLaunchKernelGGL(iqn_embed_fwd_kernel, grid, dim3(kWG), lds, st, p);
  return check_launch("iqn_embed_fwd_kernel");
}

int launch_iqn_embed_bwd(const float* dZ, int64_t ldz, const float* tau, const float* H1,
                         int64_t ldh, const float* phi, int64_t ldp, int64_t B, int N, float* dW,
                         float* db, int n_cos, int d, float* dH1, int64_t lddh, float* scratch,
                         int64_t scratch_bytes, hipStream_t st) {
  RC_CHECK(iqn_check_embed("iqn_embed_backward", B, N, n_cos, d));
  if (ldh < d || ldz < d || ldp < d || lddh < d)
    return set_error(SMI_E_ARG, "iqn_embed_backward: leading dims too small");
  const int64_t M = B * N;
  const int ns = iqn_dw_split(M);
  if (ns > 1 && (!scratch || scratch_bytes < iqn_embed_scratch_bytes(B, N, n_cos, d)))
    return set_error(SMI_E_ARG, "iqn_embed_backward: scratch too small (smi_iqn_embed_scratch_bytes)");
  const int cblocks = (d + kIqnDwCols - 1) / kIqnDwCols;
  if (cblocks > INT32_MAX / 2) return set_error(SMI_E_ARG, "iqn_embed_backward: d over the launch grid");
  const int64_t rps = ((M + ns - 1) / ns + 3) / 4 * 4;
  const IqnBwdArgs p{dZ, ldz, tau, H1, ldh, phi, ldp, B, N, M, n_cos, d, dW, db, dH1, lddh,
                     scratch, ns, rps};
  const int64_t cap = (int64_t)kDistBlocksPerCU * dqn_cus();
  int64_t g = (B * d + kWG - 1) / kWG;
  hipLaunchKernelGGL(iqn_embed_dh1_kernel, dim3((unsigned)(g < cap ? g : cap)), dim3(kWG), 0, st, p);
  RC_CHECK(check_launch("iqn_embed_dh1_kernel"));
  hipLaunchKernelGGL(iqn_embed_dw_kernel, dim3((unsigned)cblocks, (unsigned)ns), dim3(kWG), 0, st, p);
  RC_CHECK(check_launch("iqn_embed_dw_kernel"));
  if (ns > 1) {
    g = ((int64_t)d * n_cos + kWG - 1) / kWG;
    hipLaunchKernelGGL(iqn_embed_dw_sum_kernel, dim3((unsigned)(g < cap ? g : cap)), dim3(kWG), 0,
                       st, p);
    RC_CHECK(check_launch("iqn_embed_dw_sum_kernel"));
  }
  return SMI_OK;
}

template <bool HUBER>
static const char* iqn_td_launch(const IqnTdArgs& p, int dueling, int double_q, dim3 grid,
                                 size_t lds, hipStream_t st) {
#define IQN_TD_FORM(D, Q)                                                                   \
  do {                                                                                      \
    hipLaunchKernelGGL((iqn_td_kernel<D, Q, HUBER>), grid, dim3(kWG), lds, st, p);          \
    return HUBER ? "iqn_td_kernel<" #D "," #Q ",1>" : "iqn_td_kernel<" #D "," #Q ",0>";     \
  } while (0)
  if (dueling && double_q) IQN_TD_FORM(1, 1);
  if (dueling) IQN_TD_FORM(1, 0);
  if (double_q) IQN_TD_FORM(0, 1);
  IQN_TD_FORM(0, 0);
#undef IQN_TD_FORM
}

int launch_iqn_td(const float* adv, int64_t lda, const float* adv_n, int64_t ldn,
                  const float* adv_t, int64_t ldt, const float* val, const float* val_n,
                  const float* val_t, const float* tau, const float* actions, int64_t as,
                  const float* rewards, int64_t rs, const float* dones, int64_t ds, const float* w,
                  int64_t B, int64_t B_global, int64_t row0, int A, int N, int Nt, float kappa,
                  float gamma, int dueling, int double_q, float* dadv, int64_t ldd, float* dval,
                  float* td_all, float* t_out, int32_t* astar_out, double* partials,
                  int64_t partials_bytes, float* stats, hipStream_t st) {
  RC_CHECK(iqn_check("iqn_td", A, N, Nt));
  if (!(kappa >= 0.f)) return set_error(SMI_E_ARG, "iqn_td: kappa < 0 or NaN");
  if (lda < A || ldt < A || ldd < A || (double_q && ldn < A))
    return set_error(SMI_E_ARG, "iqn_td: leading dims too small");
  const int64_t rpb = dqn_rows_per_block(B, dqn_cus());
  const int64_t nb = (B + rpb - 1) / rpb;
  if (rpb > INT32_MAX || nb > INT32_MAX) return set_error(SMI_E_ARG, "iqn_td: B over the launch grid");
  if (partials_bytes < nb * 2 * (int64_t)sizeof(double))
    return set_error(SMI_E_ARG, "iqn_td: partials workspace too small (smi_iqn_partials_bytes)");
  const float* slabs[3] = {adv, adv_t, double_q ? adv_n : nullptr};
  const int64_t lds3[3] = {lda, ldt, ldn};
  const int ns3[3] = {N, Nt, Nt};
  const IqnTdArgs p{adv, lda, adv_n, ldn, adv_t, ldt, val, val_n, val_t, tau, actions, as,
                    rewards, rs, dones, ds, w, B, A, N, Nt, kappa, gamma, B_global, row0,
                    (int)rpb, iqn_stage_mode(slabs, lds3, ns3, 3, A), dadv, ldd, dval, td_all,
                    t_out, astar_out, partials};
  const size_t lds = (size_t)kNW * round4(A * (N > Nt ? N : Nt)) * sizeof(float);
  const dim3 grid((unsigned)nb);
  const char* what = kappa > 0.f ? iqn_td_launch<true>(p, dueling, double_q, grid, lds, st)
                                 : iqn_td_launch<false>(p, dueling, double_q, grid, lds, st);
  RC_CHECK(check_launch(what));
  RC_CHECK(launch_dqn_dist_stats(partials, (int)nb, (double)B_global, stats, st));
  return check_launch(what);                     // smi_last_launch names the TD form
}

int launch_iqn_q(const float* adv, int64_t lda, const float* val, int64_t rows, int A, int K,
                 int dueling, float* q, int64_t ldq, int32_t* greedy, hipStream_t st) {
  RC_CHECK(iqn_check("iqn_q", A, K, K));
  if (lda < A || ldq < A) return set_error(SMI_E_ARG, "iqn_q: leading dims too small");
  const int64_t cap = (int64_t)kDistBlocksPerCU * dqn_cus();
  int64_t g = (rows + kNW - 1) / kNW;
  g = g < 1 ? 1 : (g > cap ? cap : g);
  const int mode = iqn_stage_mode(&adv, &lda, &K, 1, A);
  const size_t lds = (size_t)kNW * round4(A * K) * sizeof(float);
  if (dueling)
    hipLaunchKernelGGL(iqn_q_kernel<true>, dim3((unsigned)g), dim3(kWG), lds, st, adv, lda, val,
                       rows, A, K, mode, q, ldq, greedy);
  else
    hipLaunchKernelGGL(iqn_q_kernel<false>, dim3((unsigned)g), dim3(kWG), lds, st, adv, lda, val,
                       rows, A, K, mode, q, ldq, greedy);
  return check_launch(dueling ? "iqn_q_kernel<1>" : "iqn_q_kernel<0>");
}

}  // namespace smi
