// noisy_kernels.hip — noisy linear layers (NoisyNet, Fortunato et al. 2018,
// factorised Gaussian noise) of DQNLearner / QAgentBatch / FFQfunc.  The
// reference has no noisy layers; the specification below is this project's own.
//
//   noisy_draw        the noise vectors of up to 8 layers: a stateless
//                     counter-based draw (Philox4x32-10 + Box-Muller)
//   noisy_gemm<DX>    forward (DX = false) and input gradient (DX = true): ONE
//                     fp32-MFMA GEMM with TWO accumulator chains over one staged
//                     activation tile; the noisy weight W_mu + W_sig (.) (f_out
//                     f_in^T) never exists in memory
//   noisy_sigma_grad  the sigma gradients of every layer of a net from the mu
//                     gradients, one launch
//
// A layer (in -> out) has W_mu, W_sig [out][ldw >= in], b_mu, b_sig [out] and the
// noise vectors f_in [in], f_out [out]:
//   y[m][n]  = act((x W_mu^T + b_mu)[m][n] + f_out[n] * (((x (.) f_in) W_sig^T)[m][n] + b_sig[n]))
//   dx[m][k] = [mask[m][k] > 0] * ((dy W_mu)[m][k] + f_in[k] * (((dy (.) f_out) W_sig)[m][k]))
//   g_sigW[n][k] = g_muW[n][k] * (f_out[n] * f_in[k]),  g_sigb[n] = g_mub[n] * f_out[n]
// fp32 throughout (v_mfma_f32_16x16x4_f32), no contraction into fma beyond what
// is written (#pragma clang fp contract(off) over every function below).
//
// Draw (noisy_draw).  The image of a net is the layers' [f_in (in) | f_out
// (out)] concatenated.  Element e < in + out of layer l at step *step of stream
// `stream_id`: (x0, x1) = words 0 and 1 of Philox4x32-10(key = {seed lo, seed
// hi}, counter = {e, l, (uint32)*step, stream_id});
//   u1 = ((x0 >> 9) + 0.5) 2^-23,  u2 = ((x1 >> 9) + 0.5) 2^-23   (IQN's rule:
//        exact in fp32, strictly inside (0, 1), so logf(u1) is finite)
//   eps = sqrtf(-2 logf(u1)) * cospif(2 u2)      (2 u2 is exact)
//   f   = copysignf(sqrtf(fabsf(eps)), eps)
// f goes to f_image, eps to eps_image when it is given.  *step is read on the
// device (a replayed graph draws new noise); the counter holds the layer and
// the element within the layer only, so a layer's slice depends neither on the
// other layers' widths nor on a data-parallel shard's row offset.
//
// GEMM (noisy_gemm).  C [M][N] from A [M][K] (k contiguous) and the B pair:
//   forward   A = x,  K = in,  N = out, B(k, n) = W[n][k]  (k contiguous rows n),
//             ks = f_in (scales the reduction), ns = f_out
//   dX        A = dy, K = out, N = in,  B(k, n) = W[k][n]  (n contiguous rows k),
//             ks = f_out, ns = f_in
// A workgroup (256 threads) owns a 64 x 64 output tile; wave w owns rows [16 w,
// 16 w + 16) x 64 columns and holds two accumulator sets of four f32x4 (mu and
// sigma).  K-steps of 32 are double-buffered through LDS: the global loads of
// step t + 1 (the A tile ONCE, the two B tiles, the 32-entry ks slice) are
// issued before step t's MFMAs and stored to the other LDS image after them, one
// barrier per step.  The sigma chain's A operand is the LDS value times ks[k] at
// the operand read (one v_mul per MFMA pair).  LDS images follow the operand's
// contiguous dimension (leading dims 36 / 80 as in linear_kernels.hip).  Loads
// are 16-byte or dword, decided once per launch and operand, W_mu and W_sig
// each on its own (base 16-byte aligned, leading dimension and contiguous
// extent multiples of 4: the sigma image of a model starts at any offset); addresses
// are clamped and the values zeroed afterwards (no predicated loads).
// Sum order, the same for both chains: within a K-step a fresh chain from +0
// takes the MFMAs u = 0 .. 7 in order, MFMA u holding k = 32 t + 4 u + {0, 1, 2,
// 3} (the instruction's own k-ordered chain); the K-step sums are then added to
// the running totals, t ascending (two-level, as gemm_kernel).  Epilogue:
//   forward  v = (mu + b_mu[n]) + ns[n] * (sig + b_sig[n]);  act 0 none, 1 ReLU
//            (v > 0 ? v : 0), 2 tanhf;  a NULL bias reads as 0
//   dX       v = mu + ns[n] * sig;  mask (optional): mask[m][n] > 0 ? v : 0
// Two chains were built rather than the single chain over the concatenated K
// ([x | x (.) f_in] against [W_mu | W_sig (.) f_out[n]]): that form folds f_out
// into the B operand (one more rounding per product) and needs the B scale per
// (k, n) element at the operand read, 4x the multiplies; 8 more accumulator
// registers per lane cost no occupancy here (the tile's 60 KiB of LDS already
// limits a CU to two workgroups).
//
// Sigma gradients (noisy_sigma_grad).  g_muW / g_mub of layer l sit at w_off[l]
// / b_off[l] of g_mu_base and the sigma gradients at the same offsets of
// g_sig_base.  g_sigW[n][k] = g_muW[n][k] * (f_out[n] * f_in[k]) (the product in
// parentheses first), g_sigb[n] = g_mub[n] * f_out[n]: plain fp32 products,
// every entry written.  A thread owns four consecutive k of one row: 16-byte
// accesses where the layer allows (in, w_off and the layer's offset in the
// noise image multiples of 4, the three bases 16-byte aligned), dwords otherwise.
#include <math.h>
#include <stdio.h>
#include "smi_device.hpp"
#include "smi_internal.hpp"
#include "philox.hpp"

namespace smi {

constexpr int NZ_BK = 32;
constexpr int NZ_LD_KC = 36;      // [row][k] images (k contiguous)
constexpr int NZ_LD_RC = 80;      // [k][row] images (row contiguous)
constexpr int NZ_STAGE = 2560;    // floats per operand image per stage
constexpr int kNoisyMaxLayers = SMI_NOISY_MAX_LAYERS;

// ----------------------------------------------------------------------- draw
struct NoisyDrawArgs {
  int n;
  int in[kNoisyMaxLayers], out[kNoisyMaxLayers];
  int beg[kNoisyMaxLayers + 1];                  // element prefix of the image
};

__global__ void __launch_bounds__(kWG)
noisy_draw_kernel(uint64_t seed, const int32_t* __restrict__ step, uint32_t stream_id,
                  NoisyDrawArgs a, float* __restrict__ f_image, float* __restrict__ eps_image) {
#pragma clang fp contract(off)
  const uint32_t s = (uint32_t)step[0];
  const int total = a.beg[a.n];
  for (int i = blockIdx.x * kWG + threadIdx.x; i < total; i += gridDim.x * kWG) {
    int l = 0;
#pragma unroll
    for (int j = 1; j < kNoisyMaxLayers; ++j)
      if (j < a.n && i >= a.beg[j]) l = j;
    const uint32_t e = (uint32_t)(i - a.beg[l]);
    uint32_t x0, x1;
    philox_w01((uint32_t)seed, (uint32_t)(seed >> 32), e, (uint32_t)l, s, stream_id, x0, x1);
    const float u1 = ((float)(x0 >> 9) + 0.5f) * 0x1p-23f;
    const float u2 = ((float)(x1 >> 9) + 0.5f) * 0x1p-23f;
    const float eps = sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
    f_image[i] = copysignf(sqrtf(fabsf(eps)), eps);
    if (eps_image) eps_image[i] = eps;
  }
}

int launch_noisy_draw(uint64_t seed, const int32_t* step, int stream_id, int n_layers,
                      const smi_noisy_dims& dims, float* f_image, float* eps_image,
                      hipStream_t st) {
  if (!step || !f_image) return set_error(SMI_E_ARG, "noisy_draw: null pointer");
  if (n_layers < 1 || n_layers > kNoisyMaxLayers || stream_id < 0)
    return set_error(SMI_E_ARG, "noisy_draw: n_layers outside [1, 8] or stream_id < 0");
  NoisyDrawArgs a{};
  a.n = n_layers;
  int64_t tot = 0;
  for (int l = 0; l < n_layers; ++l) {
    if (dims.in_dim[l] < 1 || dims.out_dim[l] < 1)
      return set_error(SMI_E_ARG, "noisy_draw: a layer width < 1");
    a.in[l] = dims.in_dim[l]; a.out[l] = dims.out_dim[l];
    a.beg[l] = (int)tot;
    tot += (int64_t)dims.in_dim[l] + dims.out_dim[l];
    if (tot > (1 << 30)) return set_error(SMI_E_ARG, "noisy_draw: noise image above 2^30 entries");
  }
  a.beg[n_layers] = (int)tot;
  int64_t g = (tot + kWG - 1) / kWG;
  g = g > 1024 ? 1024 : g;
  hipLaunchKernelGGL(noisy_draw_kernel, dim3((unsigned)g), dim3(kWG), 0, st, seed, step,
                     (uint32_t)stream_id, a, f_image, eps_image);
  return check_launch("noisy_draw_kernel");
}

// ----------------------------------------------------------------------- GEMM
struct NoisyGemmArgs {
  int M, N, K;
  const float* A; int64_t lda;                   // A[m*lda + k]
  const float* Bmu; const float* Bsig; int64_t ldb;   // fwd: B[n*ldb + k]; dX: B[k*ldb + n]
  const float* ks;                               // [K] scales the sigma chain's A operand
  const float* ns;                               // [N] scales the sigma sums
  const float* bmu; const float* bsig; int act;  // forward
  const float* mask; int64_t ldm;                // dX
  float* C; int64_t ldc;
  int avec, bmvec, bsvec;                        // 16-byte loads of A, Bmu, Bsig
};

struct NzTile { float v[8]; };

// one 64 (rows) x 32 (k) tile, 8 elements per thread; rows >= rdata and k >= kmax
// read as zero (clamped address, then zeroed).  KC: the rows are k-contiguous
// (row stride ld); otherwise k strides ld and the rows are contiguous.
template <bool KC>
__device__ __forceinline__ void nz_load(const float* __restrict__ P, int64_t ld, int r0, int rdata,
                                        int k0, int kmax, bool vec, NzTile& t) {
  if (vec) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int q = threadIdx.x + j * kWG;
      const int r = KC ? q >> 3 : (q & 15) << 2;
      const int k = KC ? (q & 7) << 2 : q >> 4;
      const int rr = r0 + r, kk = k0 + k;
      // the contiguous extent is a multiple of 4: a quad is all in or all out
      const int rc = rr < rdata ? rr : rdata - (KC ? 1 : 4);
      const int kc = kk < kmax ? kk : kmax - (KC ? 4 : 1);
      const float* src = KC ? P + (int64_t)rc * ld + kc : P + (int64_t)kc * ld + rc;
      const float4 x = *reinterpret_cast<const float4*>(src);
      const bool ok = rr < rdata && kk < kmax;
      t.v[4 * j + 0] = ok ? x.x : 0.f; t.v[4 * j + 1] = ok ? x.y : 0.f;
      t.v[4 * j + 2] = ok ? x.z : 0.f; t.v[4 * j + 3] = ok ? x.w : 0.f;
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int idx = threadIdx.x + j * kWG;
    const int r = KC ? idx >> 5 : idx & 63;
    const int k = KC ? idx & 31 : idx >> 6;
    const int rr = r0 + r, kk = k0 + k;
    const int rc = rr < rdata ? rr : rdata - 1;
    const int kc = kk < kmax ? kk : kmax - 1;
    const float x = KC ? P[(int64_t)rc * ld + kc] : P[(int64_t)kc * ld + rc];
    t.v[j] = (rr < rdata && kk < kmax) ? x : 0.f;
  }
}

template <bool KC>
__device__ __forceinline__ void nz_store(float* __restrict__ S, bool vec, const NzTile& t) {
  if (vec) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int q = threadIdx.x + j * kWG;
      const float4 x = float4{t.v[4 * j], t.v[4 * j + 1], t.v[4 * j + 2], t.v[4 * j + 3]};
      if (KC) *reinterpret_cast<float4*>(S + (q >> 3) * NZ_LD_KC + ((q & 7) << 2)) = x;
      else *reinterpret_cast<float4*>(S + (q >> 4) * NZ_LD_RC + ((q & 15) << 2)) = x;
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int idx = threadIdx.x + j * kWG;
    if (KC) S[(idx >> 5) * NZ_LD_KC + (idx & 31)] = t.v[j];
    else S[(idx >> 6) * NZ_LD_RC + (idx & 63)] = t.v[j];
  }
}

template <bool DX>
__global__ void __launch_bounds__(kWG)
noisy_gemm_kernel(NoisyGemmArgs g) {
#pragma clang fp contract(off)
  constexpr bool BK = !DX;                       // B rows (n) k-contiguous
  __shared__ __attribute__((aligned(16))) float sA[2][NZ_STAGE];
  __shared__ __attribute__((aligned(16))) float sM[2][NZ_STAGE];
  __shared__ __attribute__((aligned(16))) float sS[2][NZ_STAGE];
  __shared__ float sF[2][NZ_BK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int m0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
  const int nk = (g.K + NZ_BK - 1) / NZ_BK;
  f32x4 tmu[4], tsg[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    tmu[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    tsg[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  NzTile ra, rm, rs;
  float rf = 0.f;
  auto load = [&](int kt) {
    const int k0 = kt * NZ_BK;
    nz_load<true>(g.A, g.lda, m0, g.M, k0, g.K, g.avec, ra);
    nz_load<BK>(g.Bmu, g.ldb, n0, g.N, k0, g.K, g.bmvec, rm);
    nz_load<BK>(g.Bsig, g.ldb, n0, g.N, k0, g.K, g.bsvec, rs);
    const int kk = k0 + (tid & 31);
    const float x = g.ks[kk < g.K ? kk : g.K - 1];
    rf = kk < g.K ? x : 0.f;
  };
  auto store = [&](int sidx) {
    nz_store<true>(sA[sidx], g.avec, ra);
    nz_store<BK>(sM[sidx], g.bmvec, rm);
    nz_store<BK>(sS[sidx], g.bsvec, rs);
    if (tid < NZ_BK) sF[sidx][tid] = rf;
  };
  load(0);
  store(0);
  __syncthreads();
  const int ar = wave * 16 + li;
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) load(kt + 1);
    const float* As = sA[cur];
    const float* Ms = sM[cur];
    const float* Ss = sS[cur];
    const float* Fs = sF[cur];
    f32x4 amu[4], asg[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      amu[c] = f32x4{0.f, 0.f, 0.f, 0.f};
      asg[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    float av[8], as[8], bm[4][8], bs[4][8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = 4 * u + lk;
      av[u] = As[ar * NZ_LD_KC + k];
      as[u] = av[u] * Fs[k];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int n = c * 16 + li;
        bm[c][u] = BK ? Ms[n * NZ_LD_KC + k] : Ms[k * NZ_LD_RC + n];
        bs[c][u] = BK ? Ss[n * NZ_LD_KC + k] : Ss[k * NZ_LD_RC + n];
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        amu[c] = mfma4(av[u], bm[c][u], amu[c]);
        asg[c] = mfma4(as[u], bs[c][u], asg[c]);
      }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      tmu[c] += amu[c];
      tsg[c] += asg[c];
    }
    if (kt + 1 < nk) store(cur ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int n = n0 + c * 16 + li;
    if (n >= g.N) continue;
    const float sn = g.ns[n];
    float b_mu = 0.f, b_sg = 0.f;
    if constexpr (!DX) {
      b_mu = g.bmu ? g.bmu[n] : 0.f;
      b_sg = g.bsig ? g.bsig[n] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + wave * 16 + lk * 4 + i;
      if (m >= g.M) continue;
      float v;
      if constexpr (!DX) {
        v = (tmu[c][i] + b_mu) + sn * (tsg[c][i] + b_sg);
        if (g.act == ACT_RELU) v = v > 0.f ? v : 0.f;
        else if (g.act == ACT_TANH) v = tanhf(v);
      } else {
        v = tmu[c][i] + sn * tsg[c][i];
        if (g.mask) v = g.mask[(int64_t)m * g.ldm + n] > 0.f ? v : 0.f;
      }
      g.C[(int64_t)m * g.ldc + n] = v;
    }
  }
}

static bool nz_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int launch_noisy_fwd(const float* x, int64_t ldx, int rows, int in_dim, const float* w_mu,
                     const float* w_sig, int64_t ldw, const float* b_mu, const float* b_sig,
                     const float* f_in, const float* f_out, int out_dim, int act, float* y,
                     int64_t ldy, hipStream_t st) {
  if (!x || !w_mu || !w_sig || !f_in || !f_out || !y)
    return set_error(SMI_E_ARG, "noisy_forward: null pointer");
  if (rows < 1 || in_dim < 1 || out_dim < 1)
    return set_error(SMI_E_ARG, "noisy_forward: rows, in_dim or out_dim < 1");
  if (ldx < in_dim || ldw < in_dim || ldy < out_dim)
    return set_error(SMI_E_ARG, "noisy_forward: leading dims too small");
  if (act != ACT_NONE && act != ACT_RELU && act != ACT_TANH)
    return set_error(SMI_E_ARG, "noisy_forward: act 0/1/2");
  NoisyGemmArgs g{};
  g.M = rows; g.N = out_dim; g.K = in_dim;
  g.A = x; g.lda = ldx;
  g.Bmu = w_mu; g.Bsig = w_sig; g.ldb = ldw;
  g.ks = f_in; g.ns = f_out; g.bmu = b_mu; g.bsig = b_sig; g.act = act;
  g.C = y; g.ldc = ldy;
  g.avec = nz_al16(x) && ldx % 4 == 0 && in_dim % 4 == 0;
  g.bmvec = nz_al16(w_mu) && ldw % 4 == 0 && in_dim % 4 == 0;
  g.bsvec = nz_al16(w_sig) && ldw % 4 == 0 && in_dim % 4 == 0;
  const dim3 grid((rows + 63) / 64, (out_dim + 63) / 64);
  const int kslot = ktime_begin(st);
  hipLaunchKernelGGL(noisy_gemm_kernel<false>, grid, dim3(kWG), 0, st, g);
  ktime_end(kslot, KT_GEMM_FWD, 4.0 * rows * (double)out_dim * in_dim, st);
  return check_launch("noisy_gemm_kernel<fwd>");
}

int launch_noisy_bwd_dx(const float* dy, int64_t ldg, int rows, int out_dim, const float* w_mu,
                        const float* w_sig, int64_t ldw, int in_dim, const float* f_in,
                        const float* f_out, const float* mask, int64_t ldm, float* dx,
                        int64_t lddx, hipStream_t st) {
  if (!dy || !w_mu || !w_sig || !f_in || !f_out || !dx)
    return set_error(SMI_E_ARG, "noisy_backward_input: null pointer");
  if (rows < 1 || in_dim < 1 || out_dim < 1)
    return set_error(SMI_E_ARG, "noisy_backward_input: rows, in_dim or out_dim < 1");
  if (ldg < out_dim || ldw < in_dim || lddx < in_dim || (mask && ldm < in_dim))
    return set_error(SMI_E_ARG, "noisy_backward_input: leading dims too small");
  NoisyGemmArgs g{};
  g.M = rows; g.N = in_dim; g.K = out_dim;
  g.A = dy; g.lda = ldg;
  g.Bmu = w_mu; g.Bsig = w_sig; g.ldb = ldw;
  g.ks = f_out; g.ns = f_in; g.mask = mask; g.ldm = ldm;
  g.C = dx; g.ldc = lddx;
  g.avec = nz_al16(dy) && ldg % 4 == 0 && out_dim % 4 == 0;
  g.bmvec = nz_al16(w_mu) && ldw % 4 == 0 && in_dim % 4 == 0;
  g.bsvec = nz_al16(w_sig) && ldw % 4 == 0 && in_dim % 4 == 0;
  const dim3 grid((rows + 63) / 64, (in_dim + 63) / 64);
  const int kslot = ktime_begin(st);
  hipLaunchKernelGGL(noisy_gemm_kernel<true>, grid, dim3(kWG), 0, st, g);
  ktime_end(kslot, KT_GEMM_DX, 4.0 * rows * (double)out_dim * in_dim, st);
  return check_launch("noisy_gemm_kernel<dx>");
}

// ------------------------------------------------------------ sigma gradients
struct NoisySigArgs {
  const float* gmu; float* gsig; const float* f;
  int n;
  int64_t woff[kNoisyMaxLayers], boff[kNoisyMaxLayers];
  int64_t ubeg[kNoisyMaxLayers + 1];             // unit prefix: out * ceil(in / 4) quads + out biases
  int in[kNoisyMaxLayers], out[kNoisyMaxLayers], foff[kNoisyMaxLayers];
  unsigned vec;                                  // bit l: 16-byte accesses on layer l
};

__global__ void __launch_bounds__(kWG)
noisy_sigma_grad_kernel(NoisySigArgs a) {
#pragma clang fp contract(off)
  const int64_t total = a.ubeg[a.n];
  for (int64_t i = (int64_t)blockIdx.x * kWG + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * kWG) {
    int l = 0;
#pragma unroll
    for (int j = 1; j < kNoisyMaxLayers; ++j)
      if (j < a.n && i >= a.ubeg[j]) l = j;
    const int in = a.in[l], out = a.out[l];
    const int qpr = (in + 3) >> 2;
    const int64_t u = i - a.ubeg[l];
    const float* fi = a.f + a.foff[l];
    const float* fo = fi + in;
    if (u >= (int64_t)out * qpr) {                // bias entry
      const int n = (int)(u - (int64_t)out * qpr);
      a.gsig[a.boff[l] + n] = a.gmu[a.boff[l] + n] * fo[n];
      continue;
    }
    const int n = (int)(u / qpr), k = (int)(u - (int64_t)n * qpr) << 2;
    const float fn = fo[n];
    const int64_t o = a.woff[l] + (int64_t)n * in + k;
    if ((a.vec >> l) & 1u) {
      const float4 gq = *reinterpret_cast<const float4*>(a.gmu + o);
      const float4 fq = *reinterpret_cast<const float4*>(fi + k);
      *reinterpret_cast<float4*>(a.gsig + o) =
          float4{gq.x * (fn * fq.x), gq.y * (fn * fq.y), gq.z * (fn * fq.z), gq.w * (fn * fq.w)};
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (k + t < in) a.gsig[o + t] = a.gmu[o + t] * (fn * fi[k + t]);
    }
  }
}

int launch_noisy_sigma_grad(const float* g_mu_base, float* g_sig_base, const float* f_image,
                            int n_layers, const smi_noisy_table& tab, hipStream_t st) {
  if (!g_mu_base || !g_sig_base || !f_image)
    return set_error(SMI_E_ARG, "noisy_sigma_grad: null pointer");
  if (n_layers < 1 || n_layers > kNoisyMaxLayers)
    return set_error(SMI_E_ARG, "noisy_sigma_grad: n_layers outside [1, 8]");
  NoisySigArgs a{};
  a.gmu = g_mu_base; a.gsig = g_sig_base; a.f = f_image; a.n = n_layers;
  const bool al = nz_al16(g_mu_base) && nz_al16(g_sig_base) && nz_al16(f_image);
  int64_t foff = 0, units = 0;
  for (int l = 0; l < n_layers; ++l) {
    const int in = tab.in_dim[l], out = tab.out_dim[l];
    if (in < 1 || out < 1 || tab.w_off[l] < 0 || tab.b_off[l] < 0)
      return set_error(SMI_E_ARG, "noisy_sigma_grad: a layer width < 1 or an offset < 0");
    a.in[l] = in; a.out[l] = out; a.woff[l] = tab.w_off[l]; a.boff[l] = tab.b_off[l];
    a.foff[l] = (int)foff;
    a.ubeg[l] = units;
    if (al && in % 4 == 0 && tab.w_off[l] % 4 == 0 && foff % 4 == 0) a.vec |= 1u << l;
    foff += (int64_t)in + out;
    if (foff > (1 << 30)) return set_error(SMI_E_ARG, "noisy_sigma_grad: noise image above 2^30 entries");
    units += (int64_t)out * ((in + 3) / 4) + out;
  }
  a.ubeg[n_layers] = units;
  int64_t g = (units + kWG - 1) / kWG;
  g = g > 4096 ? 4096 : g;
  hipLaunchKernelGGL(noisy_sigma_grad_kernel, dim3((unsigned)g), dim3(kWG), 0, st, a);
  return check_launch("noisy_sigma_grad_kernel");
}

}  // namespace smi
