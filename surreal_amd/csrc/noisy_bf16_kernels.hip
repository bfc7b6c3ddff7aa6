// noisy_bf16_kernels.hip — the noisy linear layer's forward and input gradient
// (noisy_kernels.hip's noisy_gemm) with bf16 operands on
// v_mfma_f32_16x16x32_bf16.  The specification is this project's own; tensors
// stay fp32 in memory:
//   fwd: y[m][n]  = act((S_mu + b_mu[n]) + f_out[n] * (S_sig + b_sig[n]))
//        S_mu  = sum_k bf16(x[m][k])            * bf16(W_mu[n][k])
//        S_sig = sum_k bf16(x[m][k] * f_in[k])  * bf16(W_sig[n][k])
//   dX:  dx[m][k] = [mask[m][k] > 0] * (T_mu + f_in[k] * T_sig)
//        T_mu  = sum_n bf16(dy[m][n])            * bf16(W_mu[n][k])
//        T_sig = sum_n bf16(dy[m][n] * f_out[n]) * bf16(W_sig[n][k])
// bf16() is pack8's rounding (bf16_stage.hpp: nearest even, NaN and infinities
// preserved).  The product with the noise vector is ONE fp32 multiply of the
// unrounded activation, rounded once afterwards (not a rounded activation times
// the noise).  Products of two bf16 values are exact in fp32 and the MFMA
// accumulates in fp32.  The epilogue is fp32 in the order written, which is
// the fp32 kernel's; no contraction into fma (#pragma clang fp contract(off)
// over every kernel below).  NULL biases read as 0; act 0 none, 1 ReLU (v > 0 ?
// v : 0), 2 tanhf; the mask (optional) selects v or +0.
//
// Both directions are  C[m][j] = epi(sum_z A[m][z] Bmu[j][z], sum_z (A[m][z]
// ks[z]) Bsig[j][z])  (fwd: A = x, B = W, z = k, ks = f_in, ns = f_out; dX: A =
// dy, B = W^T, z = n, ks = f_out, ns = f_in).  The kernel follows
// linear_bf16_kernels.hip: 256 threads, wave w owns rows 16 w .. 16 w + 15 of a
// 64-row tile and TWO accumulator sets (mu, sigma) of NT f32x4: NT = 4, the
// 64 x 64 form, or NT = 1, the 64 x 16 form of the head layers (outputs <= 16).
// The reduction runs in chunks of 64, two LDS stages, one barrier per chunk; the
// global loads of chunk c + 1 are issued into registers before chunk c's MFMAs
// (2 k-steps x 2 chains x NT) and rounded into the other stage after them.
//
// LDS: four bf16 images per stage, all [row][z] in 16-byte vectors of 8 bf16, a
// row 9 vectors (144 bytes = 36 dwords): A_mu = bf16(a), A_sig = bf16(a ks[z])
// (64 rows each), B_mu, B_sig (16 NT rows each); NT = 4: 72 KiB (dynamic LDS, two
// workgroups per CU), NT = 1: 45 KiB.  Both A images come from ONE global load
// of the activation: the chunk's ks slice is fetched with the prefetch and the
// multiply happens in the staging registers just before pack8 (scaling at the
// operand read, as the fp32 kernel does, would unpack / multiply / repack per
// MFMA).  Banks: every image starts a multiple of 16 rows = 576 dwords = 9 x 64
// after the first, so an image's base adds nothing mod 64 and the plain
// kernel's argument holds for the third and the fourth image as for the first
// two: an operand read's 16 lanes hold rows r0 .. r0 + 15 at one z group and
// start at dwords 36 r mod 64, 16 different multiples of 4 (every bank once);
// the z-contiguous staging store (thread: row t >> 3, vector t & 7) is 2-way on
// 4 banks at worst; the transposed store starts at 16 (t & 3) + 4 zo + 36 c mod
// 64 (every bank once).
//
// Staging, what a thread carries between fetch and stage:
//   A     every thread, both directions: rows t >> 3 and (t >> 3) + 32, 8
//         consecutive z each (16 floats), and the 8 ks of those z (8 floats;
//         the slice is the same for both rows)
//   fwd   NT = 4: the same two rows of W_mu and of W_sig (32 floats); NT = 1:
//         waves 0 and 1 row t' >> 3 of W_mu, waves 2 and 3 of W_sig (8 floats)
//   dX    W's rows are the reduction: transposed in registers by load_t4x8 and
//         the plain kernel's store map (t' = t & 127: column quad cq = (t' & 3) |
//         (t' >> 5) << 2, z octet zo = (t' >> 2) & 7, threads t' < 32 NT): waves 0
//         and 1 take W_mu, waves 2 and 3 W_sig (32 floats)
// so every thread prefetches 56 floats in the 64-wide forms (32 in fwd,16; in
// dx,16 the 32 threads t' < 32 of each wave pair carry 56 and the others 24, as
// in the plain kernel's 16-wide input gradient).  Registers: the end of this
// comment.
//
// Edges: any M, K, N >= 1; clamped addresses, values zeroed by a select, no
// predicated loads (bf16_loads.hpp).  16-byte or dword loads are decided once
// per launch and PER OPERAND: A, W_mu, W_sig and ks each on its own (base
// alignment, leading dimension and contiguous extent multiples of 4 floats):
// the sigma image of a model and a layer's noise slice start at any offset.
// A padded z has a = 0 and ks = 0 (0 * 0, never 0 * NaN); a padded row may form
// 0 * ks = NaN for a non-finite ks, in a row that is never stored.
//
// Split-K (linear_bf16_plan.hpp, with half the workspace: two chains): fewer
// than 256 tiles over at least 4 chunks are cut over gridDim.z into slabs of a
// multiple of 64, at least two chunks each.  Slab z writes its raw mu sums to
// part[z] and its sigma sums to part[S + z] ([2 S][M][N] in the library
// workspace); noisy_bf16_reduce_kernel sums both in a fixed order and applies
// the epilogue above.  No atomics: two calls give the same bits.
//
// Sum order of one output, the same for both chains: within a 32-wide k-step
// the instruction's own chain; the two k-steps of a chunk and the chunks of a
// slab ascending into the running accumulator; in the reducer four lanes, lane
// j taking slabs j, j + 4, .. ascending from +0, then (l0 + l1) + (l2 + l3).
//
// VGPRs / dynamic LDS bytes of the four forms as built (no scratch, no spills):
// fwd,64 124 / 73728; dx,64 130 / 73728; fwd,16 72 / 46080; dx,16 108 / 46080.
// The 64-wide forms keep 3 waves per SIMD by registers; their LDS admits two
// workgroups per CU (2 waves per SIMD), the fp32 kernel's residency.
#include <cmath>
#define SMI_GEMM_UNIT gemm_noisy_bf16
#include "gemm_args.hpp"
#include "bf16_stage.hpp"
#include "bf16_loads.hpp"
#include "linear_bf16_plan.hpp"

namespace smi {

namespace {

constexpr int LDV = kLinBfLdv;
static_assert(kWG == 256 && kLinBfRows == 64 && kLinBfChunk == 64 && LDV == 9,
              "the staging maps below are written for 256 threads and 64 x 64 slices");

struct NoisyBfArgs {
  int M, N, K;                                   // C [M][N], reduction K
  const float* A; int64_t lda;                   // A[m*lda + z]
  const float* Bmu; const float* Bsig; int64_t ldb;   // fwd: B[j*ldb + z]; dX: B[z*ldb + j]
  const float* ks;                               // [K] scales the sigma chain's A operand
  const float* ns;                               // [N] scales the sigma sums
  const float* bmu; const float* bsig; int act;  // forward
  const float* mask; int64_t ldm;                // dX
  float* C; int64_t ldc;
  int kchunk;                                    // reduction range of slab z: [z kchunk, ..)
  int splits; float* part;                       // split-K partials [2 splits][M][N] (nullptr: none)
  int avec, bmvec, bsvec, kvec;                  // 16-byte loads of A, Bmu, Bsig, ks
};

// stage bytes of a form: two A images of 64 rows and two B images of 16 NT rows
constexpr int noisy_bf16_lds_bytes(int nt) { return 2 * 2 * (kLinBfRows + 16 * nt) * LDV * 16; }

template <int EPI>
__device__ __forceinline__ float noisy_epilogue(const NoisyBfArgs& g, int m, int n, float mu,
                                                float sig, float sn, float b_mu, float b_sg) {
#pragma clang fp contract(off)
  float v;
  if constexpr (EPI == EPI_FWD) {
    v = (mu + b_mu) + sn * (sig + b_sg);
    if (g.act == ACT_RELU) v = v > 0.f ? v : 0.f;
    else if (g.act == ACT_TANH) v = tanhf(v);
  } else {
    v = mu + sn * sig;
    if (g.mask) v = g.mask[(int64_t)m * g.ldm + n] > 0.f ? v : 0.f;
  }
  return v;
}

}  // namespace

// grid (row tiles, column tiles, slabs)
template <int EPI, int NT>
__global__ void __launch_bounds__(kWG)
noisy_bf16_kernel(NoisyBfArgs g) {
#pragma clang fp contract(off)
  constexpr int BR = 16 * NT;                         // columns of the tile = rows of a B image
  constexpr int NB = EPI == EPI_FWD ? 8 * NT : 32;    // B floats a thread prefetches
  constexpr int IMG = (2 * kLinBfRows + 2 * BR) * LDV;   // vectors per stage
  extern __shared__ uint4 lds[];
  const int tid = threadIdx.x, l = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const TileIdx ti = gemm_tile_index();
  const int m0 = ti.mt * kLinBfRows, n0 = ti.nt * BR;
  const int zb = ti.z * g.kchunk;
  const int ze = min(g.K, zb + g.kchunk);
  const int nc = (ze - zb + kLinBfChunk - 1) / kLinBfChunk;
  const int ar = tid >> 3, av = tid & 7;              // A and forward-B staging: row, vector
  const int t2 = tid & 127;                           // index within the wave pair
  const int cq = (t2 & 3) | ((t2 >> 5) << 2), zo = (t2 >> 2) & 7;
  const bool sigw = w >= 2;                           // this wave pair stages W_sig (uniform)
  const float* Bw = sigw ? g.Bsig : g.Bmu;
  const bool bwvec = sigw ? g.bsvec : g.bmvec;

  float pa[16], pk[8], pb[NB];
  auto fetch = [&](int z0) {
    const int z = z0 + 8 * av;
#pragma unroll
    for (int h = 0; h < 2; ++h) load_z8(g.A, g.lda, m0 + ar + 32 * h, g.M, z, ze, g.avec, pa + 8 * h);
    load_z8(g.ks, 0, 0, 1, z, ze, g.kvec, pk);
    if constexpr (EPI == EPI_FWD) {
      if constexpr (NT == 4) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          load_z8(g.Bmu, g.ldb, n0 + ar + 32 * h, g.N, z, ze, g.bmvec, pb + 8 * h);
          load_z8(g.Bsig, g.ldb, n0 + ar + 32 * h, g.N, z, ze, g.bsvec, pb + 16 + 8 * h);
        }
      } else {
        load_z8(Bw, g.ldb, n0 + (t2 >> 3), g.N, z, ze, bwvec, pb);
      }
    } else {
      if (t2 < 32 * NT) load_t4x8(Bw, g.ldb, z0 + 8 * zo, ze, n0 + 4 * cq, g.N, bwvec, pb);
    }
  };
  auto stage = [&](int s) {
    uint4* Sam = lds + s * IMG;
    uint4* Sas = Sam + kLinBfRows * LDV;
    uint4* Sbm = Sas + kLinBfRows * LDV;
    uint4* Sbs = Sbm + BR * LDV;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float sv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) sv[e] = pa[8 * h + e] * pk[e];   // one fp32 product, rounded below
      Sam[(ar + 32 * h) * LDV + av] = pack8(pa + 8 * h);
      Sas[(ar + 32 * h) * LDV + av] = pack8(sv);
    }
    if constexpr (EPI == EPI_FWD) {
      if constexpr (NT == 4) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          Sbm[(ar + 32 * h) * LDV + av] = pack8(pb + 8 * h);
          Sbs[(ar + 32 * h) * LDV + av] = pack8(pb + 16 + 8 * h);
        }
      } else {
        (sigw ? Sbs : Sbm)[(t2 >> 3) * LDV + av] = pack8(pb);
      }
    } else {
      if (t2 < 32 * NT) {
        uint4* Sb = sigw ? Sbs : Sbm;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float col[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) col[e] = pb[4 * e + c];
          Sb[(4 * cq + c) * LDV + zo] = pack8(col);
        }
      }
    }
  };

  f32x4 amu[NT], asg[NT];
#pragma unroll
  for (int c = 0; c < NT; ++c) {
    amu[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    asg[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int lm = l & 15, lg = l >> 4;
  if (nc > 0) {
    fetch(zb);
    stage(0);
  }
  __syncthreads();
  for (int c = 0; c < nc; ++c) {
    const bool more = c + 1 < nc;
    if (more) fetch(zb + (c + 1) * kLinBfChunk);
    const uint4* ap = lds + (c & 1) * IMG + (16 * w + lm) * LDV + lg;
    const uint4* bp = lds + (c & 1) * IMG + (2 * kLinBfRows + lm) * LDV + lg;
    // every operand of the chunk first (one LDS round trip), then its MFMAs
    uint4 a[2][2], b[2][NT][2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      a[0][kk] = ap[4 * kk];
      a[1][kk] = ap[kLinBfRows * LDV + 4 * kk];
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        b[0][t][kk] = bp[16 * t * LDV + 4 * kk];
        b[1][t][kk] = bp[(BR + 16 * t) * LDV + 4 * kk];
      }
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        amu[t] = mfma32(a[0][kk], b[0][t][kk], amu[t]);
        asg[t] = mfma32(a[1][kk], b[1][t][kk], asg[t]);
      }
    if (more) stage((c + 1) & 1);
    __syncthreads();
  }

  // epilogue: 4 rows x NT columns per lane (D[row 4 lg + e][col lm])
  const int64_t MN = (int64_t)g.M * g.N;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n = n0 + 16 * t + lm;
    if (n >= g.N) continue;
    const float sn = g.ns[n];
    float b_mu = 0.f, b_sg = 0.f;
    if constexpr (EPI == EPI_FWD) {
      b_mu = g.bmu ? g.bmu[n] : 0.f;
      b_sg = g.bsig ? g.bsig[n] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int m = m0 + 16 * w + 4 * lg + e;
      if (m >= g.M) continue;
      if (g.part) {                                   // split-K slab: raw sums of both chains
        const int64_t o = (int64_t)m * g.N + n;
        g.part[ti.z * MN + o] = amu[t][e];
        g.part[(g.splits + ti.z) * MN + o] = asg[t][e];
        continue;
      }
      g.C[(int64_t)m * g.ldc + n] = noisy_epilogue<EPI>(g, m, n, amu[t][e], asg[t][e], sn, b_mu, b_sg);
    }
  }
}

// split-K reducer: a workgroup owns 64 consecutive outputs x 4 slab lanes; lane
// zl sums slabs zl, zl + 4, .. of both chains ascending, the 4 lane sums are
// combined through LDS in a fixed order, then the layer's epilogue
template <int EPI>
__global__ void __launch_bounds__(kWG)
noisy_bf16_reduce_kernel(NoisyBfArgs g) {
#pragma clang fp contract(off)
  __shared__ float red[2][4][64];
  const int S = g.splits;
  const int64_t MN = (int64_t)g.M * g.N;
  const int el = threadIdx.x & 63, zl = threadIdx.x >> 6;
  const int64_t e = (int64_t)blockIdx.x * 64 + el;
  const int64_t ec = e < MN ? e : MN - 1;
  float smu = 0.f, ssg = 0.f;
  for (int z = zl; z < S; z += 4) {
    smu += g.part[z * MN + ec];
    ssg += g.part[(S + z) * MN + ec];
  }
  red[0][zl][el] = smu;
  red[1][zl][el] = ssg;
  __syncthreads();
  if (zl != 0 || e >= MN) return;
  const float mu = (red[0][0][el] + red[0][1][el]) + (red[0][2][el] + red[0][3][el]);
  const float sig = (red[1][0][el] + red[1][1][el]) + (red[1][2][el] + red[1][3][el]);
  const int m = (int)(e / g.N), n = (int)(e - (int64_t)m * g.N);
  float b_mu = 0.f, b_sg = 0.f;
  if constexpr (EPI == EPI_FWD) {
    b_mu = g.bmu ? g.bmu[n] : 0.f;
    b_sg = g.bsig ? g.bsig[n] : 0.f;
  }
  g.C[(int64_t)m * g.ldc + n] = noisy_epilogue<EPI>(g, m, n, mu, sig, g.ns[n], b_mu, b_sg);
}

// ------------------------------------------------------------------- host
static bool nzb_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int noisy_bf16_launch(int epi, NoisyBfArgs g, hipStream_t st) {
  const bool fwd = epi == EPI_FWD;
  // half the workspace per chain: the plan's capacity test counts one image
  const LinBfPlan pl = linear_bf16_plan(g.M, g.N, g.K, smi_workspace_floats() / 2);
  g.kchunk = pl.kchunk;
  g.splits = pl.splits;
  g.part = nullptr;
  if (pl.splits > 1) {
    g.part = workspace_f32(2 * (int64_t)pl.splits * g.M * g.N);
    if (!g.part) return set_error(SMI_E_ARG, "noisy bf16: workspace unavailable for split-K");
  }
  const dim3 grid(pl.gm, pl.gn, pl.splits);
  const size_t lds = noisy_bf16_lds_bytes(pl.nt);
  const char* form;
  const char* red;
  const int kslot = ktime_begin(st);
#define SMI_NBF(E, NTV, NAME)                                                               \
  do {                                                                                      \
    allow_lds(noisy_bf16_kernel<E, NTV>, lds);                                              \
    hipLaunchKernelGGL((noisy_bf16_kernel<E, NTV>), grid, dim3(kWG), lds, st, g);           \
    form = "noisy_bf16_kernel<" NAME ">";                                                   \
    red = "noisy_bf16_reduce_kernel<noisy_bf16_kernel<" NAME ">>";                          \
  } while (0)
  if (fwd) { if (pl.nt == 4) SMI_NBF(EPI_FWD, 4, "fwd,64"); else SMI_NBF(EPI_FWD, 1, "fwd,16"); }
  else { if (pl.nt == 4) SMI_NBF(EPI_DX, 4, "dx,64"); else SMI_NBF(EPI_DX, 1, "dx,16"); }
#undef SMI_NBF
  ktime_end(kslot, fwd ? KT_GEMM_FWD : KT_GEMM_DX, 4.0 * g.M * (double)g.N * g.K, st);
  const int rc = check_launch(form);
  if (rc || pl.splits == 1) return rc;
  // the reducer is the last launch of a split call and names the form it sums
  const int rslot = ktime_begin(st);
  const int64_t MN = (int64_t)g.M * g.N;
  const dim3 rgrid((unsigned)((MN + 63) / 64));
  if (fwd) hipLaunchKernelGGL(noisy_bf16_reduce_kernel<EPI_FWD>, rgrid, dim3(kWG), 0, st, g);
  else hipLaunchKernelGGL(noisy_bf16_reduce_kernel<EPI_DX>, rgrid, dim3(kWG), 0, st, g);
  ktime_end(rslot, KT_GEMM_REDUCE, 2.0 * pl.splits * MN, st);
  return check_launch(red);
}

int launch_noisy_fwd_bf16(const float* x, int64_t ldx, int rows, int in_dim, const float* w_mu,
                          const float* w_sig, int64_t ldw, const float* b_mu, const float* b_sig,
                          const float* f_in, const float* f_out, int out_dim, int act, float* y,
                          int64_t ldy, hipStream_t st) {
  if (!x || !w_mu || !w_sig || !f_in || !f_out || !y)
    return set_error(SMI_E_ARG, "noisy_forward_bf16: null pointer");
  if (rows < 1 || in_dim < 1 || out_dim < 1)
    return set_error(SMI_E_ARG, "noisy_forward_bf16: rows, in_dim or out_dim < 1");
  if (ldx < in_dim || ldw < in_dim || ldy < out_dim)
    return set_error(SMI_E_ARG, "noisy_forward_bf16: leading dims too small");
  if (act != ACT_NONE && act != ACT_RELU && act != ACT_TANH)
    return set_error(SMI_E_ARG, "noisy_forward_bf16: act 0/1/2");
  NoisyBfArgs g{};
  g.M = rows; g.N = out_dim; g.K = in_dim;
  g.A = x; g.lda = ldx;
  g.Bmu = w_mu; g.Bsig = w_sig; g.ldb = ldw;          // B(z = k, j = n) = W[n][k]
  g.ks = f_in; g.ns = f_out; g.bmu = b_mu; g.bsig = b_sig; g.act = act;
  g.C = y; g.ldc = ldy;
  // every operand is z-contiguous: quads along k
  g.avec = nzb_al16(x) && ldx % 4 == 0 && in_dim % 4 == 0;
  g.bmvec = nzb_al16(w_mu) && ldw % 4 == 0 && in_dim % 4 == 0;
  g.bsvec = nzb_al16(w_sig) && ldw % 4 == 0 && in_dim % 4 == 0;
  g.kvec = nzb_al16(f_in) && in_dim % 4 == 0;
  return noisy_bf16_launch(EPI_FWD, g, st);
}

int launch_noisy_bwd_dx_bf16(const float* dy, int64_t ldg, int rows, int out_dim, const float* w_mu,
                             const float* w_sig, int64_t ldw, int in_dim, const float* f_in,
                             const float* f_out, const float* mask, int64_t ldm, float* dx,
                             int64_t lddx, hipStream_t st) {
  if (!dy || !w_mu || !w_sig || !f_in || !f_out || !dx)
    return set_error(SMI_E_ARG, "noisy_backward_input_bf16: null pointer");
  if (rows < 1 || in_dim < 1 || out_dim < 1)
    return set_error(SMI_E_ARG, "noisy_backward_input_bf16: rows, in_dim or out_dim < 1");
  if (ldg < out_dim || ldw < in_dim || lddx < in_dim || (mask && ldm < in_dim))
    return set_error(SMI_E_ARG, "noisy_backward_input_bf16: leading dims too small");
  NoisyBfArgs g{};
  g.M = rows; g.N = in_dim; g.K = out_dim;
  g.A = dy; g.lda = ldg;
  g.Bmu = w_mu; g.Bsig = w_sig; g.ldb = ldw;          // B(z = n', j = k') = W[n'][k']
  g.ks = f_out; g.ns = f_in; g.mask = mask; g.ldm = ldm;
  g.C = dx; g.ldc = lddx;
  // dy and f_out in quads along z = n, W in quads along its columns
  g.avec = nzb_al16(dy) && ldg % 4 == 0 && out_dim % 4 == 0;
  g.bmvec = nzb_al16(w_mu) && ldw % 4 == 0 && in_dim % 4 == 0;
  g.bsvec = nzb_al16(w_sig) && ldw % 4 == 0 && in_dim % 4 == 0;
  g.kvec = nzb_al16(f_out) && out_dim % 4 == 0;
  return noisy_bf16_launch(EPI_DX, g, st);
}

}  // namespace smi
