// lstm_mfma.hip — the nn.LSTM stem of PPOModel (surreal/model/ppo_net.py:
// 137-152, 277-279, 310-312) as persistent sequence kernels for gfx950.
//
// The input projection x W_ih^T + b_ih of every step is one large GEMM
// (linear_kernels.hip) before the recurrence; what stays sequential is
//   gates_t = xproj_t + (h_{t-1} W_hh^T + b_hh)          [torch order i,f,g,o]
//   c_t = sigmoid(f) c_{t-1} + sigmoid(i) tanh(g),  h_t = sigmoid(o) tanh(c_t)
// Segments are independent, so one workgroup owns 16 segments for ALL steps
// (no inter-workgroup synchronisation): h_{t-1} lives in LDS as the MFMA A
// operand, c_{t-1} in registers, W_hh streams from L2 (160 KB at H = 100,
// shared by every workgroup).  Wave w owns hidden-unit tiles ut = w, w+4, ...
// of 16 units and computes the four gate columns of each (4 accumulators of
// v_mfma_f32_16x16x4_f32), so the cell update happens in the MFMA output
// registers: lane (li, lk) holds rows lk*4..lk*4+3 of unit ut*16+li.
//
// Backward (BPTT, reverse over steps) keeps dh_rec and dc in the same
// registers: dgates_t are formed element-wise, written to HBM (for the weight
// GEMMs) and to LDS, and dh_rec_{t-1} = dgates_t W_hh is the next MFMA pass
// (K = 4H, B operand contiguous along units).
//
// This unit: the matrix-core forms (H <= 128 at four segments per workgroup,
// H 129..256 at sixteen) and the public launch_lstm_* launchers.  The
// one-segment VALU forms are lstm_valu.hip (built with -fno-slp-vectorize).
#include "smi_device.hpp"
#include "smi_internal.hpp"
#include "lstm_cell.hpp"

namespace smi {

constexpr int LR = 16;   // segments per workgroup
#ifdef SMI_PROF
__device__ unsigned long long g_lstm_ticks[8];   // this unit's phase ticks (LSTM_TICK, lstm_cell.hpp)
#endif

// LDS leading dim for a [16][K] A-operand image: >= round4(K) and == 4 (mod 8),
// so the 16 rows x 4 k of one MFMA operand read hit 64 distinct banks.
__host__ __device__ inline int lstm_ld(int k) {
  int l = round4(k);
  if ((l & 7) != 4) l += 4;
  return l;
}

// Activations (sigm, ftanh): lstm_cell.hpp.
// a quarter of K rounded up to a multiple of 4: 4 * lstm_q(H) is the padded
// row length of lstm_fwd_kernel's h_{t-1} image in LDS (lstm_fwd_lds)
__host__ __device__ inline int lstm_q(int K) { return (((K + 3) >> 2) + 3) & ~3; }

// H 129..256 (the r4 forms take H <= 128): 9..16 unit tiles of 16 over the 4
// waves, MAXUT tiles per wave
constexpr int MAXUT = 4;
__global__ void __launch_bounds__(kWG)
lstm_fwd_kernel(LstmFwdArgs a) {
  if (a.skip && a.skip[0] != 0) return;
  const int keepS = a.keep > 0 ? a.keep : a.S;     // steps whose c / gates are stored
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int H = a.H, B = a.B, G4 = 4 * H;
  const int LDH = lstm_ld(4 * lstm_q(H));
  float* hA[2] = {sm, sm + LR * LDH};
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int r0 = blockIdx.x * LR;
  const int NUT = (H + 15) >> 4;
  const int64_t BH = (int64_t)B * H;
  for (int e = threadIdx.x; e < LR * LDH; e += kWG) {
    const int r = e / LDH, k = e - r * LDH;
    const bool ok = k < H && r0 + r < B;
    const float v = ok ? a.h0[(int64_t)(r0 + r) * H + k] : 0.f;
    hA[0][e] = v;
    hA[1][e] = 0.f;
    if (ok) a.hbuf[(int64_t)(r0 + r) * H + k] = v;        // hbuf[0] = h0
  }
  float creg[MAXUT][4];
#pragma unroll
  for (int u = 0; u < MAXUT; ++u) {
    const int unit = (wave + 4 * u) * 16 + li;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int gr = r0 + lk * 4 + i;
      const bool ok = unit < H && gr < B;
      creg[u][i] = ok ? a.c0[(int64_t)gr * H + unit] : 0.f;
      if (ok && a.cbuf) a.cbuf[(int64_t)gr * H + unit] = creg[u][i];
    }
  }
  // per-lane W_hh row bases (clamped: rows of units >= H read unit H-1 and are
  // never stored)
  const float* wrow[MAXUT][4];
  float bh[MAXUT][4];
#pragma unroll
  for (int u = 0; u < MAXUT; ++u) {
    int unit = (wave + 4 * u) * 16 + li;
    unit = unit < H ? unit : H - 1;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      wrow[u][g] = a.w_hh + (int64_t)(g * H + unit) * H;
      bh[u][g] = a.b_hh[g * H + unit];
    }
  }
  const int nks = (H + 3) >> 2;        // k-steps of 4
  __syncthreads();
  for (int t = 0; t < a.S; ++t) {
    const float* hp = hA[t & 1];
    float* hn = hA[(t + 1) & 1];
    // x-projection of this step (epilogue operand), issued before the MFMAs
    float xp[MAXUT][4][4];
#pragma unroll
    for (int u = 0; u < MAXUT; ++u) {
      int unit = (wave + 4 * u) * 16 + li;
      unit = unit < H ? unit : H - 1;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int gr = r0 + lk * 4 + i;
        gr = gr < B ? gr : B - 1;
        const float* xr = a.xproj + ((int64_t)t * B + gr) * G4 + unit;
#pragma unroll
        for (int g = 0; g < 4; ++g) xp[u][g][i] = xr[g * H];
      }
    }
    f32x4 acc[MAXUT][4];
#pragma unroll
    for (int u = 0; u < MAXUT; ++u)
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[u][g] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* ap = hp + li * LDH + lk;
    int ks = 0;
    for (; ks + 4 <= nks; ks += 4) {
      float av[4], bv[MAXUT][4][4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = (ks + s) * 4 + lk;
        const int kc = k < H ? k : H - 1;         // A is zero there (LDS pad)
        av[s] = ap[(ks + s) * 4];
#pragma unroll
        for (int u = 0; u < MAXUT; ++u)
#pragma unroll
          for (int g = 0; g < 4; ++g) bv[u][g][s] = wrow[u][g][kc];
      }
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int u = 0; u < MAXUT; ++u)
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[u][g] = mfma4(av[s], bv[u][g][s], acc[u][g]);
    }
    for (; ks < nks; ++ks) {
      const int k = ks * 4 + lk;
      const int kc = k < H ? k : H - 1;
      const float av = ap[ks * 4];
#pragma unroll
      for (int u = 0; u < MAXUT; ++u)
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[u][g] = mfma4(av, wrow[u][g][kc], acc[u][g]);
    }
    // cell update in the accumulator registers
#pragma unroll
    for (int u = 0; u < MAXUT; ++u) {
      const int ut = wave + 4 * u;
      const int unit = ut * 16 + li;
      if (ut >= NUT) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = lk * 4 + i, gr = r0 + row;
        const float gi = xp[u][0][i] + (acc[u][0][i] + bh[u][0]);
        const float gf = xp[u][1][i] + (acc[u][1][i] + bh[u][1]);
        const float gg = xp[u][2][i] + (acc[u][2][i] + bh[u][2]);
        const float go = xp[u][3][i] + (acc[u][3][i] + bh[u][3]);
        const float ig = sigm(gi), fg = sigm(gf), cg = ftanh(gg), og = sigm(go);
        const float c = fg * creg[u][i] + ig * cg;
        const float h = og * ftanh(c);
        const bool ok = unit < H && gr < B;
        creg[u][i] = ok ? c : 0.f;
        if (unit < H) hn[row * LDH + unit] = ok ? h : 0.f;
        if (ok) {
          a.hbuf[(int64_t)(t + 1) * BH + (int64_t)gr * H + unit] = h;
          if (a.cbuf && t < keepS) a.cbuf[(int64_t)(t + 1) * BH + (int64_t)gr * H + unit] = c;
          if (a.gates && t < keepS) {
            float* gp = a.gates + ((int64_t)t * B + gr) * G4 + unit;
            gp[0] = ig; gp[H] = fg; gp[2 * H] = cg; gp[3 * H] = og;
          }
        }
      }
    }
    __syncthreads();
  }
}



__global__ void __launch_bounds__(kWG)
lstm_bwd_kernel(LstmBwdArgs a) {
  if (a.skip && a.skip[0] != 0) return;
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int H = a.H, B = a.B, G4 = 4 * H;
  const int LDG = lstm_ld(G4);
  float* dG[2] = {sm, sm + LR * LDG};
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int r0 = blockIdx.x * LR;
  const int NUT = (H + 15) >> 4;
  const int64_t BH = (int64_t)B * H;
  for (int e = threadIdx.x; e < 2 * LR * LDG; e += kWG) sm[e] = 0.f;
  float dcreg[MAXUT][4];
  f32x4 dhrec[MAXUT];
#pragma unroll
  for (int u = 0; u < MAXUT; ++u) {
    dhrec[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) dcreg[u][i] = 0.f;
  }
  int ucl[MAXUT];
#pragma unroll
  for (int u = 0; u < MAXUT; ++u) {
    const int unit = (wave + 4 * u) * 16 + li;
    ucl[u] = unit < H ? unit : H - 1;
  }
  const int nks = G4 >> 2;              // K = 4H, k-steps of 4
  __syncthreads();
  for (int t = a.S - 1; t >= 0; --t) {
    float* dg = dG[t & 1];
#pragma unroll
    for (int u = 0; u < MAXUT; ++u) {
      const int ut = wave + 4 * u;
      const int unit = ut * 16 + li;
      if (ut >= NUT) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = lk * 4 + i;
        int gr = r0 + row;
        const bool ok = unit < H && gr < B;
        gr = gr < B ? gr : B - 1;
        const int uc = ucl[u];
        const float* gp = a.gates + ((int64_t)t * B + gr) * G4 + uc;
        const float ig = gp[0], fg = gp[H], cg = gp[2 * H], og = gp[3 * H];
        const float c = a.cbuf[(int64_t)(t + 1) * BH + (int64_t)gr * H + uc];
        const float cp = a.cbuf[(int64_t)t * BH + (int64_t)gr * H + uc];
        const float dh = a.dh[(int64_t)t * BH + (int64_t)gr * H + uc] + dhrec[u][i];
        const float tc = ftanh(c);
        const float dc = dh * og * (1.f - tc * tc) + dcreg[u][i];
        const float d_o = (dh * tc) * (og * (1.f - og));
        const float d_i = (dc * cg) * (ig * (1.f - ig));
        const float d_g = (dc * ig) * (1.f - cg * cg);
        const float d_f = (dc * cp) * (fg * (1.f - fg));
        dcreg[u][i] = ok ? dc * fg : 0.f;
        if (ok) {
          float* o = a.dgates + ((int64_t)t * B + gr) * G4 + unit;
          o[0] = d_i; o[H] = d_f; o[2 * H] = d_g; o[3 * H] = d_o;
          float* l = dg + row * LDG + unit;
          l[0] = d_i; l[H] = d_f; l[2 * H] = d_g; l[3 * H] = d_o;
        }
      }
    }
    __syncthreads();
    if (t == 0) break;
    // dh_rec for step t-1:  dgates_t (16 x 4H) @ W_hh (4H x H)
#pragma unroll
    for (int u = 0; u < MAXUT; ++u) dhrec[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* ap = dg + li * LDG + lk;
    int ks = 0;
    for (; ks + 8 <= nks; ks += 8) {
      float av[8], bv[MAXUT][8];
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const int k = (ks + s) * 4 + lk;
        av[s] = ap[(ks + s) * 4];
#pragma unroll
        for (int u = 0; u < MAXUT; ++u) bv[u][s] = a.w_hh[(int64_t)k * H + ucl[u]];
      }
#pragma unroll
      for (int s = 0; s < 8; ++s)
#pragma unroll
        for (int u = 0; u < MAXUT; ++u) dhrec[u] = mfma4(av[s], bv[u][s], dhrec[u]);
    }
    for (; ks < nks; ++ks) {
      const int k = ks * 4 + lk;
      const float av = ap[ks * 4];
#pragma unroll
      for (int u = 0; u < MAXUT; ++u) dhrec[u] = mfma4(av, a.w_hh[(int64_t)k * H + ucl[u]], dhrec[u]);
    }
  }
}

constexpr int kWG8 = 512;
// ---------------------------------------------------------------------------
// 4-segment variants (H <= 128, the reference default H = 100 included): a
// workgroup owns LR4 = 4 segments, so the 1024-segment C3 batch spreads over
// 256 workgroups — one per CU — instead of 64.  A step's recurrent GEMM is
// then 4 rows x 4H columns x H, which is exactly the shape of
// v_mfma_f32_4x4x1_16b_f32 with block 0's A operand (the 4 rows of h_{t-1},
// lanes 0-3) broadcast to all 16 blocks (cbsz 4): a 4 x 64 outer-product
// step whose output column is the lane.  Wave w owns gate columns
// 64w .. 64w+63 with its W_hh column in registers; 8 accumulators over
// k mod 8 hide the 44-cycle dependent latency (measured: 12 cycles/MFMA at 4
// chains, tools/exp/mfma4x4.hip).  The cell update runs one (row, unit) per
// thread after the pre-activations pass through LDS.
//
// Backward: dh_rec = dgates_t (4 x 4H) W_hh (4H x H) with units on lanes
// (ceil(H/64) groups of 64) and K = 4H split over the waves of a group; the
// partial sums meet in LDS and are added in a fixed order by the cell threads.
// dst[k] = r[k] for k < n, 0 for n <= k < N: float4 runs when r is 16-byte
// aligned and n % 4 == 0, float2 runs when 8-byte aligned and n even, else
// scalar loads (the branch is uniform across a launch's rows when the row
// stride keeps the alignment)
template <int N>
__device__ __forceinline__ void load_row(const float* r, int n, float* dst) {
  static_assert(N % 4 == 0, "rows in float4 runs");
  const uintptr_t ad = reinterpret_cast<uintptr_t>(r);
  if ((ad & 15) == 0 && (n & 3) == 0) {
#pragma unroll
    for (int k = 0; k < N; k += 4) {
      const float4 v = k < n ? *reinterpret_cast<const float4*>(r + k) : float4{0.f, 0.f, 0.f, 0.f};
      dst[k] = v.x; dst[k + 1] = v.y; dst[k + 2] = v.z; dst[k + 3] = v.w;
    }
  } else if ((ad & 7) == 0 && (n & 1) == 0) {
#pragma unroll
    for (int k = 0; k < N; k += 2) {
      const float2 v = k < n ? *reinterpret_cast<const float2*>(r + k) : float2{0.f, 0.f};
      dst[k] = v.x; dst[k + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int k = 0; k < N; ++k) dst[k] = k < n ? r[k] : 0.f;
  }
}

constexpr int LR4 = 4;
constexpr int LSTM_HQ = 4;    // h float4 LDS reads in flight (forward r4)

__device__ __forceinline__ f32x4 mfma4x64(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 4, 0, 0);
}

// KP: H rounded up to a multiple of 8 (W_hh registers per lane).  KX > 0:
// the input projection is fused (din <= KX, a multiple of 8): W_ih's column
// joins W_hh's in registers, x_t of the 4 segments is staged in LDS one step
// ahead, and the k loop runs over [x_t | h_{t-1}] — no xproj GEMM and no
// [S][B][4H] round trip through HBM.
// VF (round 6): the launcher checked that W_hh rows are float4 runs (H % 4 == 0,
// 16-byte aligned) and W_ih rows float2 runs (din even, 8-byte aligned), so the
// row loads take ONE vector width without a run-time branch -- load_row's
// uniform alignment branch made the waitcnt pass wait vmcnt(0) at its merge,
// serializing the W_hh and W_ih loads into separate memory round trips
// (n % V == 0: a run is wholly inside the row or wholly past it; runs past it
// read a zero vector by address -- a select on the loaded value would make
// the waitcnt pass wait for the load right there)
__device__ __attribute__((aligned(16))) float g_lstm_zero4[4] = {0.f, 0.f, 0.f, 0.f};
template <int N, int V>
__device__ __forceinline__ void load_row_v(const float* r, int n, float* dst) {
  static_assert(N % 4 == 0 && (V == 4 || V == 2), "vector rows");
#pragma unroll
  for (int k = 0; k < N; k += V) {
    const float* src = k < n ? r + k : g_lstm_zero4;
    if constexpr (V == 4) {
      const float4 v = *reinterpret_cast<const float4*>(src);
      dst[k] = v.x; dst[k + 1] = v.y; dst[k + 2] = v.z; dst[k + 3] = v.w;
    } else {
      const float2 v = *reinterpret_cast<const float2*>(src);
      dst[k] = v.x; dst[k + 1] = v.y;
    }
  }
}

// IMG: a.w_ih / a.w_hh point into the TRANSPOSED image [W_ihT [din][4H]
// | W_hhT [H][4H] | 4H zeros] (launch_lstm_weight_image, kept current by
// adam_split_kernel), so the lane's column is w[k] = T[k * 4H + col]: one dword
// per lane at consecutive addresses, the BPTT's access pattern, instead of 64
// rows' cache lines behind every load instruction.  No alignment or H % 4
// requirement; k >= n reads the image's zero row, a zero by address (zoff: its
// float offset from t; the row offset is a scalar select, no branch).  Same
// register values as the row loads, same MFMA order: bit-identical results.
template <int N>
__device__ __forceinline__ void load_col(const float* t, int n, int ld, uint32_t zoff, int col,
                                         float* dst) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const uint32_t row = k < n ? (uint32_t)(k * ld) : zoff;          // wave-uniform
    dst[k] = t[row + (uint32_t)col];
  }
}

template <int KP, int KX, bool VF = false, bool IMG = false>
__global__ void __launch_bounds__(kWG8)
lstm_fwd_r4_kernel(LstmFwdArgs a) {
  if (a.skip && a.skip[0] != 0) return;
  LSTM_T0();
  const int keepS = a.keep > 0 ? a.keep : a.S;     // steps whose c / gates are stored
  constexpr int KXS = KX > 0 ? KX : 8;
  __shared__ __attribute__((aligned(16))) float hS[2][LR4 * KP];
  __shared__ __attribute__((aligned(16))) float xS[2][LR4 * KXS];
  __shared__ float pre[LR4][4 * KP];
  const int H = a.H, B = a.B, G4 = 4 * H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.x * LR4;
  const int64_t BH = (int64_t)B * H;
  const int col = wave * 64 + lane;
  const bool cact = wave * 64 < G4;              // wave-uniform
  const int colc = col < G4 ? col : G4 - 1;
  float w[KP];
  float wx[KXS];
  float bh = a.b_hh[colc];
  if constexpr (KX > 0) bh += a.b_ih[colc];
  // the lane's W_hh (and W_ih) row in registers, loaded in 16- (8-) byte runs
  // where the rows allow (a load per k put 64 rows' lines behind every
  // instruction, 32 instructions per line)
  if constexpr (IMG) {
    load_col<KP>(a.w_hh, H, G4, (uint32_t)(H * G4), colc, w);
    if constexpr (KX > 0) load_col<KX>(a.w_ih, a.din, G4, (uint32_t)((a.din + H) * G4), colc, wx);
  } else if constexpr (VF) {
    load_row_v<KP, 4>(a.w_hh + (int64_t)colc * H, H, w);
    if constexpr (KX > 0) load_row_v<KX, 2>(a.w_ih + (int64_t)colc * a.din, a.din, wx);
  } else {
    load_row<KP>(a.w_hh + (int64_t)colc * H, H, w);
    if constexpr (KX > 0) load_row<KX>(a.w_ih + (int64_t)colc * a.din, a.din, wx);
  }
  // x staging: thread tid < 4*KX owns (row tid / KX, k tid % KX) of x_t
  const int xr = tid / KXS, xk = tid - (tid / KXS) * KXS;
  const bool xown = KX > 0 && tid < LR4 * KXS;
  const int64_t xoff0 = (int64_t)min(r0 + xr, B - 1) * a.ldx + min(xk, a.din - 1);
  const bool xval = xk < a.din;
  // the raw value (clamped address): the zero for k >= din is selected when it
  // is written to LDS a step later, so the load stays in flight across the
  // step (a select right after the load made the compiler wait vmcnt(0) on it
  // in every step, the x fetch latency on the recurrence's critical path)
  auto xload = [&](int t) -> float { return a.x[(int64_t)t * B * a.ldx + xoff0]; };
  // Round 6: x_0, x_1, c0 and h0 are loaded unconditionally (clamped
  // addresses, the selects after the loads) together with the weights above
  // and stored after; a load used only under a per-lane condition (xown, ok)
  // was sunk into that branch and waited on there, one round trip each
  float xnext = 0.f, x0 = 0.f;
  if constexpr (KX > 0) {
    x0 = xload(0);
    xnext = xload(a.S > 1 ? 1 : 0);
  }
  // cell owned by this thread: (crow, cunit)
  const bool cell = tid < LR4 * H;
  const int crow = cell ? tid / H : 0;
  const int cunit = cell ? tid - crow * H : 0;
  const int cgr = r0 + crow;
  const bool cok = cell && cgr < B;
  const float c0v = a.c0[(int64_t)min(cgr, B - 1) * H + cunit];
  static_assert(LR4 * KP <= kWG8, "one h0 slot per thread");
  const int he = min(tid, LR4 * KP - 1);
  const int hr = he / KP, hk = he - hr * KP;
  float h0v = a.h0[(int64_t)min(r0 + hr, B - 1) * H + min(hk, H - 1)];
  // (pinned: their only uses sit under per-lane conditions)
  asm volatile("" : "+v"(h0v));
  if constexpr (KX > 0) asm volatile("" : "+v"(x0));
  if constexpr (KX > 0) {
    if (xown && a.S > 0) xS[0][xr * KXS + xk] = xval ? x0 : 0.f;
  }
  float creg = cok ? c0v : 0.f;
  if (cok && a.cbuf) a.cbuf[(int64_t)cgr * H + cunit] = creg;
  if (tid < LR4 * KP) {
    const bool ok = hk < H && r0 + hr < B;
    const float v = ok ? h0v : 0.f;
    hS[0][he] = v;
    hS[1][he] = 0.f;
    if (ok) a.hbuf[(int64_t)(r0 + hr) * H + hk] = v;       // hbuf[0] = h0
  }
  int64_t xoff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gr = r0 + i < B ? r0 + i : B - 1;
    xoff[i] = (int64_t)gr * G4 + colc;
  }
  float xp[4] = {0.f, 0.f, 0.f, 0.f};
  if (KX == 0 && a.S > 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) xp[i] = a.xproj[xoff[i]];
  }
  __syncthreads();
  LSTM_TICK(6);                                  // prologue (weights, x_0, c0 / h0)
  // x_t W_ih^T does not depend on h_{t-1}: its MFMAs for step t+1 are issued
  // right after step t's pre-activations are published, so the matrix pipe
  // works through them while the same waves run the cell update (VALU /
  // transcendentals / stores).  Same chains, same k order as issuing them at
  // the top of step t+1: bit-identical results.
  f32x4 acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto x_part = [&](int tt) {
    if constexpr (KX > 0) {
      // the same LDS read ring as the h part below: the wave issues these
      // MFMAs ahead of its cell update, so LDS round trips here delay the cell
      const float4* xr4 = reinterpret_cast<const float4*>(xS[tt & 1] + (lane & 3) * KXS);
      constexpr int NQX = KX / 4;
      float4 q[LSTM_HQ];
#pragma unroll
      for (int j = 0; j < LSTM_HQ && j < NQX; ++j) q[j] = xr4[j];
#pragma unroll
      for (int j = 0; j < NQX; ++j) {
        const float4 u = q[j % LSTM_HQ];
        const int ab = (j & 1) * 4;
        acc[ab + 0] = mfma4x64(u.x, wx[4 * j + 0], acc[ab + 0]);
        acc[ab + 1] = mfma4x64(u.y, wx[4 * j + 1], acc[ab + 1]);
        acc[ab + 2] = mfma4x64(u.z, wx[4 * j + 2], acc[ab + 2]);
        acc[ab + 3] = mfma4x64(u.w, wx[4 * j + 3], acc[ab + 3]);
        if (j + LSTM_HQ < NQX) q[j % LSTM_HQ] = xr4[j + LSTM_HQ];
      }
      __builtin_amdgcn_sched_group_barrier(0x100, LSTM_HQ < NQX ? LSTM_HQ : NQX, 0);
#pragma unroll
      for (int j = 0; j < NQX; ++j) {
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        if (j + LSTM_HQ < NQX) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
    }
  };
  if (cact && a.S > 0) x_part(0);
  for (int t = 0; t < a.S; ++t) {
    const float* hp = hS[t & 1];
    float* hn = hS[(t + 1) & 1];
    if (cact) {
      const float4* hr = reinterpret_cast<const float4*>(hp + (lane & 3) * KP);
      // h_{t-1} through a ring of LSTM_HQ float4 LDS reads in flight (the
      // compiler's own schedule kept one read ahead, so every 4 MFMAs (32
      // cycles) waited out an LDS round trip); the same MFMAs per accumulator
      // in the same k order: float4 j feeds acc[4 (j & 1) .. + 3]
      constexpr int NQ = KP / 4;
      float4 q[LSTM_HQ];
#pragma unroll
      for (int j = 0; j < LSTM_HQ; ++j) q[j] = hr[j];
#pragma unroll
      for (int j = 0; j < NQ; ++j) {
        const float4 u = q[j % LSTM_HQ];
        const int ab = (j & 1) * 4;
        acc[ab + 0] = mfma4x64(u.x, w[4 * j + 0], acc[ab + 0]);
        acc[ab + 1] = mfma4x64(u.y, w[4 * j + 1], acc[ab + 1]);
        acc[ab + 2] = mfma4x64(u.z, w[4 * j + 2], acc[ab + 2]);
        acc[ab + 3] = mfma4x64(u.w, w[4 * j + 3], acc[ab + 3]);
        if (j + LSTM_HQ < NQ) q[j % LSTM_HQ] = hr[j + LSTM_HQ];
      }
      // pin that schedule (left alone, the scheduler shrinks the ring back to
      // one read for register pressure): the ring's first reads, then per
      // float4 its 4 MFMAs and the read that refills its slot
      __builtin_amdgcn_sched_group_barrier(0x100, LSTM_HQ, 0);
#pragma unroll
      for (int j = 0; j < NQ; ++j) {
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        if (j + LSTM_HQ < NQ) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      const f32x4 sum = ((acc[0] + acc[1]) + (acc[2] + acc[3])) +
                        ((acc[4] + acc[5]) + (acc[6] + acc[7]));
      if (col < G4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) pre[i][col] = xp[i] + (sum[i] + bh);
      }
      if (KX == 0 && t + 1 < a.S) {
#pragma unroll
        for (int i = 0; i < 4; ++i) xp[i] = a.xproj[(int64_t)(t + 1) * B * G4 + xoff[i]];
      }
    }
    if constexpr (KX > 0) {   // x_{t+1} into the other buffer, x_{t+2} in flight
      if (xown && t + 1 < a.S) xS[(t + 1) & 1][xr * KXS + xk] = xval ? xnext : 0.f;
      if (xown && t + 2 < a.S) xnext = xload(t + 2);
    }
    LSTM_TICK(0);
    __syncthreads();
    if (cact) {               // next step's chains: x_{t+1} part now (see above)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (t + 1 < a.S) x_part(t + 1);
    }
    if (cell) {
      const float ig = sigm(pre[crow][cunit]), fg = sigm(pre[crow][H + cunit]);
      const float cg = ftanh(pre[crow][2 * H + cunit]), og = sigm(pre[crow][3 * H + cunit]);
      const float c = fg * creg + ig * cg;
      const float h = og * ftanh(c);
      creg = cok ? c : 0.f;
      hn[crow * KP + cunit] = cok ? h : 0.f;
      if (cok) {
        a.hbuf[(int64_t)(t + 1) * BH + (int64_t)cgr * H + cunit] = h;
        if (a.cbuf && t < keepS) a.cbuf[(int64_t)(t + 1) * BH + (int64_t)cgr * H + cunit] = c;
        if (a.gates && t < keepS) {
          float* gp = a.gates + ((int64_t)t * B + cgr) * G4 + cunit;
          gp[0] = ig; gp[H] = fg; gp[2 * H] = cg; gp[3 * H] = og;
        }
      }
    }
    LSTM_TICK(1);
    __syncthreads();
    LSTM_TICK(2);
  }
}

// One cell's BPTT step inputs (activated gates, c_t, c_{t-1}, dL/dh_t from the
// heads) and the factors of the cell backward that depend on the stored gates
// and c_t alone.  Written as one expression per gate, the cell backward
// compiled 1 - tc^2 and 1 - cg^2 into FMAs and dc into fma(1 - tc^2, dh og,
// dc_{t+1}); every other product and difference was a rounding of its own
// (the VALU forms still are that code).  Both helpers state exactly those
// operations with contraction off, so that computing the factors a phase
// early (lstm_bwd_r4_kernel) cannot change a rounding.
struct BpttIn { float ig, fg, cg, og, c, cp, dh; };
struct BpttFac { float tc, omt, fo, fi, fgg, ff; };

__device__ __forceinline__ BpttFac bptt_factors(const BpttIn& s) {
#pragma clang fp contract(off)
  BpttFac f;
  f.tc = ftanh(s.c);
  f.omt = fmaf(-f.tc, f.tc, 1.f);
  f.fo = s.og * (1.f - s.og);
  f.fi = s.ig * (1.f - s.ig);
  f.fgg = fmaf(-s.cg, s.cg, 1.f);
  f.ff = s.fg * (1.f - s.fg);
  return f;
}

// d = (d_i, d_f, d_g, d_o) and dc_t fg (the caller masks it) from dh_rec
__device__ __forceinline__ float bptt_cell(const BpttIn& s, const BpttFac& f, float dhr, float dcreg,
                                           float d[4]) {
#pragma clang fp contract(off)
  const float dh = s.dh + dhr;
  const float dc = fmaf(dh * s.og, f.omt, dcreg);
  d[3] = (dh * f.tc) * f.fo;
  d[0] = (dc * s.cg) * f.fi;
  d[2] = (dc * s.ig) * f.fgg;
  d[1] = (dc * s.cp) * f.ff;
  return dc * s.fg;
}

// KW: k range per wave (4H / waves-per-unit-group) rounded up to 8.  The
// launcher picks KW = 32 exactly when H <= 64 (one unit group, 8 waves over K)
// and 104 / 128 beyond (two groups, 4 waves each), so KW fixes the split.
//
// What sits between a step's two barriers on the cell threads is one LDS trip
// for the WPG partial sums, dh = dh_t + dh_rec, six dependent multiplies and
// the four LDS writes.  Everything else rides in the MFMA phase's shadow: the
// dgates stores of step t, the loads of step t-2 (two register sets, sa / sb,
// alternated by step parity in a loop unrolled by two, so every loaded
// register has one role for its whole life) and, after the wave's MFMAs are
// issued, the gate-only factors of step t-1.  The loads are issued by
// every thread from clamped addresses and consumed (pinned) by every thread a
// whole step later: with no branch around either, the one vmcnt wait of the
// loop is a counted one.  (The earlier form fetched t-1 under if (cell) / if (t > 0)
// after the cell's stores and waited for it before the first barrier.)
__device__ float g_lstm_zero_row[128];            // a W_hh row of zeros (H <= 128)
// (KW = 32 keeps two workgroups per CU, 128 registers, as before)
template <int KW>
__global__ void __launch_bounds__(kWG8, KW <= 32 ? 4 : 2)
lstm_bwd_r4_kernel(LstmBwdArgs a) {
  if (a.skip && a.skip[0] != 0) return;
  LSTM_T0();
  constexpr int G4P = 4 * 128 + KW;               // dG row stride (reads run up to KW past 4H)
  constexpr int WPG = KW <= 32 ? 8 : 4;           // waves per unit group of 64 lanes
  __shared__ __attribute__((aligned(16))) float dG[LR4 * G4P];
  __shared__ float red[8][LR4][64];
  const int H = a.H, B = a.B, G4 = 4 * H;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // in scalar registers
  const int r0 = blockIdx.x * LR4;
  const int64_t BH = (int64_t)B * H, BG4 = (int64_t)B * G4;
  const int kw = (G4 + WPG - 1) / WPG;
  const int ug = wave / WPG, kp = wave - ug * WPG;
  const int k0 = kp * kw;
  const int unit = ug * 64 + lane;
  const int uc = unit < H ? unit : H - 1;
  for (int e = tid; e < LR4 * G4P; e += kWG8) dG[e] = 0.f;
  // zero partial sums: the first step's dh_rec is 0 + 0 + .. = +0 without a branch
  for (int e = tid; e < 8 * LR4 * 64; e += kWG8) (&red[0][0][0])[e] = 0.f;
  const bool cell = tid < LR4 * H;
  const int crow = cell ? tid / H : 0;
  const int cunit = cell ? tid - crow * H : 0;
  const int cgr = r0 + crow;
  const bool cok = cell && cgr < B;
  const int64_t grc = cgr < B ? cgr : B - 1;
  const int cug = cunit >> 6, cl = cunit & 63;
  const int64_t goff = grc * G4 + cunit, hoff = grc * H + cunit;
  auto fetch = [&](int t, BpttIn& s) {
    const float* gp = a.gates + ((int64_t)t * BG4 + goff);
    s.ig = gp[0]; s.fg = gp[H]; s.cg = gp[2 * H]; s.og = gp[3 * H];
    const int64_t o = (int64_t)t * BH + hoff;
    s.c = a.cbuf[o + BH];
    s.cp = a.cbuf[o];
    s.dh = a.dh[o];
  };
  BpttIn sa, sb;                                  // steps S-1, S-3, .. / S-2, S-4, ..
  fetch(a.S - 1, sa);
  fetch(a.S > 1 ? a.S - 2 : 0, sb);
  // W_hh[k0 + j][unit] in registers.  Rows past the wave's k range are zeros by
  // address, as in load_col: a select on the loaded value is free to sink
  // below the barrier, where the KW wave-uniform conditions it left behind
  // spilled.  Lanes of units >= H hold unit H-1's column: their sums land in
  // red[][][lane >= H], which no cell reads (the earlier form zeroed them).
  float w[KW];
  const int jn = min(kw, G4 - k0);                  // the wave's rows: k0 + j, j < jn
#pragma unroll
  for (int j = 0; j < KW; ++j) {
    const bool in = j < jn;                           // wave-uniform
    const float* base = in ? a.w_hh : g_lstm_zero_row;
    const uint32_t ro = in ? (uint32_t)((k0 + j) * H) : 0u;
    w[j] = base[ro + (uint32_t)uc];
  }
  // (pinned here as in the loop: the loop's waits are then counted from the
  // loop's own loads on both ways into it)
  asm volatile("" : "+v"(sa.ig), "+v"(sa.fg), "+v"(sa.cg), "+v"(sa.og), "+v"(sa.c), "+v"(sa.cp),
               "+v"(sa.dh));
  asm volatile("" : "+v"(sb.ig), "+v"(sb.fg), "+v"(sb.cg), "+v"(sb.og), "+v"(sb.c), "+v"(sb.cp),
               "+v"(sb.dh));
  BpttFac f = bptt_factors(sa);
  float dcreg = 0.f;
  // the weights land here (vmcnt(0); nothing selects on them, so their waits
  // would otherwise sit at their first MFMAs, inside the loop)
  __builtin_amdgcn_s_waitcnt(0x0F70);
  __syncthreads();
  LSTM_TICK(7);                                  // prologue (W_hh, first steps' inputs)
  // cell phase of step t from its inputs x, up to the barrier: d = its dgates
  auto cells = [&](const BpttIn& x, float d[4]) __attribute__((always_inline)) {
    if (cell) {
      // the partial sums in one LDS round trip, added in the order p = 0, 1, ..
      float r[WPG];
#pragma unroll
      for (int p = 0; p < WPG; ++p) r[p] = red[cug * WPG + p][crow][cl];
      float dhr = 0.f;
#pragma unroll
      for (int p = 0; p < WPG; ++p) dhr += r[p];
      const float dcf = bptt_cell(x, f, dhr, dcreg, d);
      dcreg = cok ? dcf : 0.f;
      float* l = dG + crow * G4P + cunit;
      l[0] = cok ? d[0] : 0.f; l[H] = cok ? d[1] : 0.f;
      l[2 * H] = cok ? d[2] : 0.f; l[3 * H] = cok ? d[3] : 0.f;
    }
    LSTM_TICK(3);
    __syncthreads();
    LSTM_TICK(4);
  };
  auto store = [&](int t, const float d[4]) __attribute__((always_inline)) {
    if (cok) {
      float* o = a.dgates + ((int64_t)t * BG4 + (int64_t)cgr * G4 + cunit);
      o[0] = d[0]; o[H] = d[1]; o[2 * H] = d[2]; o[3 * H] = d[3];
    }
  };
  // a step t > 0: x holds its inputs, y those of step t-1 (in flight)
  auto step = [&](int t, BpttIn& x, BpttIn& y) __attribute__((always_inline)) {
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    cells(x, d);
    f32x4 acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // dgates operand reads LQ float4 ahead (as in the forward's h loop)
    constexpr int NQ = KW / 4, LQ = 4;
    const float4* dr = reinterpret_cast<const float4*>(dG + (lane & 3) * G4P + k0);
    float4 q[LQ];
#pragma unroll
    for (int j = 0; j < LQ && j < NQ; ++j) q[j] = dr[j];
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      const float4 u = q[j % LQ];
      if (j + LQ < NQ) q[j % LQ] = dr[j + LQ];
      const int a0 = (j & 1) * 4;
      acc[a0 + 0] = mfma4x64(u.x, w[4 * j + 0], acc[a0 + 0]);
      acc[a0 + 1] = mfma4x64(u.y, w[4 * j + 1], acc[a0 + 1]);
      acc[a0 + 2] = mfma4x64(u.z, w[4 * j + 2], acc[a0 + 2]);
      acc[a0 + 3] = mfma4x64(u.w, w[4 * j + 3], acc[a0 + 3]);
      // once the matrix pipe has work: step t's dgates stores, and step t-2's
      // inputs into x, whose values of step t are spent
      if (j == 1) {
        store(t, d);
        fetch(t > 1 ? t - 2 : 0, x);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // step t-1's inputs, loaded a step ago: the loop's one (counted) vmcnt wait,
    // here for all seven, so that the cell phase meets none
    asm volatile("" : "+v"(y.ig), "+v"(y.fg), "+v"(y.cg), "+v"(y.og), "+v"(y.c), "+v"(y.cp),
                 "+v"(y.dh));
    // under the MFMAs just issued (pinned: their one use is in the next cell
    // phase, where the compiler would otherwise compute them)
    f = bptt_factors(y);
    asm volatile("" : "+v"(f.tc), "+v"(f.omt), "+v"(f.fo), "+v"(f.fi), "+v"(f.fgg), "+v"(f.ff));
    const f32x4 sum = ((acc[0] + acc[1]) + (acc[2] + acc[3])) +
                      ((acc[4] + acc[5]) + (acc[6] + acc[7]));
#pragma unroll
    for (int i = 0; i < 4; ++i) red[wave][i][lane] = sum[i];
    LSTM_TICK(5);
    __syncthreads();
  };
  // steps S-1 .. 1 in pairs (one way out of the loop: a second one led back to
  // the loop head in the structured flow and, with x's loads in flight on it,
  // turned the cell phase's waits into vmcnt(0)), then the odd one and step 0
  int t = a.S - 1;
  for (int i = t >> 1; i > 0; --i, t -= 2) {
    step(t, sa, sb);
    step(t - 1, sb, sa);
  }
  float d[4] = {0.f, 0.f, 0.f, 0.f};
  if (t == 1) {
    step(1, sa, sb);
    cells(sb, d);
  } else {
    cells(sa, d);
  }
  store(0, d);
}

static int device_cus() {
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
      cus = 256;
  }
  return cus;
}
// the VALU forms (one segment per workgroup) when every segment gets a CU of
// its own; at two or more segments per CU the r4 MFMA form (384 / 512
// segments: 4.32 / 4.98 ms per learn against 4.76 / 5.44 with two segments per
// workgroup and 4.42 / 5.12 with the q form at two workgroups per CU, round 6,
// profiles/r06/ab/lstm_form_*)
static bool lstm_valu(int B, int H) { return H >= 1 && H <= 128 && B <= device_cus(); }
// the r4 forward's image form (IMG) runs for (B, H): wherever the r4 form does
bool lstm_fwd_image_ok(int B, int H) { return H >= 1 && H <= 128 && B >= 1 && !lstm_valu(B, H); }

// image = [W_ihT [din][4H] | W_hhT [H][4H] | 4H zeros] from the natural rows,
// one output element per thread (coalesced stores; the strided reads are one
// per thread)
__global__ void __launch_bounds__(kWG)
lstm_weight_image_kernel(const float* __restrict__ w_ih, const float* __restrict__ w_hh, int din,
                         int H, float* __restrict__ image) {
  const int G4 = 4 * H, nih = G4 * din, nw = nih + G4 * H;
  const int o = blockIdx.x * kWG + threadIdx.x;
  if (o >= nw + G4) return;
  if (o < nih) {
    const int k = o / G4, col = o - k * G4;
    image[o] = w_ih[col * din + k];
  } else if (o < nw) {
    const int k = (o - nih) / G4, col = (o - nih) - k * G4;
    image[o] = w_hh[col * H + k];
  } else {
    image[o] = 0.f;                 // the zero row the forward's padding k read
  }
}

int launch_lstm_weight_image(const float* w_ih, const float* w_hh, int din, int H, float* image,
                             hipStream_t st) {
  if (H < 1 || H > 128 || din < 1 || din > 4096)
    return set_error(SMI_E_ARG, "lstm_weight_image: H must be in [1, 128], din in [1, 4096]");
  const int n = 4 * H * (din + H + 1);
  hipLaunchKernelGGL(lstm_weight_image_kernel, dim3((n + kWG - 1) / kWG), dim3(kWG), 0, st, w_ih,
                     w_hh, din, H, image);
  return check_launch("lstm_weight_image_kernel");
}

#ifdef SMI_PROF
extern "C" int smi_lstm_phase_ticks(unsigned long long* out /* [8] */) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lstm_ticks), sizeof(g_lstm_ticks)) != hipSuccess)
    return SMI_E_LAUNCH;
  static const unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_lstm_ticks), zero, sizeof(zero)) == hipSuccess ? SMI_OK
                                                                                        : SMI_E_LAUNCH;
}
#endif

int64_t lstm_fwd_lds(int H) { return (int64_t)2 * LR * lstm_ld(4 * lstm_q(H)) * 4; }
int64_t lstm_bwd_lds(int H) { return (int64_t)2 * LR * lstm_ld(4 * H) * 4; }

// the r4 forward's fixed-width row loads (VF): W_hh float4 runs, W_ih float2
// runs (else: the alignment-branching loads)
static bool r4_vf(const LstmFwdArgs& a, bool fused_x) {
  auto al = [](const void* p, uintptr_t m) { return (reinterpret_cast<uintptr_t>(p) & m) == 0; };
  if (a.H % 4 != 0 || !al(a.w_hh, 15)) return false;
  return !fused_x || (a.din % 2 == 0 && a.din >= 2 && al(a.w_ih, 7));
}

int launch_lstm_fwd(const float* xproj, const float* w_hh, const float* b_hh, const float* h0,
                    const float* c0, int S, int B, int H, float* hbuf, float* cbuf, float* gates,
                    hipStream_t st, const int* skip, int keep, bool image) {
  if (B <= 0 || S < 0) return SMI_OK;
  if (H < 1 || H > 256) return set_error(SMI_E_ARG, "lstm: hidden size must be in [1, 256]");
  if (image && !lstm_fwd_image_ok(B, H)) return SMI_E_NOFIT;    // w_hh is W_hhT: the r4 form only
  LstmFwdArgs a{xproj, w_hh, b_hh, h0, c0, S, B, H, hbuf, cbuf, gates, skip};
  a.keep = keep;
  const int kslot = ktime_begin(st);
  // algorithmic flops: the recurrent GEMM h W_hh^T of every step
  struct End { int s; hipStream_t st; double f;
               ~End() { ktime_end(s, KT_LSTM_FWD, f, st); } } end_{kslot, st, 8.0 * B * H * (double)H * S};
  if (lstm_valu(B, H)) return check_launch(lstm_v_fwd(a, 0, st));
  if (H <= 128) {
    const dim3 g4((B + LR4 - 1) / LR4);
    const bool vf = r4_vf(a, false);
#define SMI_R4F(KP_)                                                                        \
    do {                                                                                    \
      if (image) {                                                                          \
        hipLaunchKernelGGL((lstm_fwd_r4_kernel<KP_, 0, false, true>), g4, dim3(kWG8), 0,    \
                           st, a);                                                          \
        return check_launch("lstm_fwd_r4_kernel<" #KP_ ",0,img>");                          \
      } else if (vf) {                                                                      \
        hipLaunchKernelGGL((lstm_fwd_r4_kernel<KP_, 0, true>), g4, dim3(kWG8), 0, st, a);   \
        return check_launch("lstm_fwd_r4_kernel<" #KP_ ",0,vf>");                           \
      } else {                                                                              \
        hipLaunchKernelGGL((lstm_fwd_r4_kernel<KP_, 0>), g4, dim3(kWG8), 0, st, a);         \
        return check_launch("lstm_fwd_r4_kernel<" #KP_ ",0>");                              \
      }                                                                                     \
    } while (0)
    if (H <= 32) SMI_R4F(32);
    else if (H <= 64) SMI_R4F(64);
    else if (H <= 104) SMI_R4F(104);
    else SMI_R4F(128);
#undef SMI_R4F
  }
  const size_t lds = (size_t)lstm_fwd_lds(H);
  const dim3 grid((B + LR - 1) / LR);
  allow_lds(lstm_fwd_kernel, lds);
  hipLaunchKernelGGL(lstm_fwd_kernel, grid, dim3(kWG), lds, st, a);
  return check_launch("lstm_fwd_kernel<4>");
}

// LSTM forward with the input projection fused (din <= 64, H <= 104): returns
// SMI_E_NOFIT when the shape needs the xproj GEMM + launch_lstm_fwd instead
int launch_lstm_fwd_x(const float* x, int64_t ldx, int din, const float* w_ih, const float* b_ih,
                      const float* w_hh, const float* b_hh, const float* h0, const float* c0,
                      int S, int B, int H, float* hbuf, float* cbuf, float* gates,
                      hipStream_t st, const int* skip, int keep, bool image) {
  // no step, no launch (the outputs stay untouched): the fused forms' prologues
  // load x_0 unconditionally, and at S == 0 the K-split form clamps that index
  // to S * KX - 1 = -1
  if (B <= 0 || S <= 0) return SMI_OK;
  if (!lstm_fwd_x_fuses(din, H)) return SMI_E_NOFIT;
  const bool valu = lstm_valu(B, H);
  // w_ih / w_hh are W_ihT / W_hhT inside one image: the r4 form only (callers
  // ask lstm_fwd_image_ok first)
  if (image && valu) return SMI_E_NOFIT;
  if (image && w_hh != w_ih + (int64_t)4 * H * din)
    return set_error(SMI_E_ARG, "lstm: W_hhT must follow W_ihT in the weight image");
  if (valu && lstm_fwd_v_lds(S, din <= 48 ? 48 : 64, (4 * H + 63) & ~63) > kVxMax)
    return SMI_E_NOFIT;                            // staged x + x parts > the LDS budget
  LstmFwdArgs a{nullptr, w_hh, b_hh, h0, c0, S, B, H, hbuf, cbuf, gates, skip,
                x, ldx, din, w_ih, b_ih, keep};
  const int kslot = ktime_begin(st);
  struct End { int s; hipStream_t st; double f;
               ~End() { ktime_end(s, KT_LSTM_FWD, f, st); } } end_{
      kslot, st, 8.0 * B * H * (double)(H + din) * S};
  if (valu) return check_launch(lstm_v_fwd(a, din <= 48 ? 48 : 64, st));
  const dim3 g4((B + LR4 - 1) / LR4);
  const bool vf = r4_vf(a, true);
#define SMI_R4X(KP_, KX_)                                                                     \
  do {                                                                                        \
    if (image) {                                                                              \
      hipLaunchKernelGGL((lstm_fwd_r4_kernel<KP_, KX_, false, true>), g4, dim3(kWG8), 0, st,  \
                         a);                                                                  \
      return check_launch("lstm_fwd_r4_kernel<" #KP_ "," #KX_ ",img>");                       \
    } else if (vf) {                                                                          \
      hipLaunchKernelGGL((lstm_fwd_r4_kernel<KP_, KX_, true>), g4, dim3(kWG8), 0, st, a);     \
      return check_launch("lstm_fwd_r4_kernel<" #KP_ "," #KX_ ",vf>");                        \
    } else {                                                                                  \
      hipLaunchKernelGGL((lstm_fwd_r4_kernel<KP_, KX_>), g4, dim3(kWG8), 0, st, a);           \
      return check_launch("lstm_fwd_r4_kernel<" #KP_ "," #KX_ ">");                           \
    }                                                                                         \
  } while (0)
  if (din <= 48) {
    if (H <= 64) SMI_R4X(64, 48);
    else SMI_R4X(104, 48);
  } else {
    if (H <= 64) SMI_R4X(64, 64);
    else SMI_R4X(104, 64);
  }
#undef SMI_R4X
}

// BR of the BPTT's one-segment-per-workgroup K-split form (lstm_bwd_q_kernel)
// when launch_lstm_bwd would run it for (B, H), else 0: the form that the
// BPTT + weight-gradient launch (linear_dw.hip) embeds
int lstm_bwd_q_form(int B, int H, const float* w_hh) {
  if (!lstm_valu(B, H) || !lstm_bwd_q_ok(H, w_hh)) return 0;
  return H <= 64 ? 16 : H <= 100 ? 25 : 32;
}

// two independent fused-input forwards (same H and input width, e.g. the GAE
// critic pass and the reference policy's forward) in ONE launch at one segment
// per workgroup (the K-split form): SMI_E_NOFIT when that form does not run
// for B0 + B1 segments on this device or the widths differ
bool lstm_fwd_x_dual_fits(int B0, int B1, int S, int H, int din) {
  if (din < 1 || din > 64 || H < 1 || H > 104 || B0 <= 0 || B1 <= 0)
    return false;
  if (!lstm_valu(B0 + B1, H)) return false;
  return lstm_fwd_v_lds(S, din <= 48 ? 48 : 64, (4 * H + 63) & ~63) <= kVxMax;
}

int launch_lstm_fwd_x_dual(const LstmFwdArgs& a0, const LstmFwdArgs& a1, hipStream_t st) {
  const int H = a0.H, din = a0.din;
  const int smax = a0.S > a1.S ? a0.S : a1.S;
  // as launch_lstm_fwd_x: no step, no launch; one empty set of two has no form here
  if (a0.S <= 0 && a1.S <= 0) return SMI_OK;
  if (a0.S <= 0 || a1.S <= 0) return SMI_E_NOFIT;
  if (a0.H != a1.H || a0.din != a1.din || !lstm_fwd_x_dual_fits(a0.B, a1.B, smax, H, din))
    return SMI_E_NOFIT;
  const int kx = din <= 48 ? 48 : 64;
  const int kslot = ktime_begin(st);
  const char* form = lstm_q_fwd_dual(a0, a1, kx, st);
  ktime_end(kslot, KT_LSTM_FWD,
            8.0 * H * (double)(H + din) * ((double)a0.B * a0.S + (double)a1.B * a1.S), st);
  return check_launch(form);
}

int launch_lstm_bwd(const float* dh, const float* gates, const float* cbuf, const float* w_hh,
                    int S, int B, int H, float* dgates, hipStream_t st, const int* skip) {
  if (B <= 0 || S <= 0) return SMI_OK;
  if (H < 1 || H > 256) return set_error(SMI_E_ARG, "lstm: hidden size must be in [1, 256]");
  LstmBwdArgs a{dh, gates, cbuf, w_hh, S, B, H, dgates, skip};
  const int kslot = ktime_begin(st);
  struct End { int s; hipStream_t st; double f;
               ~End() { ktime_end(s, KT_LSTM_BWD, f, st); } } end_{kslot, st,
                                                                 8.0 * B * H * (double)H * (S - 1)};
  if (lstm_valu(B, H)) return check_launch(lstm_v_bwd(a, st));
  if (H <= 128) {
    const int nu = (H + 63) / 64, wpg = 8 / nu;
    const int kw = (4 * H + wpg - 1) / wpg;
    const dim3 g4((B + LR4 - 1) / LR4);
#define SMI_R4B(KW_)                                                              \
    do {                                                                          \
      hipLaunchKernelGGL(lstm_bwd_r4_kernel<KW_>, g4, dim3(kWG8), 0, st, a);      \
      return check_launch("lstm_bwd_r4_kernel<" #KW_ ">");                        \
    } while (0)
    // (kw is H / 2 <= 32 for H <= 64 and >= 65 beyond)
    if (kw <= 32) SMI_R4B(32);
    else if (kw <= 104) SMI_R4B(104);
    else SMI_R4B(128);
#undef SMI_R4B
  }
  const size_t lds = (size_t)lstm_bwd_lds(H);
  if (lds > 160 * 1024) return set_error(SMI_E_NOFIT, "lstm: hidden size too large for LDS");
  const dim3 grid((B + LR - 1) / LR);
  allow_lds(lstm_bwd_kernel, lds);
  hipLaunchKernelGGL(lstm_bwd_kernel, grid, dim3(kWG), lds, st, a);
  return check_launch("lstm_bwd_kernel<4>");
}


}  // namespace smi
