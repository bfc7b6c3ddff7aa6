// lstm_valu.hip — the LSTM recurrence at one segment per workgroup on the
// VALU (small local batches), built with -fno-slp-vectorize: its fmaf chains
// must stay scalar v_fmac_f32 (the SLP vectorizer packs them into v_pk_fma_f32
// + operand moves: same sums, slower); the flag on the MFMA forms changed their
// rounding, so they are a unit of their own (lstm_mfma.hip).
//
// VALU variants for small local batches (strong scaling: a rank of the N = 8
// C3 job holds 128 segments).  The MFMA forms (lstm_mfma.hip) waste the recurrence's
// matrix pipe at few segments per workgroup (v_mfma_f32_4x4x1 always computes
// 4 rows) and a step's latency does not fall with the batch.  Here a
// workgroup owns one segment and thread (u, q) = 4u + q owns ONE gate
// column g = q*H + u (gate q of hidden unit u) with its W_hh row (and, fused,
// its W_ih row) in registers:
//   pre_g   = x_t W_ih[g] + b_ih[g] + h_{t-1} W_hh[g] + b_hh[g]   (FMA chains,
//             h_{t-1} broadcast from LDS as 16-byte reads)
//   a_g     = sigmoid / tanh (gate g lives in lane 4u + q)
//   i,f,g,o of unit u gathered inside the lane quad with DPP quad broadcasts
//   c, h    computed redundantly by the quad's 4 lanes (identical values)
// so a step is one matvec, one quad exchange and ONE barrier (h_t published
// to LDS): the 128-segment batch fills 128 CUs.  The forward runs the K-split
// form below (lstm_fwd_q_kernel); this row form is the BPTT's fallback
// (lstm_bwd_v_kernel) where the K-split form's float4 loads do not apply.
// Backward: thread (u, q) holds column u of W_hh restricted to gate q's rows,
// dh_rec[u] = sum_q sum_j dgates[q*H + j] W_hh[q*H + j][u] is a per-lane
// partial over gate q plus a fixed-order quad sum.
#include "smi_device.hpp"
#include "smi_internal.hpp"
#include "lstm_cell.hpp"

namespace smi {

#ifdef SMI_PROF
__device__ unsigned long long g_lstm_ticks[8];   // this unit's phase ticks (LSTM_TICK, lstm_cell.hpp)
#endif

// s0..s3 += v[k] * w[k] over k < KP, v read from LDS as KP / 4 float4s in
// chunks of kVC, the next chunk's reads issued before the current chunk's FMAs
// (scalar FMAs: the same sums on v_pk_fma_f32, half the instructions, measured
// slower at 128 segments -- 1.70 / 1.61 us per forward / BPTT step against
// 1.62 / 1.50)
constexpr int kVC = 4;
template <int KP>
__device__ __forceinline__ void v_dot_pipelined(const float4* __restrict__ v, const float (&w)[KP],
                                                float& s0, float& s1, float& s2, float& s3) {
  constexpr int N4 = KP / 4, NC = (N4 + kVC - 1) / kVC;
  float4 buf[2][kVC];
  auto ld = [&](int c) {
#pragma unroll
    for (int i = 0; i < kVC; ++i)
      if (c * kVC + i < N4) buf[c & 1][i] = v[c * kVC + i];
  };
  ld(0);
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (c + 1 < NC) ld(c + 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < kVC; ++i) {
      const int k4 = c * kVC + i;
      if (k4 < N4) {
        const float4 hv = buf[c & 1][i];
        s0 = fmaf(hv.x, w[4 * k4], s0);
        s1 = fmaf(hv.y, w[4 * k4 + 1], s1);
        s2 = fmaf(hv.z, w[4 * k4 + 2], s2);
        s3 = fmaf(hv.w, w[4 * k4 + 3], s3);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <int KP>
__global__ void __launch_bounds__(kVT)
lstm_bwd_v_kernel(LstmBwdArgs a) {
  if (a.skip && a.skip[0] != 0) return;
  __shared__ __attribute__((aligned(16))) float dG[2][4 * KP];
  const int H = a.H, B = a.B, G4 = 4 * H;
  const int tid = threadIdx.x, u = tid >> 2, q = tid & 3;
  const bool act = u < H;
  const int uc = act ? u : H - 1;
  const int g = q * H + uc;
  const int64_t b = blockIdx.x;                  // one segment per workgroup (grid = B)
  const int64_t BH = (int64_t)B * H;
  for (int e = tid; e < 2 * 4 * KP; e += blockDim.x) (&dG[0][0])[e] = 0.f;
  float w[KP];                                   // W_hh[q*H + j][u]
#pragma unroll
  for (int j = 0; j < KP; ++j) {
    const float x = a.w_hh[(int64_t)(q * H + (j < H ? j : H - 1)) * H + uc];
    w[j] = j < H ? x : 0.f;
  }
  // per-step inputs, fetched two steps ahead into alternating register sets:
  // a step's loads are issued right after its dgates store and used two steps
  // later, so neither their latency nor the stores ahead of them (vmcnt counts
  // loads and stores in issue order) reach the critical path
  struct In { float gq, ct, ctm, dho; };
  In A, Bn;
  float dcreg = 0.f, dhr = 0.f;
  auto fetch = [&](int t, In& X) {               // t clamped by the caller: always issued
    X.gq = a.gates[((int64_t)t * B + b) * G4 + g];
    X.ct = a.cbuf[(int64_t)(t + 1) * BH + b * H + uc];
    X.ctm = a.cbuf[(int64_t)t * BH + b * H + uc];
    X.dho = a.dh[(int64_t)t * BH + b * H + uc];
  };
  if (a.S <= 0) return;
  fetch(a.S - 1, A);
  fetch(a.S >= 2 ? a.S - 2 : 0, Bn);
  __syncthreads();
  // one step; false after step 0
  auto step = [&](int t, In& X) -> bool {
    float* dgw = dG[t & 1];
    const float ig = quad_bcast<0>(X.gq), fg = quad_bcast<1>(X.gq);
    const float cg = quad_bcast<2>(X.gq), og = quad_bcast<3>(X.gq);
    const float dh = X.dho + dhr;
    const float tc = ftanh(X.ct);
    const float dc = dh * og * (1.f - tc * tc) + dcreg;
    const float d_o = (dh * tc) * (og * (1.f - og));
    const float d_i = (dc * cg) * (ig * (1.f - ig));
    const float d_g = (dc * ig) * (1.f - cg * cg);
    const float d_f = (dc * X.ctm) * (fg * (1.f - fg));
    dcreg = act ? dc * fg : 0.f;
    float dq = q == 0 ? d_i : q == 1 ? d_f : q == 2 ? d_g : d_o;
    dq = act ? dq : 0.f;
    if (act) {
      dgw[q * KP + u] = dq;
      a.dgates[((int64_t)t * B + b) * G4 + g] = dq;
    }
    fetch(t >= 2 ? t - 2 : 0, X);
    __syncthreads();
    if (t == 0) return false;
    const float4* dp = reinterpret_cast<const float4*>(dgw + q * KP);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    v_dot_pipelined<KP>(dp, w, s0, s1, s2, s3);
    const float p = (s0 + s1) + (s2 + s3);
    // fixed-order quad sum: every lane of the quad gets the same dh_rec
    dhr = (quad_bcast<0>(p) + quad_bcast<1>(p)) + (quad_bcast<2>(p) + quad_bcast<3>(p));
    return true;
  };
  for (int t = a.S - 1; t >= 0; t -= 2) {
    if (!step(t, A)) break;
    if (!step(t - 1, Bn)) break;
  }
}

// ---------------------------------------------------------------------------
// One segment per workgroup with the recurrent product's K split over the
// lane quad (round 5; a rank's share of a strong-scaled job).  The row
// form above gives thread (u, q) a whole W_hh row, so every
// thread reads all of h_{t-1} each step (26 ds_read_b128 per wave at H = 100:
// 728 LDS cycles per CU per step) and runs one 104-long FMA stream.  Here
// thread (u, q) = (tid >> 2, tid & 3) holds the FOUR gate rows j*H + u of
// unit u over its quarter k in [q*KQ, (q+1)*KQ) as (k, k+1) pairs:
//   forward  p_j = sum_k h_{t-1}[k] W_hh[j*H + u][k] on v_pk_fma_f32 (KQ/2
//            packed FMAs per gate over 2-float LDS reads: 13 ds_read_b64 per
//            wave), the four lanes' partials summed by two quad DPP adds
//            (l ^ 1, then l ^ 2: every lane of the quad ends with the same
//            four sums); lane q then finishes gate q exactly as the row forms
//            do (activation, quad broadcast, the cell computed alike in the
//            four lanes).  The x part is precomputed with the same K split of
//            W_ih over the staged x sequence (XQ > 0), or read from xproj
//            (XQ == 0) one step ahead.  W_hh is loaded while the x parts are
//            formed; the step's hbuf / cbuf / gates stores are issued after
//            the barrier, behind the next step's LDS reads.
//   BPTT     thread (ug, rr) = (tid >> 4, tid & 15) holds W_hh[r][4ug..4ug+3]
//            for the rows r in [rr*BR, rr*BR + BR) (BR = ceil(H / 4)), reads
//            those BR dgates of the step (a [16][BRP] padded LDS image: b128
//            reads, 64 distinct banks) and sums its four units on packed
//            FMAs; the 16 partials of a unit meet through four DPP adds
//            (quad l ^ 1, l ^ 2, row half-mirror, row rotate 8: identical
//            sums in all 16 lanes), and the cell backward keeps the (u, q)
//            mapping (unit u's sum sits in its own 16-lane row).
// Measured (tools/exp/lstm_v_exp.hip, 128 segments, H 100, one MI355X): see
// DESIGN.md §9.  Sums are fixed-order (deterministic); their association
// differs from the row forms' (fp32 rounding only).
// a1: a second, independent sequence set in the same launch (workgroups >=
// a0.B: the GAE critic pass and the reference policy's forward, two weight
// sets over two inputs); single launches pass a0 twice over a0.B workgroups
// A4 (the matrix-core x parts, XQ > 0 and XM): every lane finishes all four gates of its unit (after
// the two quad DPP adds each lane holds all four sums, and xP keeps unit u's
// four x parts at 4u .. 4u + 3): four independent activations instead of one
// followed by four quad broadcasts on the step's dependent chain (same ops on
// the same values: bit-identical)
template <int KQ, int XQ, bool XM, int WI>
__global__ void __launch_bounds__(kVT)
lstm_fwd_q_kernel(LstmFwdArgs a0, LstmFwdArgs a1) {
  constexpr bool A4 = XQ > 0 && XM;
  static_assert(WI != 2 || KQ % 4 == 0, "float4 k runs");
  const bool second = (int)blockIdx.x >= a0.B;
  const LstmFwdArgs& a = second ? a1 : a0;
  const int b = second ? (int)blockIdx.x - a0.B : (int)blockIdx.x;
  // the skip flag is read with the prologue's loads and tested before the
  // first global store (its own round trip in front of them cost ~1 us)
  const int skipv = a.skip ? a.skip[0] : 0;
  LSTM_T0();
  const int keepS = a.keep > 0 ? a.keep : a.S;
  static_assert(KQ % 2 == 0 && XQ % 4 == 0, "K split: pairs of h, float4 runs of x");
  constexpr int KX = 4 * XQ, KXS = XQ > 0 ? KX : 4;
  __shared__ __attribute__((aligned(16))) float hS[2][4 * KQ];
  extern __shared__ __attribute__((aligned(16))) float xS[];    // [S][KXS] x, then [S][blockDim] x parts
  float* xP = xS + (((int64_t)a.S * KXS + 3) & ~3);
  const int H = a.H, B = a.B, G4 = 4 * H, NT = blockDim.x;
  const int tid = threadIdx.x, u = tid >> 2, q = tid & 3;
  const bool act = u < H;
  const int uc = act ? u : H - 1;
  const int g = q * H + uc;
  const int64_t BH = (int64_t)B * H;
  // Round 6: the prologue issues all of its loads (biases, c0 / h0, the
  // matrix-core W_ih operands, the x sequence) before waiting on any, each
  // unconditionally from a clamped address with nothing selected on it
  // afterwards.  A load whose value was used under a per-lane condition was
  // sunk into its own exec-masked branch with a vmcnt(0) wait at the merge,
  // and loads behind a dependent store waited for it: one memory round trip
  // per load group.  Padding needs no select: a weight loaded for k past the
  // row (or for a gate row / unit past the shape) only ever multiplies a zero
  // of the LDS-staged x / h images (or feeds a result that is dropped), and
  // x * 0 = +-0 leaves every sum bit-identical; the staged x / h0 images get
  // their zeros by a multiply.
  // the x sequence's first XB * NT elements (all of it up to S * KX = 7168
  // at KX 48 on 448 threads), issued first; stored to LDS after the rest
  constexpr int XB = 4;                           // x loads in flight per thread
  float xv[XB];
  if constexpr (XQ > 0) {
#pragma unroll
    for (int j = 0; j < XB; ++j) {
      const int e = min(tid + j * NT, a.S * KX - 1);
      const int t = e / KX, k = e - t * KX;
      xv[j] = a.x[((int64_t)t * B + b) * a.ldx + min(k, a.din - 1)];
    }
  }
  const float bhh = a.b_hh[g];
  const float bih = XQ > 0 ? a.b_ih[g] : 0.f;
  const float creg0 = a.c0[(int64_t)b * H + uc];
  const float h0v = a.h0[(int64_t)b * H + min(tid, H - 1)];   // (NT >= 4 KQ: one h0 slot per thread)
  // the matrix-core x parts' B operands (W_ih^T, below) and bias sums, issued
  // before W_hh's so that the x parts wait on them alone: wave w's gate tiles
  // w + ti*NW (ti < 4 covers ceil(H/4) tiles over ceil(H/16) waves).  The k
  // order is permuted so a lane's operands are contiguous: MFMA step s of lane
  // l takes k = 16 (s >> 2) + 4 (l >> 4) + (s & 3) (A from the staged x rows
  // alike), so the four lane groups of a row read 64 contiguous bytes per k
  // chunk
  constexpr int XT = 4, KS = KX / 4;
  constexpr bool XMF = XQ > 0 && XM;
  float bw[XMF ? XT : 1][XMF ? KS : 1];
  float bbi[XMF ? XT : 1], bbh[XMF ? XT : 1];
  if constexpr (XMF) {
    const int lane = tid & 63, wave = tid >> 6, NW = NT >> 6;
    // float2 runs (the dispatcher takes this form only for an even din and an
    // 8-byte aligned W_ih); k >= din and gate rows >= G4 load clamped (finite)
    // weights: they meet the zero x columns / are dropped with their output rows
#pragma unroll
    for (int ti = 0; ti < XT; ++ti) {
      const int gg = min((wave + ti * NW) * 16 + (lane & 15), G4 - 1);
      const float* wr = a.w_ih + (int64_t)gg * a.din;
#pragma unroll
      for (int m = 0; m < KS / 4; ++m) {
        const int k0 = 16 * m + 4 * (lane >> 4);
        const float2 p0 = *reinterpret_cast<const float2*>(wr + min(k0, a.din - 2));
        const float2 p1 = *reinterpret_cast<const float2*>(wr + min(k0 + 2, a.din - 2));
        bw[ti][4 * m] = p0.x; bw[ti][4 * m + 1] = p0.y;
        bw[ti][4 * m + 2] = p1.x; bw[ti][4 * m + 3] = p1.y;
      }
      bbi[ti] = a.b_ih[gg];
      bbh[ti] = a.b_hh[gg];
    }
  }
  // W_hh rows j*H + u over the k pairs (8i + 2q, 8i + 2q + 1), i < KQ / 2: the
  // quad's four lanes read 32 contiguous bytes of a row per load (a lane-
  // contiguous quarter row put every lane of a load on its own cache line: the
  // prologue re-fetched W_hh from L2 many times over); issued last of the
  // prologue's loads, in flight through the x staging and the x parts
  vf2 wv[4][KQ / 2];
  // The vector width is the dispatcher's (fwd_q_dispatch: WI 2 needs H % 4 ==
  // 0 and a 16-byte aligned W_hh, WI 1 H even and 8 bytes).  A run-time
  // vec / scalar branch here was merged by the compiler into one path of
  // single-dword loads with selected addresses: 112 load instructions per lane
  // instead of 28, each touching 16 rows (13 us of the prologue, round 6).
  if constexpr (WI == 2) {
    // k runs (16 i + 4q .. + 3): 64 contiguous bytes of a row per quad and load;
    // k past H: a clamped (finite) weight times the zero h padding
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float* r = a.w_hh + (int64_t)(j * H + uc) * H;
#pragma unroll
      for (int i = 0; i < KQ / 4; ++i) {
        const float4 v = *reinterpret_cast<const float4*>(r + min(16 * i + 4 * q, H - 4));
        wv[j][2 * i] = vf2{v.x, v.y};
        wv[j][2 * i + 1] = vf2{v.z, v.w};
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float* r = a.w_hh + (int64_t)(j * H + uc) * H;
#pragma unroll
      for (int i = 0; i < KQ / 2; ++i) {
        const int k = WI ? 8 * i + 2 * q : q * KQ + 2 * i;
        if constexpr (WI == 1) {
          const float2 t2 = *reinterpret_cast<const float2*>(r + min(k, H - 2));
          wv[j][i] = vf2{t2.x, t2.y};
        } else {
          wv[j][i] = vf2{r[min(k, H - 1)], r[min(k + 1, H - 1)]};
        }
      }
    }
  }
  if constexpr (XQ > 0) {
    // stored unconditionally at the clamped index (a thread past the end
    // writes the owner's own value; a store under a per-lane condition let the
    // compiler sink its load into the branch, with a vmcnt(0) at the merge)
#pragma unroll
    for (int j = 0; j < XB; ++j) {
      const int e = min(tid + j * NT, a.S * KX - 1);
      xS[e] = xv[j] * (float)(e % KX < a.din);
    }
    for (int e0 = tid + XB * NT; e0 < a.S * KX; e0 += XB * NT) {     // longer sequences
      float v[XB];
#pragma unroll
      for (int j = 0; j < XB; ++j) {
        const int e = min(e0 + j * NT, a.S * KX - 1);
        const int t = e / KX, k = e - t * KX;
        v[j] = a.x[((int64_t)t * B + b) * a.ldx + min(k, a.din - 1)];
      }
#pragma unroll
      for (int j = 0; j < XB; ++j) {
        const int e = e0 + j * NT;
        if (e < a.S * KX) xS[e] = v[j] * (float)(e % KX < a.din);
      }
    }
  }
  if (skipv != 0) return;                        // (uniform)
  const float bh = bhh + bih;
  float creg = creg0;
  if (act && q == 0 && a.cbuf) a.cbuf[(int64_t)b * H + u] = creg;
  {
    // (clamped like the x stores: 4 KQ >= H, so a thread past 4 KQ writes the
    // value slot 4 KQ - 1 holds)
    const int e = min(tid, 4 * KQ - 1);
    hS[0][e] = h0v * (float)(e < H);
    hS[1][e] = 0.f;
    if (tid < H) a.hbuf[(int64_t)b * H + tid] = h0v;
  }
  __syncthreads();
  LSTM_TICK(0);                                  // x staged, c0 / h0, W_ih issued
  if constexpr (XMF) {
    // x parts of every step on the matrix cores: xP[t][tid(g)] = sum_k x_t[k]
    // W_ih[g][k] + b_ih[g] + b_hh[g] as v_mfma_f32_16x16x4_f32 tiles of 16 steps
    // x 16 gate rows (A = the staged x rows, B = W_ih^T, one k-ordered fmaf
    // chain per element); a tile's B operand stays in registers across the
    // step tiles
    const int lane = tid & 63, wave = tid >> 6, NW = NT >> 6;
    const int nmt = (a.S + 15) >> 4;
#pragma unroll
    for (int ti = 0; ti < XT; ++ti) {
      const int nt = wave + ti * NW;
      if (nt * 16 >= G4) break;
      const int gs = nt * 16 + (lane & 15);                 // the D column's gate
      const float bsum = bbi[ti] + bbh[ti];                  // (gs >= G4 dropped)
      const int dst = gs < G4 ? 4 * (gs % H) + gs / H : 0;
      auto x_tile = [&](int mt) {
        const int r = min(mt * 16 + (lane & 15), a.S - 1);
        const float4* xr = reinterpret_cast<const float4*>(xS + r * KX + 4 * (lane >> 4));
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        // every k chunk (no early exit at din: columns past din are the zero
        // padding of the staged x, exact zeros in the sums), so a tile's LDS
        // reads issue together instead of one wait per chunk
#pragma unroll
        for (int m = 0; m < KS / 4; ++m) {
          const float4 xv = xr[4 * m];
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.x, bw[ti][4 * m], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.y, bw[ti][4 * m + 1], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.z, bw[ti][4 * m + 2], acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv.w, bw[ti][4 * m + 3], acc, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int t = mt * 16 + 4 * (lane >> 4) + i;
          if (t < a.S && gs < G4) xP[(int64_t)t * NT + dst] = acc[i] + bsum;
        }
      };
      // the step tiles unrolled (S <= 61 in this form: kVxMax), no loop back
      // edge for the waitcnt pass to merge over (the first tile had waited
      // vmcnt(0), i.e. on W_hh's loads as well as its own W_ih operands)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
        if (mt < nmt) x_tile(mt);
      for (int mt = 4; mt < nmt; ++mt) x_tile(mt);
    }
    __syncthreads();
    LSTM_TICK(1);                                // x parts on the matrix cores
  } else if constexpr (XQ > 0) {
    // x parts of every step: W_ih rows j*H + u over x columns [q*XQ, q*XQ + XQ)
    float wx[4][XQ];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float* r = a.w_ih + (int64_t)(j * H + uc) * a.din;
#pragma unroll
      for (int kk = 0; kk < XQ; ++kk) {
        const int k = q * XQ + kk;
        wx[j][kk] = k < a.din ? r[k] : 0.f;
      }
    }
    for (int t = 0; t < a.S; ++t) {
      const float4* xp = reinterpret_cast<const float4*>(xS + t * KX + q * XQ);
      float pj[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k4 = 0; k4 < XQ / 4; ++k4) {
        const float4 v = xp[k4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          pj[j] = fmaf(v.x, wx[j][4 * k4], pj[j]);
          pj[j] = fmaf(v.y, wx[j][4 * k4 + 1], pj[j]);
          pj[j] = fmaf(v.z, wx[j][4 * k4 + 2], pj[j]);
          pj[j] = fmaf(v.w, wx[j][4 * k4 + 3], pj[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pj[j] += dpp_x1(pj[j]);
        pj[j] += dpp_x2(pj[j]);
      }
      const float mine = q == 0 ? pj[0] : q == 1 ? pj[1] : q == 2 ? pj[2] : pj[3];
      xP[(int64_t)t * NT + tid] = mine + bh;
    }
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0): W_hh (and xproj of step 0) landed
  LSTM_TICK(2);                                  // W_hh wait
  float* hb = a.hbuf + BH + (int64_t)b * H + uc;
  float* cb = a.cbuf ? a.cbuf + BH + (int64_t)b * H + uc : nullptr;
  float* gp = a.gates ? a.gates + (int64_t)b * G4 + g : nullptr;
  const int64_t gstep = (int64_t)B * G4;
  float xnext = 0.f;
  if constexpr (XQ == 0) {
    if (a.S > 0) xnext = a.xproj[(int64_t)b * G4 + g];
  }
  float ph = 0.f, pc = 0.f, pav = 0.f;
  for (int t = 0; t < a.S; ++t) {
    const float* hp = hS[t & 1] + (WI == 2 ? 4 * q : WI ? 2 * q : q * KQ);
    float* hn = hS[(t + 1) & 1];
    float xacc = 0.f;
    float4 x4 = float4{0.f, 0.f, 0.f, 0.f};
    if constexpr (A4) {
      x4 = *reinterpret_cast<const float4*>(xP + (int64_t)t * NT + 4 * uc);
    } else if constexpr (XQ > 0) {
      xacc = xP[(int64_t)t * NT + tid];
    } else {
      xacc = xnext + bh;
    }
    float2 hv[KQ / 2];
    if constexpr (WI == 2) {
      const float4* h4 = reinterpret_cast<const float4*>(hp);
#pragma unroll
      for (int i = 0; i < KQ / 4; ++i) {
        const float4 v = h4[4 * i];
        hv[2 * i] = float2{v.x, v.y};
        hv[2 * i + 1] = float2{v.z, v.w};
      }
    } else {
      const float2* h2 = reinterpret_cast<const float2*>(hp);
#pragma unroll
      for (int i = 0; i < KQ / 2; ++i) hv[i] = h2[WI ? 4 * i : i];
    }
    if constexpr (XQ == 0) {          // xproj of step t + 1, in flight through the step
      if (t + 1 < a.S) xnext = a.xproj[((int64_t)(t + 1) * B + b) * G4 + g];
    }
    // the previous step's stores, behind this step's LDS reads
    if (t > 0 && act) {
      if (q == 0) {
        hb[0] = ph;
        hb += BH;
        if (cb && t - 1 < keepS) cb[0] = pc;
        if (cb) cb += BH;
      }
      if (gp && t - 1 < keepS) gp[0] = pav;
      if (gp) gp += gstep;
    }
    vf2 pp[4] = {vf2{0.f, 0.f}, vf2{0.f, 0.f}, vf2{0.f, 0.f}, vf2{0.f, 0.f}};
#pragma unroll
    for (int i = 0; i < KQ / 2; ++i) {
      const vf2 h2v = vf2{hv[i].x, hv[i].y};
#pragma unroll
      for (int j = 0; j < 4; ++j) pp[j] = __builtin_elementwise_fma(h2v, wv[j][i], pp[j]);
    }
    float pj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pj[j] = pp[j].x + pp[j].y;
      pj[j] += dpp_x1(pj[j]);
      pj[j] += dpp_x2(pj[j]);
    }
    float ig, fg, cg, og, av;
    if constexpr (A4) {
      ig = sigm(x4.x + pj[0]);
      fg = sigm(x4.y + pj[1]);
      cg = ftanh(x4.z + pj[2]);
      og = sigm(x4.w + pj[3]);
      av = q == 0 ? ig : q == 1 ? fg : q == 2 ? cg : og;
    } else {
      const float mine = q == 0 ? pj[0] : q == 1 ? pj[1] : q == 2 ? pj[2] : pj[3];
      const float pre = xacc + mine;
      av = q == 2 ? ftanh(pre) : sigm(pre);
      ig = quad_bcast<0>(av); fg = quad_bcast<1>(av);
      cg = quad_bcast<2>(av); og = quad_bcast<3>(av);
    }
    const float c = fg * creg + ig * cg;
    const float h = og * ftanh(c);
    creg = c;
    if (act && q == 0) hn[u] = h;
    ph = h; pc = c; pav = av;
    __syncthreads();
  }
  LSTM_TICK(3);                                  // the step loop
  if (a.S > 0 && act) {
    if (q == 0) {
      hb[0] = ph;
      if (cb && a.S - 1 < keepS) cb[0] = pc;
    }
    if (gp && a.S - 1 < keepS) gp[0] = pav;
  }
}

// BR: rows of W_hh per lane of a 16-lane row (16 BR >= 4H); the body is
// lstm_bwd_q_body (lstm_cell.hpp), shared with the BPTT + weight-gradient
// launch of linear_dw.hip
template <int BR>
__global__ void __launch_bounds__(kVT)
lstm_bwd_q_kernel(LstmBwdArgs a) {
  LSTM_T0();
  lstm_bwd_q_body<BR>(a, blockIdx.x);
  LSTM_TICK(4);                                  // the whole BPTT (its own launch)
}

// Every dispatcher below returns the literal that names the instantiation it
// launched (smi_last_launch, include/surreal_mi.h).
static const char* bwd_v_dispatch_kp(const LstmBwdArgs& a, hipStream_t st) {
  const dim3 grid(a.B), blk((4 * a.H + 63) & ~63);
#define SMI_BV(KP)                                                                 \
  do {                                                                             \
    hipLaunchKernelGGL((lstm_bwd_v_kernel<KP>), grid, blk, 0, st, a);              \
    return "lstm_bwd_v_kernel<1," #KP ">";                                         \
  } while (0)
  if (a.H <= 64) SMI_BV(64);
  else if (a.H <= 104) SMI_BV(104);
  else SMI_BV(128);
#undef SMI_BV
}

// a1 (optional): the second sequence set of a dual launch (same H / x width)
template <int XQ>
static const char* fwd_q_dispatch(const LstmFwdArgs& a, hipStream_t st, const LstmFwdArgs* a1 = nullptr) {
  const dim3 grid(a.B + (a1 ? a1->B : 0)), blk((4 * a.H + 63) & ~63);
  const LstmFwdArgs& a2 = a1 ? *a1 : a;
  const int smax = a1 && a1->S > a.S ? a1->S : a.S;
  auto aligned = [&](const float* LstmFwdArgs::*p, uintptr_t m) {
    return (reinterpret_cast<uintptr_t>(a.*p) & m) == 0 && (reinterpret_cast<uintptr_t>(a2.*p) & m) == 0;
  };
  // the matrix-core x parts load W_ih rows as float2 runs
  const bool xm = XQ > 0 && a.din % 2 == 0 && aligned(&LstmFwdArgs::w_ih, 7);
  // W_hh register layout: 0 a contiguous quarter row
  // per lane, 1 k pairs interleaved over the quad (float2 loads), 2 float4 runs
  // interleaved (float4 loads); a shape / alignment the vector loads cannot
  // take steps down (the kernel has no run-time vector / scalar branch)
  int wi = 2;
  if (wi == 2 && !(a.H % 4 == 0 && aligned(&LstmFwdArgs::w_hh, 15))) wi = 1;
  if (wi == 1 && !(a.H % 2 == 0 && aligned(&LstmFwdArgs::w_hh, 7))) wi = 0;
  const size_t lds = XQ > 0 ? lstm_fwd_v_lds(smax, 4 * XQ, blk.x) : 0;
  // <KQ,XQ,xm|xv,wW[,a4]>: xm the matrix-core x parts (a4: with all four
  // gates in every lane), xv the VALU ones (and the xproj input, XQ 0)
#define SMI_FQN(KQ, TAIL)                                                          \
  (XQ == 0 ? "lstm_fwd_q_kernel<" #KQ ",0," TAIL                                   \
   : XQ == 12 ? "lstm_fwd_q_kernel<" #KQ ",12," TAIL : "lstm_fwd_q_kernel<" #KQ ",16," TAIL)
#define SMI_FQ(KQ, W)                                                              \
  do {                                                                             \
    if constexpr (XQ > 0) {                                                        \
      if (xm) {                                                                    \
        allow_lds(lstm_fwd_q_kernel<KQ, XQ, true, W>, lds);                        \
        hipLaunchKernelGGL((lstm_fwd_q_kernel<KQ, XQ, true, W>), grid, blk, lds, st, a, a2); \
        return SMI_FQN(KQ, "xm,w" #W ",a4>");                                      \
      }                                                                            \
    }                                                                              \
    allow_lds(lstm_fwd_q_kernel<KQ, XQ, false, W>, lds);                           \
    hipLaunchKernelGGL((lstm_fwd_q_kernel<KQ, XQ, false, W>), grid, blk, lds, st, a, a2); \
    return SMI_FQN(KQ, "xv,w" #W ">");                                             \
  } while (0)
  if (a.H <= 64) {
    if (wi == 2) SMI_FQ(16, 2);
    else if (wi == 1) SMI_FQ(16, 1);
    else SMI_FQ(16, 0);
  } else if (a.H <= 112 && wi == 2) {
    SMI_FQ(28, 2);
  } else if (a.H <= 104) {
    if (wi == 1) SMI_FQ(26, 1);
    else SMI_FQ(26, 0);
  } else {
    if (wi == 2) SMI_FQ(32, 2);
    else if (wi == 1) SMI_FQ(32, 1);
    else SMI_FQ(32, 0);
  }
#undef SMI_FQ
#undef SMI_FQN
}
// two sequence sets in one launch, one segment per workgroup (fused x parts)
const char* lstm_q_fwd_dual(const LstmFwdArgs& a, const LstmFwdArgs& a1, int kx, hipStream_t st) {
  if (kx <= 48) return fwd_q_dispatch<12>(a, st, &a1);
  return fwd_q_dispatch<16>(a, st, &a1);
}
const char* lstm_v_fwd(const LstmFwdArgs& a, int kx, hipStream_t st) {
  if (kx == 0) return fwd_q_dispatch<0>(a, st);
  if (kx <= 48) return fwd_q_dispatch<12>(a, st);
  return fwd_q_dispatch<16>(a, st);
}
// the BPTT's K-split form loads W_hh as float4 runs (lstm_bwd_q_body)
bool lstm_bwd_q_ok(int H, const float* w_hh) {
  return H % 4 == 0 && (reinterpret_cast<uintptr_t>(w_hh) & 15) == 0;
}
// lstm_bwd_v_kernel: the fallback for H % 4 != 0 or an unaligned W_hh
const char* lstm_v_bwd(const LstmBwdArgs& a, hipStream_t st) {
  if (lstm_bwd_q_ok(a.H, a.w_hh)) {
    const dim3 grid(a.B), blk((4 * a.H + 63) & ~63);
#define SMI_BQ(BR_)                                                                       \
    do {                                                                                  \
      hipLaunchKernelGGL((lstm_bwd_q_kernel<BR_>), grid, blk, 0, st, a);                  \
      return "lstm_bwd_q_kernel<" #BR_ ">";                                               \
    } while (0)
    if (a.H <= 64) SMI_BQ(16);
    else if (a.H <= 100) SMI_BQ(25);
    else SMI_BQ(32);
#undef SMI_BQ
  }
  return bwd_v_dispatch_kp(a, st);
}
#ifdef SMI_PROF
// this unit's phase ticks
extern "C" int smi_lstm_v_phase_ticks(unsigned long long* out /* [8] */) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lstm_ticks), sizeof(g_lstm_ticks)) != hipSuccess)
    return SMI_E_LAUNCH;
  static const unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_lstm_ticks), zero, sizeof(zero)) == hipSuccess ? SMI_OK
                                                                                        : SMI_E_LAUNCH;
}
#endif

}  // namespace smi
