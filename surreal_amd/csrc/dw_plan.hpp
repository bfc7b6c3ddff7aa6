// dw_plan.hpp — the planner of the grouped weight-gradient launch.  It decides
// every slab length, and with it the rounding of every grouped weight gradient:
// plain host arithmetic that must stay free of device and runtime calls.
#pragma once
#include <cstdint>
#include <cmath>
#include <algorithm>

namespace smi {

constexpr int DWD_P = 4;           // steps in flight per wave (dwd_tile, linear_dw.hip)

// tile class of a group entry: MT x NT sub-tiles and the 16-byte operand flags
constexpr int dw_cls(int mt, int nt, bool va, bool vb) {
  return mt | (nt << 3) | ((mt == 4 && va) << 7) | ((nt >= 4 && vb) << 8);
}

// Grouped weight gradients: every dW GEMM of one backward phase (the head's
// three layers and the LSTM's fused W_ih | W_hh) in ONE launch.  Workgroups are
// dealt to GEMMs by a prefix over their (tiles x slabs); slab lengths are
// balanced so every workgroup reduces about the same number of rows; each GEMM
// writes its own split-K partials, and one grouped reducer finishes them all.
// One launch and one reduce per phase instead of a launch + reduce per layer
// (and no side stream): the ~20 us fixed cost of a dW launch is paid once.
// Every GEMM is cut into up to four rectangles (DwEnt; dw_plan): its full 64 x
// 64 tiles, an M edge and an N edge whose tiles are fitted to the remainder in
// 16-wide sub-tiles, and their corner.  An entry's tiles are all of one class.
constexpr int kDwGemmMax = 8;     // GEMMs of one reducer (two launches' worth)
constexpr int kDwGroupMax = 16;   // entries of one reducer (C3: 4 + 4 + 4 + 2 of four GEMMs)
constexpr int kDwSplitMax = 16;   // entries of one grouped launch

// output tile width of the grouped launch in 16-column sub-tiles, and its
// occupancy.  Measured (C3 bench, one MI355X, interleaved trials): 64 x 64
// tiles at 3 waves per SIMD (130 VGPRs) 120.5 us per grouped launch (0.336 of
// the f32 MFMA peak), learn 8.21 ms, against 64 x 128 tiles at 2 waves per
// SIMD (222 VGPRs) 129.6 us, 8.46 ms: the third wave hides more of the
// operand-stream latency (the launch waits on memory ~60 % of its wave
// cycles, PMC SQ_WAIT_INST_ANY / SQ_WAVE_CYCLES) than the halved MFMA reuse
// per loaded byte costs.
constexpr int DWG_NT = 4;
constexpr int DWG_OCC = 3;

// whether an M x N weight gradient over row-major operands joins an open group
// (the grouped kernel's range; the dW2 / bias column included in N by the caller)
inline bool dw_group_takes(int M, int N) { return M >= 1 && N >= 1 && M <= 512 && N <= 512; }

// target workgroups of a grouped launch for `work` tile-rows.  Measured at C3 (bench, one MI355X), 21504 rows:
// 256 -> 4.44 ms of dW per learn, 512 -> 3.71, 768 -> 3.17, 1024 -> 2.83
// (45 TF/s), 1536 -> 3.32, 3072 -> 4.43; at 2688 rows (one rank of eight,
// tools/bench_dwgroup.py --segments 128): 1024 -> 65 us per launch (128-row
// slabs), 512 -> 48, 256 -> 46: slabs shorter than ~384 rows are all ramp.
// With the 64 x 64 tiles at 3 waves per SIMD (DWG_NT): 1024 -> 120.5 us
// per C3 launch, 1536 -> 110.0 (0.37 of the f32 MFMA peak), 2048 -> 110.5.
// Round 5, 128 segments (3200 rows): the LSTM's gradient alone (the heads'
// run with the BPTT) at 128 / 175 (work / 384) / 256 / 384 workgroups: 23.8 /
// 22.9 / 21.1 / 21.3 us; the whole group at 512 vs 458: 26.5 vs 28.0 us —
// work / 256.
inline int dw_group_target(double work) {
  const double w = work / 256.0;
  return w >= 1536.0 ? 1536 : w <= 128.0 ? 128 : (int)w;
}

// relative time per row of a 16-wide tail tile against a full 64 x 64 tile
// (per-workgroup clock trace of the C3 launch: 832-row slabs took 18.3 us on
// tail tiles, 47 us on full ones)
constexpr double kDwdNarrowCost = 0.4;

// 64-element groups per block of the grouped reducer
constexpr int kRedU = 4;

// One GEMM as the planner sees it, and the plan of one grouped launch: pure
// host arithmetic (no device call, no pointers), so a CPU test can sweep it
// (smi_diag_dw_plan).
struct DwPlanGemm {
  int M, N, K;
  int vec;                        // 2*VA + VB: 16-byte loads of the 4-wide A / B operands;
                                  // + 4 / 8: the A / B base pointers are 16-byte aligned
  int ones;                       // the last column is the bias gradient's all-ones column
  int split_col;                  // two-source B: first column of the second source, -1: one source
};
struct DwPlanEnt {
  int gi, m0, n0, M, N, mt, nt, cls, gm, gn, kchunk, S;
  int64_t part_off;               // its partials, floats from the plan's base
};
struct DwPlan {
  DwPlanEnt e[kDwSplitMax];
  int wg0[kDwSplitMax + 1], rb0[kDwSplitMax + 1];
  int n;
  int64_t need;                   // floats of partials
};

// The rectangles of one GEMM (up to four: interior, M edge, N edge, corner;
// an empty one is not made).  Edge tiles are fitted to the remainder in 16-
// wide sub-tiles: MT' = ceil((M mod 64) / 16) and NT' = ceil((N mod 64) / 16),
// a lane loading its MT' (NT') consecutive columns with one instruction.  A
// fitted N edge keeps the bias column in a lane of its own (dwd_load), so its
// data columns must fit 15 lanes; a two-source operand is fitted only where a
// lane's run cannot straddle the sources (one column per lane, or the edge
// wholly in the second source); 2- and 3-wide loads want the operand's base
// 16-byte aligned, as VA / VB do.  An edge that cannot be fitted stays 4 wide
// (the padded tile, 16-byte or per-column loads as before).  fit 0: the whole
// GEMM as one rectangle of padded 64 x 64 tiles; fit 1: only an M remainder of
// <= 16 rows is cut off, as 16-wide tail tiles over padded columns (the classes
// of the 8-wave launch, dw_fit_level).
inline int dw_plan_rects(const DwPlanGemm& p, int gi, int fit, DwPlanEnt* out) {
  const bool va = (p.vec & 2) != 0, vb = (p.vec & 1) != 0;
  auto ent = [&](int m0, int n0, int M, int N, int mt, int nt) {
    DwPlanEnt e{};
    e.gi = gi; e.m0 = m0; e.n0 = n0; e.M = M; e.N = N; e.mt = mt; e.nt = nt;
    e.cls = dw_cls(mt, nt, va, vb);
    e.gm = (M + 16 * mt - 1) / (16 * mt);
    e.gn = (N + 16 * nt - 1) / (16 * nt);
    return e;
  };
  const int Mf = p.M / 64 * 64, Me = p.M - Mf, Nf = p.N / 64 * 64, Ne = p.N - Nf;
  if (fit == 1 && Me >= 1 && Me <= 16) {
    int k = 0;
    if (Mf) out[k++] = ent(0, 0, Mf, p.N, 4, DWG_NT);
    out[k++] = ent(Mf, 0, Me, p.N, 1, DWG_NT);
    return k;
  }
  if (fit < 2) {
    out[0] = ent(0, 0, p.M, p.N, 4, DWG_NT);
    return 1;
  }
  int mte = (Me + 15) / 16, nte = 0;
  if ((mte == 2 || mte == 3) && !(p.vec & 4)) mte = 4;
  if (Ne > 0) {
    const int R = Ne - (p.ones ? 1 : 0);            // data columns of the edge
    nte = p.ones ? std::max(1, (R + 14) / 15) : (R + 15) / 16;
    if (nte > 4) nte = 4;
    if (p.split_col >= 0 && nte > 1 && Nf < p.split_col) nte = 4;
    if ((nte == 2 || nte == 3) && !(p.vec & 8)) nte = 4;
    // (a 16-wide tail's chain restarts in the streaming loop only, which its
    // padded tiles take with 16-byte X loads only: keep the same loop)
    if (mte == 1 && !vb) nte = 4;
  }
  int n = 0;
  if (Mf && Nf) out[n++] = ent(0, 0, Mf, Nf, 4, 4);
  if (Me && Nf) out[n++] = ent(Mf, 0, Me, Nf, mte, 4);
  if (Mf && Ne) out[n++] = ent(0, Nf, Mf, Ne, 4, nte);
  if (Me && Ne) out[n++] = ent(Mf, Nf, Me, Ne, mte, nte);
  return n;
}

// fitted edge classes on the 4-wave launch; the 8-wave launch (the weight
// gradients that share the BPTT's launch) keeps the 16-wide M tail alone
inline int dw_fit_level(int wv) { return wv == 4 ? 2 : 1; }

// Rectangles, slabs and partial offsets of one grouped launch of ng GEMMs: wv
// waves per workgroup, slots resident workgroups, cap floats of workspace, at
// most max_ent entries (a GEMM whose rectangles no longer fit is cut less).
// Returns 0, or -1 when the partials cannot fit cap.
//
// Slab lengths decide the VALUE of every output element (which rows meet in
// one fp32 MFMA chain), the tile geometry does not: an MFMA's output columns
// are independent.  So the slabs are balanced over ROW BANDS exactly as before
// the edges were fitted -- a GEMM is one band, or two when its <= 16-row tail
// is cut off and given longer slabs (a tail tile costs ~0.4 of a full tile per
// row) -- priced by their padded 64-wide tiles, and every rectangle takes the
// slabs of its band.  Fitting changes how much of a tile a workgroup computes,
// never which rows an element sums in which order: results are bit-identical
// to the padded launch's.
inline int dw_plan(const DwPlanGemm* gemms, int ng, int wv, int slots, int64_t cap, int max_ent,
                   int target_fixed, DwPlan& P) {
  constexpr int kBandMax = 6;                       // bands of one launch (tail cuts while there is room)
  constexpr int NTF = DWG_NT;
  const int rs = 4 * wv * DWD_P;                    // rows per prefetch window
  if (max_ent > kDwSplitMax) max_ent = kDwSplitMax;
  struct Band { int gi, m0, M; int64_t tiles; double cost; int64_t kc; };
  Band band[2 * kDwGemmMax];
  int nb = 0, tail_band[kDwGemmMax];                // (the GEMM's tail band, -1: one band)
  int first_band[kDwGemmMax];
  double work = 0.0, work_u = 0.0;                  // tiles x rows (x cost)
  for (int i = 0; i < ng; ++i) {
    const DwPlanGemm& g = gemms[i];
    const int tail = g.M % 64, gn = (g.N + 16 * NTF - 1) / (16 * NTF);
    const bool narrow = tail > 0 && tail <= 16;
    const bool cut = narrow && g.M > 64 && nb + (ng - i) + 1 <= kBandMax;
    first_band[i] = nb;
    tail_band[i] = -1;
    if (cut) {
      band[nb++] = Band{i, 0, g.M - tail, (int64_t)(g.M / 64) * gn, 1.0, 0};
      tail_band[i] = nb;
      band[nb++] = Band{i, g.M - tail, tail, gn, kDwdNarrowCost, 0};
    } else {
      const int gm = (g.M + 63) / 64;
      band[nb++] = Band{i, 0, g.M, (int64_t)gm * gn,
                        narrow ? ((gm - 1) + kDwdNarrowCost) / gm : 1.0, 0};
    }
  }
  for (int b = 0; b < nb; ++b) {
    work_u += (double)band[b].tiles * gemms[band[b].gi].K;
    work += (double)band[b].tiles * gemms[band[b].gi].K * band[b].cost;
  }
  // Balanced workgroups.  A launch with more work than one resident round
  // (CUs x occupancy) runs as whole rounds (one at C3: a second, partly filled
  // round was the launch's tail — the per-workgroup clock trace showed the
  // last 40 % of the span at falling concurrency), and each band's slab
  // length is set so that its slabs cost about the same time (tail tiles ~0.4
  // of a full tile per row).  Below one round every workgroup is resident
  // anyway and the span is the longest slab: equal slab lengths (shorter
  // fp32 chains on the tail tiles).
  int target = target_fixed > 0 ? target_fixed : dw_group_target(work_u);
  const bool fixed_target = target_fixed > 0;
  if (!fixed_target && target >= slots) {
    // whole rounds of at most ~2048 cost-rows per workgroup
    constexpr double kDwdRoundRows = 2048.0;
    const int rounds = (int)std::max(1.0, std::ceil(work / (slots * kDwdRoundRows)));
    target = slots * rounds;
  } else {
    for (int b = 0; b < nb; ++b) band[b].cost = 1.0;
    work = work_u;
  }
  double r0 = work / target;                        // cost-rows per workgroup
  // slab lengths are rounded up to whole prefetch windows, so the workgroup
  // count can land a few above the target; in whole rounds every extra
  // workgroup is a second round of its own (the C3 launch was 769 for 768
  // slots: the last workgroup started at 59 us and set the span), so the
  // cost-rows per workgroup grow in small steps until the count fits
  const bool rounds_fit = !fixed_target && target >= slots;
  for (int pass = 0; pass < 400; ++pass) {
    int64_t need = 0, wgs = 0;
    for (int b = 0; b < nb; ++b) {
      const DwPlanGemm& g = gemms[band[b].gi];
      int64_t S = (int64_t)(g.K * band[b].cost / r0 + 0.5);
      if (S < 1) S = 1;
      int64_t kc = ((g.K + S - 1) / S + rs - 1) / rs * rs;
      if (kc < 2 * rs) kc = 2 * rs;                 // >= 8 MFMA steps per wave
      if (kc >= g.K) kc = ((int64_t)g.K + rs - 1) / rs * rs;
      band[b].kc = kc;
      const int64_t s_b = (g.K + kc - 1) / kc;
      need += s_b * band[b].M * g.N;
      wgs += s_b * band[b].tiles;
    }
    if (need > cap) { r0 *= 2.0; continue; }         // grow the slabs until the partials fit
    if (rounds_fit && wgs > target && wgs <= 2 * target) { r0 *= 1.005; continue; }
    break;
  }
  // the rectangles, each on its band's slabs (a fitted tile stands where a
  // padded one stood: the workgroup count is the bands')
  P.n = 0;
  for (int i = 0; i < ng; ++i) {
    DwPlanEnt r[4];
    int k = 0;
    for (int fit = dw_fit_level(wv); fit >= 0; --fit) {
      k = dw_plan_rects(gemms[i], i, fit, r);
      if (P.n + k + (ng - 1 - i) <= max_ent) break;
    }
    if (k == 0 || P.n + k > max_ent) return -1;
    for (int j = 0; j < k; ++j) {
      const int b = tail_band[i] >= 0 && r[j].m0 >= band[tail_band[i]].m0 ? tail_band[i] : first_band[i];
      r[j].kchunk = (int)band[b].kc;
      r[j].S = (int)((gemms[i].K + band[b].kc - 1) / band[b].kc);
      P.e[P.n++] = r[j];
    }
  }
  int64_t off = 0;
  P.wg0[0] = 0;
  P.rb0[0] = 0;
  for (int i = 0; i < P.n; ++i) {
    DwPlanEnt& e = P.e[i];
    e.part_off = off;
    off += ((int64_t)e.S * e.M * e.N + 3) / 4 * 4;   // (every entry's partials 16-byte aligned)
    P.wg0[i + 1] = P.wg0[i] + e.gm * e.gn * e.S;
    P.rb0[i + 1] = P.rb0[i] + (int)(((int64_t)e.M * e.N + 64 * kRedU - 1) / (64 * kRedU));
  }
  if (off > cap) return -1;
  P.need = off;
  return 0;
}

}  // namespace smi
