// ppo_rnn_kernels.hip — the LSTM learner's own kernels (z-filter transposes,
// the policy and value row passes, decide / reduce, the optimizer apply, the
// final statistics) and their launchers (rnn_kernels.hpp); the host sequencing
// that issues them is ppo_rnn.hip.
#include <type_traits>
#include "smi_device.hpp"
#include "smi_internal.hpp"
#include "pol_rows.hpp"
#include "rnn_kernels.hpp"

namespace smi {

// ------------------------------------------------------------ small kernels
// out[t][b][:] = zfilter(obs[b][t][:]) for t < T, out[T][b][:] = zfilter(obs_next[b][0][:]),
// for t < S (S <= T+1).  z_filter.py:59-79 (clamp +-5); use_zf == 0 copies.
// One wave per row (32-bit row index math once per row, not per element):
// lane j moves columns j, j + 64 of a D <= 128-wide row, so each load and
// store instruction covers one contiguous row.  A wave takes kZfRows rows per
// trip with every load issued before the first store (one row in flight per
// wave held the launch at ~0.24 of HBM at > 256 MB working sets).
constexpr int kZfRows = 8;
__global__ void __launch_bounds__(kWG)
zf_tmajor_kernel(const float* __restrict__ obs, const float* __restrict__ obs_next, int B, int T,
                 int S, int D, int use_zf, const float* zs, const float* zq, const float* zc,
                 float eps, float* __restrict__ out, int ldo) {
  if (D <= 0) return;                            // pixel-only: no low-dim columns
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* zm = sm;
  float* zd = sm + round4(D);
  if (use_zf) zfilter_colstats(zs, zq, zc, eps, D, zm, zd);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int nrows = S * B;
  const int w0 = blockIdx.x * (kWG / 64) + (threadIdx.x >> 6), nw = gridDim.x * (kWG / 64);
  float m0 = 0.f, d0 = 1.f, m1 = 0.f, d1 = 1.f;
  if (use_zf) {
    if (lane < D) { m0 = zm[lane]; d0 = zd[lane]; }
    if (lane + 64 < D) { m1 = zm[lane + 64]; d1 = zd[lane + 64]; }
  }
  if ((D & 1) == 0 && (ldo & 1) == 0 && (reinterpret_cast<uintptr_t>(obs) & 7) == 0 &&
      (reinterpret_cast<uintptr_t>(obs_next) & 7) == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0) {
    // even widths: 8-byte lanes, floor(128 / D) rows per load instruction
    // (D = 42: three rows on 63 lanes instead of one row on 42)
    const int D2 = D >> 1, rpi = 64 / D2;
    const int lr = lane / D2, lc = lane - lr * D2;
    const bool lv = lr < rpi;
    const int cc = lv ? 2 * lc : 0;
    float2 zm2 = {0.f, 0.f}, zd2 = {1.f, 1.f};
    if (use_zf) { zm2 = float2{zm[cc], zm[cc + 1]}; zd2 = float2{zd[cc], zd[cc + 1]}; }
    const int rpt = kZfRows * rpi;                  // rows per wave and trip
    for (int row0 = w0 * rpt; row0 < nrows; row0 += nw * rpt) {
      float2 v[kZfRows];
#pragma unroll
      for (int j = 0; j < kZfRows; ++j) {
        const int row = min(row0 + j * rpi + (lv ? lr : 0), nrows - 1);
        const int t = row / B, b = row - t * B;
        const float* src = t < T ? obs + ((int64_t)b * T + t) * D : obs_next + (int64_t)b * D;
        v[j] = *reinterpret_cast<const float2*>(src + cc);
      }
#pragma unroll
      for (int j = 0; j < kZfRows; ++j) {
        const int row = row0 + j * rpi + lr;
        if (!lv || row >= nrows) continue;
        float2 o = v[j];
        if (use_zf) {
          o.x = clamp5((o.x - zm2.x) / zd2.x);
          o.y = clamp5((o.y - zm2.y) / zd2.y);
        }
        *reinterpret_cast<float2*>(out + (int64_t)row * ldo + cc) = o;
      }
    }
    return;
  }
  const int c0 = lane < D ? lane : D - 1;               // clamped: unconditional loads
  const int c1 = lane + 64 < D ? lane + 64 : D - 1;
  const bool two = D > 64;
  for (int row0 = w0 * kZfRows; row0 < nrows; row0 += nw * kZfRows) {
    float v0[kZfRows], v1[kZfRows];
#pragma unroll
    for (int j = 0; j < kZfRows; ++j) {
      const int row = min(row0 + j, nrows - 1);
      const int t = row / B, b = row - t * B;
      const float* src = t < T ? obs + ((int64_t)b * T + t) * D : obs_next + (int64_t)b * D;
      v0[j] = src[c0];
      v1[j] = two ? src[c1] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < kZfRows; ++j) {
      const int row = row0 + j;
      if (row >= nrows) break;
      float* dst = out + (int64_t)row * ldo;
      if (lane < D) {
        float v = v0[j];
        if (use_zf) v = clamp5((v - m0) / d0);
        dst[lane] = v;
      }
      if (lane + 64 < D) {
        float v = v1[j];
        if (use_zf) v = clamp5((v - m1) / d1);
        dst[lane + 64] = v;
      }
    }
  }
}

// The same transform as a tile transpose through LDS (even D <= 128, 8-byte
// aligned rows): a workgroup takes kZfSeg segments, reads each one's S rows as
// ONE contiguous run (obs[b][0..T-1] is contiguous; the t = T row comes from
// obs_next) and writes, for every step t, the kZfSeg consecutive output rows
// t*B + b0 .. (contiguous too).  The row-per-wave kernel above reads 168-byte
// rows 4.4 KB apart: partial cache lines on every row, 0.42 of HBM at > 256 MB.
constexpr int kZfSeg = 8;
__global__ void __launch_bounds__(kWG)
zf_tile_kernel(const float* __restrict__ obs, const float* __restrict__ obs_next, int B, int T,
               int S, int D, int use_zf, const float* zs, const float* zq, const float* zc,
               float eps, float* __restrict__ out, int ldo) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* zm = sm;                                  // [round4(D)]
  float* zd = sm + round4(D);
  float* tile = sm + 2 * round4(D);                // [kZfSeg][S][D]
  if (use_zf) zfilter_colstats(zs, zq, zc, eps, D, zm, zd);
  const int b0 = blockIdx.x * kZfSeg;
  const int nseg = min(kZfSeg, B - b0);
  const int D2 = D >> 1, ST = min(S, T);
  // phase 1: each segment's rows, contiguous in obs, as float2 runs; eight
  // loads in flight per thread before their LDS stores (one at a time left
  // the block latency-bound: 0.34 of HBM)
  {
    const int per = ST * D2;                        // float2 per segment from obs
    const int tot = nseg * per;
    float2* t2 = reinterpret_cast<float2*>(tile);
    const float2* o2 = reinterpret_cast<const float2*>(obs + (int64_t)b0 * T * D);
    for (int base = 0; base < tot; base += 8 * kWG) {
      float2 r[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int e = min(base + k * kWG + (int)threadIdx.x, tot - 1);
        const int bl = e / per, q = e - bl * per;
        r[k] = o2[(int64_t)bl * T * D2 + q];
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int e = base + k * kWG + threadIdx.x;
        if (e < tot) {
          const int bl = e / per, q = e - bl * per;
          t2[(int64_t)bl * S * D2 + q] = r[k];
        }
      }
    }
    if (S > T) {
      for (int e = threadIdx.x; e < nseg * D2; e += kWG) {
        const int bl = e / D2, c = e - bl * D2;
        t2[(int64_t)bl * S * D2 + T * D2 + c] =
            reinterpret_cast<const float2*>(obs_next + (int64_t)(b0 + bl) * D)[c];
      }
    }
  }
  __syncthreads();
  // phase 2: thread (bl, c2) writes column pair c2 of segment bl at every step
  const int bl = threadIdx.x / D2, c2 = threadIdx.x - bl * D2;
  if (bl >= nseg) return;
  float2 m = {0.f, 0.f}, dd = {1.f, 1.f};
  if (use_zf) { m = float2{zm[2 * c2], zm[2 * c2 + 1]}; dd = float2{zd[2 * c2], zd[2 * c2 + 1]}; }
  const float2* tp = reinterpret_cast<const float2*>(tile + (int64_t)bl * S * D) + c2;
  float* op = out + (int64_t)(b0 + bl) * ldo + 2 * c2;
  for (int t = 0; t < S; ++t) {
    float2 v = tp[t * D2];
    if (use_zf) {
      v.x = clamp5((v.x - m.x) / dd.x);
      v.y = clamp5((v.y - m.y) / dd.y);
    }
    *reinterpret_cast<float2*>(op + (int64_t)t * B * ldo) = v;
  }
}

// zf_tile_kernel with 16-byte accesses on both sides (16-byte aligned obs,
// obs_next and out, ldo % 4 == 0): the kZfSeg segments' obs rows are ONE
// contiguous run, copied to LDS as float4 (the float2 copy above issued half
// the bytes per load instruction); the output rows of a step are written as
// float4 column chunks (the last one 1-3 wide when D % 4 != 0), every chunk of
// every (step, segment) row spread over the workgroup's threads.  Same
// arithmetic per element as the kernels above.
__global__ void __launch_bounds__(kWG)
zf_tile4_kernel(const float* __restrict__ obs, const float* __restrict__ obs_next, int B, int T,
                int S, int D, int use_zf, const float* zs, const float* zq, const float* zc,
                float eps, float* __restrict__ out, int ldo, int pad) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* zm = sm;                                  // [round4(D)]
  float* zd = sm + round4(D);
  float* tile = sm + 2 * round4(D);                // [kZfSeg][T][D], obs's own layout
  float* nxt = tile + round4(kZfSeg * T * D);      // [kZfSeg][D], the obs_next rows
  if (use_zf) zfilter_colstats(zs, zq, zc, eps, D, zm, zd);
  const int b0 = blockIdx.x * kZfSeg;
  const int nseg = min(kZfSeg, B - b0);
  {
    const int tot = nseg * T * D;                   // floats of the run (all T rows)
    const int tot4 = tot >> 2;
    const float4* src = reinterpret_cast<const float4*>(obs + (int64_t)b0 * T * D);
    float4* dst = reinterpret_cast<float4*>(tile);
    for (int base = 0; base < tot4; base += 8 * kWG) {
      float4 r[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) r[k] = src[min(base + k * kWG + (int)threadIdx.x, tot4 - 1)];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int e = base + k * kWG + threadIdx.x;
        if (e < tot4) dst[e] = r[k];
      }
    }
    for (int e = (tot4 << 2) + threadIdx.x; e < tot; e += kWG) tile[e] = obs[(int64_t)b0 * T * D + e];
    if (S > T) {
      const int tn = nseg * D, tn4 = tn >> 2;
      const float* nsrc = obs_next + (int64_t)b0 * D;
      for (int e = threadIdx.x; e < tn4; e += kWG)
        reinterpret_cast<float4*>(nxt)[e] = reinterpret_cast<const float4*>(nsrc)[e];
      for (int e = (tn4 << 2) + threadIdx.x; e < tn; e += kWG) nxt[e] = nsrc[e];
    }
  }
  __syncthreads();
  if (pad) {
    // ldo == round4(D) and columns D..ldo-1 are padding nobody reads: rows are
    // written whole, as float4 chunks, zeros in the padding, so a step's
    // kZfSeg output rows are one run of whole 128-byte lines (a row with an
    // 8-byte hole made every line a partial write)
    const int cpr = ldo >> 2, per_t = nseg * cpr;
    const int groups = kWG / per_t;
    const int g = threadIdx.x / per_t, r = threadIdx.x - g * per_t;
    if (g >= groups) return;
    const int bl = r / cpr, c = 4 * (r - bl * cpr);
    float zmv[4], zdv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      zmv[j] = use_zf && c + j < D ? zm[c + j] : 0.f;
      zdv[j] = use_zf && c + j < D ? zd[c + j] : 1.f;
    }
    const bool even = (D & 1) == 0;
    for (int t = g; t < S; t += groups) {
      const float* sp = t < T ? tile + ((int64_t)bl * T + t) * D + c : nxt + bl * D + c;
      float v[4];
      if (even) {
        const float2 lo = *reinterpret_cast<const float2*>(sp);
        const float2 hi = c + 2 < D ? *reinterpret_cast<const float2*>(sp + 2) : float2{0.f, 0.f};
        v[0] = lo.x; v[1] = lo.y; v[2] = hi.x; v[3] = hi.y;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = c + j < D ? sp[j] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (use_zf && c + j < D) v[j] = clamp5((v[j] - zmv[j]) / zdv[j]);
      *reinterpret_cast<float4*>(out + ((int64_t)t * B + b0 + bl) * ldo + c) =
          float4{v[0], v[1], v[2], v[3]};
    }
    return;
  }
  if (D % 2 == 0 && D / 2 * kZfSeg <= kWG) {
    // even widths: zf_tile_kernel's phase 2 (thread = segment x column pair,
    // conflict-free 8-byte LDS reads, one float2 store per step)
    const int D2 = D >> 1;
    const int bl = threadIdx.x / D2, c2 = threadIdx.x - bl * D2;
    if (bl >= nseg) return;
    float2 m = {0.f, 0.f}, dd = {1.f, 1.f};
    if (use_zf) { m = float2{zm[2 * c2], zm[2 * c2 + 1]}; dd = float2{zd[2 * c2], zd[2 * c2 + 1]}; }
    const float2* tp = reinterpret_cast<const float2*>(tile + (int64_t)bl * T * D) + c2;
    float* op = out + (int64_t)(b0 + bl) * ldo + 2 * c2;
    for (int t = 0; t < S; ++t) {
      float2 v = t < T ? tp[t * D2] : reinterpret_cast<const float2*>(nxt + bl * D)[c2];
      if (use_zf) {
        v.x = clamp5((v.x - m.x) / dd.x);
        v.y = clamp5((v.y - m.y) / dd.y);
      }
      *reinterpret_cast<float2*>(op + (int64_t)t * B * ldo) = v;
    }
    return;
  }
  const int cpr = (D + 3) >> 2;                    // column chunks per row
  const int per_t = nseg * cpr;
  const int tot = S * per_t;
  for (int e = threadIdx.x; e < tot; e += kWG) {
    const int t = e / per_t, r = e - t * per_t;
    const int bl = r / cpr, k = r - bl * cpr;
    const int c = 4 * k, w = min(4, D - c);
    const float* sp = t < T ? tile + ((int64_t)bl * T + t) * D + c : nxt + bl * D + c;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = j < w ? sp[j] : 0.f;
      if (use_zf && j < w) v[j] = clamp5((v[j] - zm[c + j]) / zd[c + j]);
    }
    float* op = out + ((int64_t)t * B + b0 + bl) * ldo + c;
    if (w == 4) {
      *reinterpret_cast<float4*>(op) = float4{v[0], v[1], v[2], v[3]};
    } else if (w == 2) {
      *reinterpret_cast<float2*>(op) = float2{v[0], v[1]};
    } else {
      for (int j = 0; j < w; ++j) op[j] = v[j];
    }
  }
}

// zf_tile4_kernel's padded-row form as a resident grid looping over tiles,
// software-pipelined: tile i+1's obs run is loaded into registers (kZfNR
// float4 per thread) while tile i's rows are written from LDS, then stored to
// the other LDS buffer, so every workgroup keeps reads and writes in flight at
// once (the one-shot tile kernel alternated a read phase and a write phase)
constexpr int kZfNR = 10;
__global__ void __launch_bounds__(kWG)
zf_pipe_kernel(const float* __restrict__ obs, const float* __restrict__ obs_next, int B, int T,
               int S, int D, int use_zf, const float* zs, const float* zq, const float* zc,
               float eps, float* __restrict__ out, int ldo) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  float* zm = sm;
  float* zd = sm + round4(D);
  const int TD = T * D;
  const int tile_f = round4(kZfSeg * TD), buf_f = tile_f + round4(kZfSeg * D);
  float* buf0 = sm + 2 * round4(D);
  if (use_zf) zfilter_colstats(zs, zq, zc, eps, D, zm, zd);
  const int ntile = (B + kZfSeg - 1) / kZfSeg;
  const bool has_next = S > T;
  float4 r0, r1, r2, r3, r4, r5, r6, r7, r8, r9;   // kZfNR named registers (an
  float4 rn = {0.f, 0.f, 0.f, 0.f};                // array here went to scratch)
  static_assert(kZfNR == 10, "zf_pipe_kernel: ten staging registers");
// registers <- tile TL's obs run (and its obs_next rows)
#define ZF_LOAD(TL)                                                                          \
  do {                                                                                       \
    const int lb0 = (TL) * kZfSeg, lns = min(kZfSeg, B - lb0);                               \
    const int lt4 = (lns * TD) >> 2;                                                         \
    const float4* src = reinterpret_cast<const float4*>(obs + (int64_t)lb0 * TD);            \
    if (lt4 > 0) {                                                                           \
      const int tx = threadIdx.x, m = lt4 - 1;                                               \
      r0 = src[min(tx, m)]; r1 = src[min(tx + kWG, m)]; r2 = src[min(tx + 2 * kWG, m)];      \
      r3 = src[min(tx + 3 * kWG, m)]; r4 = src[min(tx + 4 * kWG, m)];                        \
      r5 = src[min(tx + 5 * kWG, m)]; r6 = src[min(tx + 6 * kWG, m)];                        \
      r7 = src[min(tx + 7 * kWG, m)]; r8 = src[min(tx + 8 * kWG, m)];                        \
      r9 = src[min(tx + 9 * kWG, m)];                                                        \
    }                                                                                        \
    const int ln4 = (lns * D) >> 2;                                                          \
    if (has_next && ln4 > 0)                                                                 \
      rn = reinterpret_cast<const float4*>(obs_next + (int64_t)lb0 * D)[min((int)threadIdx.x, ln4 - 1)]; \
  } while (0)
// registers (+ the few floats past the last whole float4) -> LDS buffer BUF
#define ZF_STASH(TL, BUF)                                                                    \
  do {                                                                                       \
    const int lb0 = (TL) * kZfSeg, lns = min(kZfSeg, B - lb0);                               \
    const int ltot = lns * TD, lt4 = ltot >> 2;                                              \
    float4* dst = reinterpret_cast<float4*>(BUF);                                            \
    const int tx = threadIdx.x;                                                              \
    if (tx < lt4) dst[tx] = r0;                                                              \
    if (tx + kWG < lt4) dst[tx + kWG] = r1;                                                  \
    if (tx + 2 * kWG < lt4) dst[tx + 2 * kWG] = r2;                                          \
    if (tx + 3 * kWG < lt4) dst[tx + 3 * kWG] = r3;                                          \
    if (tx + 4 * kWG < lt4) dst[tx + 4 * kWG] = r4;                                          \
    if (tx + 5 * kWG < lt4) dst[tx + 5 * kWG] = r5;                                          \
    if (tx + 6 * kWG < lt4) dst[tx + 6 * kWG] = r6;                                          \
    if (tx + 7 * kWG < lt4) dst[tx + 7 * kWG] = r7;                                          \
    if (tx + 8 * kWG < lt4) dst[tx + 8 * kWG] = r8;                                          \
    if (tx + 9 * kWG < lt4) dst[tx + 9 * kWG] = r9;                                          \
    for (int e = (lt4 << 2) + tx; e < ltot; e += kWG) (BUF)[e] = obs[(int64_t)lb0 * TD + e]; \
    if (has_next) {                                                                          \
      float* nb = (BUF) + tile_f;                                                            \
      const int tn = lns * D, tn4 = tn >> 2;                                                 \
      if (tx < tn4) reinterpret_cast<float4*>(nb)[tx] = rn;                                  \
      for (int e = (tn4 << 2) + tx; e < tn; e += kWG) nb[e] = obs_next[(int64_t)lb0 * D + e]; \
    }                                                                                        \
  } while (0)
  const int cpr = ldo >> 2, per_t = kZfSeg * cpr;
  const int groups = kWG / per_t;
  const int g = threadIdx.x / per_t, rr = threadIdx.x - g * per_t;
  const int bl = rr / cpr, c = 4 * (rr - bl * cpr);
  float zmv[4], zdv[4];
  __syncthreads();                                 // zm / zd
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    zmv[j] = use_zf && c + j < D ? zm[c + j] : 0.f;
    zdv[j] = use_zf && c + j < D ? zd[c + j] : 1.f;
  }
  const bool even = (D & 1) == 0;
  int tl = blockIdx.x;
  if (tl < ntile) { ZF_LOAD(tl); ZF_STASH(tl, buf0); }
  int cur = 0;
  for (; tl < ntile; tl += gridDim.x) {
    __syncthreads();                               // buffer `cur` complete
    const int nx = tl + gridDim.x;
    if (nx < ntile) ZF_LOAD(nx);                   // in flight behind the writes below
    float* buf = buf0 + cur * buf_f;
    const int b0 = tl * kZfSeg, nseg = min(kZfSeg, B - b0);
    if (g < groups && bl < nseg) {
      for (int t = g; t < S; t += groups) {
        const float* sp = t < T ? buf + (bl * T + t) * D + c : buf + tile_f + bl * D + c;
        float v[4];
        if (even) {
          const float2 lo = *reinterpret_cast<const float2*>(sp);
          const float2 hi = c + 2 < D ? *reinterpret_cast<const float2*>(sp + 2) : float2{0.f, 0.f};
          v[0] = lo.x; v[1] = lo.y; v[2] = hi.x; v[3] = hi.y;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = c + j < D ? sp[j] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (use_zf && c + j < D) v[j] = clamp5((v[j] - zmv[j]) / zdv[j]);
        *reinterpret_cast<float4*>(out + ((int64_t)t * B + b0 + bl) * ldo + c) =
            float4{v[0], v[1], v[2], v[3]};
      }
    }
    cur ^= 1;
    if (nx < ntile) ZF_STASH(nx, buf0 + cur * buf_f);
  }
#undef ZF_LOAD
#undef ZF_STASH
}

// values[b][t] = vt[t*B + b]
__global__ void __launch_bounds__(kWG)
tmajor_to_bmajor_kernel(const float* __restrict__ vt, int S, int B, float* __restrict__ v,
                        int* ci, float* cf) {
  // the learn()'s device control state starts at zero (was rnn_init_kernel,
  // a launch of its own): nothing before this point of the GAE phase reads it
  if (blockIdx.x == 0 && ci && threadIdx.x < CI_COUNT) ci[threadIdx.x] = 0;
  if (blockIdx.x == 0 && cf && threadIdx.x < CF_COUNT) cf[threadIdx.x] = 0.f;
  const int64_t n = (int64_t)S * B;
  for (int64_t e = (int64_t)blockIdx.x * kWG + threadIdx.x; e < n; e += (int64_t)gridDim.x * kWG) {
    const int b = (int)(e / S), t = (int)(e - (int64_t)b * S);
    v[e] = vt[(int64_t)t * B + b];
  }
}

// fixed-order reduction of [nb][w] double partials -> out[w] (one workgroup).
// Column j is summed by a group of L lanes (L the largest power of two <= 64
// with w * L <= kWG, so a group never straddles a wave): lane l of the group
// adds partials l, l + L, ... in order, then a butterfly over the group.  (One
// wave per column left a 2 x 42-column ZFilter reduction 21 serial
// butterflies deep per wave: 29 us for 21.5 K doubles.)  cnt != null: also
// out[w] = n (the advantage count of the GAE moments)
__global__ void __launch_bounds__(kWG)
reduce_partials_kernel(const double* __restrict__ part, int nb, int w, double* out,
                       const int* skip, double* cnt, double n) {
  if (skip && skip[0] != 0) return;
  if (cnt && threadIdx.x == 0) cnt[0] = n;
  int L = 64;
  while (L > 1 && w * L > kWG) L >>= 1;
  const int j = threadIdx.x / L, l = threadIdx.x - j * L;
  for (int jj = j; jj < w; jj += kWG / L) {
    // four partials in flight per lane (independent sums, combined in order)
    double s4[4] = {0.0, 0.0, 0.0, 0.0};
    int i = l;
    // four of those steps' loads (16 partials) per round trip, added in the
    // steps' order (a column summed by few lanes had one trip per 4 partials)
    for (; i + 15 * L < nb; i += 16 * L) {
      double v[4][4];
#pragma unroll
      for (int it = 0; it < 4; ++it)
#pragma unroll
        for (int k = 0; k < 4; ++k) v[it][k] = part[(int64_t)(i + (4 * it + k) * L) * w + jj];
#pragma unroll
      for (int it = 0; it < 4; ++it)
#pragma unroll
        for (int k = 0; k < 4; ++k) s4[k] += v[it][k];
    }
    for (; i + 3 * L < nb; i += 4 * L) {
#pragma unroll
      for (int k = 0; k < 4; ++k) s4[k] += part[(int64_t)(i + k * L) * w + jj];
    }
    for (; i < nb; i += L) s4[0] += part[(int64_t)i * w + jj];
    double s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
    for (int o = L >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (l == 0) out[jj] = s;
  }
}

// optional export of the advantages as the epochs use them and the returns,
// both [B][E] batch-major (smi_ppo_rnn_args.adv_out / ret_out)
__global__ void __launch_bounds__(kWG)
adv_export_kernel(PolRowArgs a, float* __restrict__ adv_out, float* __restrict__ ret_out) {
  const int64_t n = (int64_t)a.B * a.E;
  const AdvNorm nadv(a);
  for (int64_t e = (int64_t)blockIdx.x * kWG + threadIdx.x; e < n; e += (int64_t)gridDim.x * kWG) {
    if (adv_out) adv_out[e] = nadv(a.adv[e]);
    if (ret_out) ret_out[e] = a.ret[e];
  }
}

// rowin / ret_tm from the batch-major inputs (once per learn), field-major in
// 64-row blocks: the per-row kernels of every epoch give a thread one row, so
// lane i reads field f of row n0 + i and one load instruction covers 64
// consecutive floats
// (a row-major 100-byte row per lane made every load instruction touch ~56
// cache lines: the row kernels waited on the texture addresser, PMC TA_BUSY)
// + each row's behaviour-policy terms (behave_terms: the reference means
// refmu of PREP and the reference std are fixed for the learn)
template <int AT>
__global__ void __launch_bounds__(kWG)
row_pack_kernel(PolRowArgs a, float* __restrict__ rowin, float* __restrict__ ret_tm) {
  constexpr int AM = AT > 0 ? AT : 32;
  const int A = AT > 0 ? AT : a.A;
  float lrsig[AM], s02[AM];                        // the reference std's per-column terms
#pragma unroll
  for (int j = 0; j < (AT > 0 ? AT : A); ++j) {
    const float rsig = expf(a.ref_lv[j]);
    s02[j] = rsig * rsig;
    lrsig[j] = logf(rsig);
  }
  const int64_t N = (int64_t)a.E * a.B;
  const int W = row_w(A);
  for (int64_t n = (int64_t)blockIdx.x * kWG + threadIdx.x; n < N; n += (int64_t)gridDim.x * kWG) {
    const int t = (int)(n / a.B), b = (int)(n - (int64_t)t * a.B);
    const int64_t src = (int64_t)b * a.T + t;
    const float* acp = a.actions + src * A;
    const float* bh = a.behave + src * 2 * A;
    float ac[AM], bmu[AM], bsd[AM], rm[AM];
#pragma unroll
    for (int j = 0; j < (AT > 0 ? AT : A); ++j) {
      ac[j] = acp[j];
      bmu[j] = bh[j];
      bsd[j] = bh[A + j];
      rm[j] = a.refmu[n * A + j];
    }
#pragma unroll
    for (int j = 0; j < (AT > 0 ? AT : A); ++j) {
      rowin[rin_idx(W, n, j)] = ac[j];
      rowin[rin_idx(W, n, A + j)] = bmu[j];
      rowin[rin_idx(W, n, 2 * A + j)] = bsd[j];
    }
    rowin[rin_idx(W, n, rin_adv(A))] = a.adv[(int64_t)b * a.E + t];
    float bl, rbd;
    behave_terms<AT>(ac, bmu, bsd, rm, lrsig, s02, A, a.c_ll, bl, rbd);
    rowin[rin_idx(W, n, rin_bl(A))] = bl;
    rowin[rin_idx(W, n, rin_rbd(A))] = rbd;
    ret_tm[n] = a.ret[(int64_t)b * a.E + t];
  }
}

// forward statistics of the policy over the E*B rows (ppo.py:203-224,
// 262-284, 553-575)
// FUSE (clip mode): the same pass also writes the per-row gradient dz and the
// d/dstd block partials that policy_rows_grad_kernel would compute for this
// epoch (the clip surrogate's gradient needs no global statistic: weight 1/N,
// no KL term), bit-identically, so the gradient phase skips its row pass
template <int NT, int AT, bool FUSE>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(1, AT > 0 ? 3 : 8)))
policy_rows_stats_kernel(PolRowArgs a) {
  constexpr int AM = AT > 0 ? AT : 32;
  __shared__ float ssig[32], slsig[32], srsig[32];
  __shared__ double scr[NT / 64][PS_N];
  __shared__ float gls[FUSE ? NT / 64 : 1][32];
  const int A = AT > 0 ? AT : a.A;
  const int64_t N = (int64_t)a.E * a.B;
  const int64_t n0 = (int64_t)blockIdx.x * NT + threadIdx.x, ns = (int64_t)gridDim.x * NT;
  // one row's inputs; with a compile-time action width the row loop runs two
  // alternating register sets, the next row's loads in flight behind this
  // row's arithmetic (clamped row index: always issued, so the waitcnt pass
  // waits for exactly the set it consumes)
  // (bl / rbd: the row's behaviour-policy terms, packed once per learn)
  struct RowIn { float m[AM], rm[AM], ac[AM], adv, ret, bl, rbd; };
  auto load_row = [&](RowIn& x, int64_t n) {
    ld_row<AT>(x.m, a.mu + n * A, A);
    ld_row<AT>(x.rm, a.refmu + n * A, A);
    ld_fields<AT>(x.ac, a.rowin, N, n, 0, A);
    x.adv = a.rowin[rin_idx(row_w(A), n, rin_adv(A))];
    x.bl = a.rowin[rin_idx(row_w(A), n, rin_bl(A))];
    x.rbd = a.rowin[rin_idx(row_w(A), n, rin_rbd(A))];
    x.ret = a.ret_tm[n];
  };
  // every load ahead of the first wait (as in pol_grad_weights): the stds'
  // log_vars (column threadIdx.x, A <= 32 < NT, clamped), the first row
  // (clamped), then the scalars with the skip flag — one round trip for all
  // (the flag, the log_vars, the clip range, the moments and the row had
  // waited one after the other)
  const int jc = min((int)threadIdx.x, A - 1);
  float lvj = a.lv[jc], rlvj = a.ref_lv[jc];
  [[maybe_unused]] RowIn X0, X1;
  if constexpr (AT > 0) load_row(X0, n0 < N ? n0 : N - 1);
  const int* zi = reinterpret_cast<const int*>(g_pol_zero);
  const double* mp = (a.norm_adv && a.moments) ? a.moments : g_pol_zero;
  int sk = *(a.skip ? a.skip : zi);
  float clip_lo = a.hyper[SMI_HYPX_CLIP_LO], clip_hi = a.hyper[SMI_HYPX_CLIP_HI];
  double mom[3] = {mp[0], mp[1], mp[2]};
  // (pinned together: left to their uses, the moments' loads sank into
  // AdvNorm's branch and the clip range's past it, a scalar round trip each)
  asm volatile("" : "+s"(sk), "+s"(clip_lo), "+s"(clip_hi));
  asm volatile("" : "+s"(mom[0]), "+s"(mom[1]), "+s"(mom[2]));
  asm volatile("" : "+v"(lvj));
  asm volatile("" : "+v"(rlvj));
  if (sk != 0) return;
  if ((int)threadIdx.x < A) {
    const int j = threadIdx.x;
    ssig[j] = expf(lvj);                     // builders.py:127 std = exp(log_var)
    slsig[j] = logf(ssig[j]);                // std0.log() of ppo_net.py:40
    srsig[j] = expf(rlvj);
  }
  __syncthreads();
  // per-column terms of the learner std (log-likelihood, KL(ref || learner))
  // and the reference std (KL(ref || behaviour)), hoisted out of the row loop;
  // divisions by them become multiplications by hoisted reciprocals (one
  // rounding more per term: row_loglik_r)
  float sig[AM], isig[AM], lsig[AM], lkl[AM], s02[AM], iden2[AM], lrsig[AM];
#pragma unroll
  for (int j = 0; j < (AT > 0 ? AT : A); ++j) {
    sig[j] = ssig[j]; lsig[j] = slsig[j];
    const float rsig = srsig[j];
    isig[j] = 1.f / sig[j];
    lkl[j] = logf(sig[j] / rsig);               // row_kl(rm, rsig, m, sig)'s per-column terms
    s02[j] = rsig * rsig;
    iden2[j] = 1.f / (2.f * (sig[j] * sig[j]));
    lrsig[j] = logf(rsig);
  }
  double acc[PS_N];
#pragma unroll
  for (int k = 0; k < PS_N; ++k) acc[k] = 0.0;
  float glv[AM];
  if constexpr (FUSE) {
#pragma unroll
    for (int j = 0; j < (AT > 0 ? AT : A); ++j) glv[j] = 0.f;
  }
  const AdvNorm nadv(a, mom);
  auto row = [&](const RowIn& x, int64_t n) {
    const float* m = x.m;
    const float* rm = x.rm;
    const float* ac = x.ac;
    const float av = nadv(x.adv);
    const float ex = expf(row_loglik_r<AT>(ac, m, isig, lsig, A, a.c_ll));
    const float lp = fmaxf(ex, 1e-5f);
    const float bl = x.bl;
    acc[PS_KL] += (double)row_kl_cc<AT>(rm, m, lkl, s02, iden2, A);
    // both modes add into fixed accumulators (adapt adds an exact 0 to the
    // clip sum): merged branches had indexed acc[] by mode, i.e. from scratch
    float t_surr, t_clip;
    if (a.mode == 0) {
      const float ratio = lp / bl;
      const float cr = fminf(fmaxf(ratio, clip_lo), clip_hi);
      const float surr = -ratio * av, csur = -cr * av;
      t_surr = surr;
      t_clip = fmaxf(surr, csur);
    } else {
      t_surr = av * (lp / fmaxf(bl, 1e-2f));
      t_clip = 0.f;
    }
    acc[PS_SURR] += (double)t_surr;
    acc[PS_CLIP] += (double)t_clip;
    acc[PS_ISW] += (double)(lp / (bl + 1e-4f));
    acc[PS_BL] += (double)bl;
    acc[PS_RBD] += (double)x.rbd;
    acc[PS_RET] += (double)x.ret;
    if constexpr (FUSE) {          // policy_rows_grad_kernel's clip branch, weight a.invN
      const float ratio = lp / bl;
      const float cr = fminf(fmaxf(ratio, clip_lo), clip_hi);
      const float surr = -ratio * av, csur = -cr * av;
      const float g_lp = ((surr >= csur) ? -(a.invN * av) : 0.f) / bl;
      const float g_ll = (ex >= 1e-5f) ? g_lp * ex : 0.f;
      float dz[AM];
#pragma unroll
      for (int j = 0; j < (AT > 0 ? AT : A); ++j) {
        const float i1 = isig[j];
        const float u = (ac[j] - m[j]) * i1;
        const float gmu = g_ll * (u * i1);
        const float gsd = g_ll * (u * u * i1 - i1);
        glv[j] += gsd;
        dz[j] = gmu * (1.f - m[j] * m[j]);
      }
      st_row<AT>(a.dz + n * A, dz, A);
    }
  };
  if constexpr (AT > 0) {
    for (int64_t n = n0; n < N; n += 2 * ns) {
      load_row(X1, min(n + ns, N - 1));
      row(X0, n);
      if (n + ns >= N) break;
      load_row(X0, min(n + 2 * ns, N - 1));
      row(X1, n + ns);
    }
  } else {
    for (int64_t n = n0; n < N; n += ns) {
      RowIn X;
      load_row(X, n);
      row(X, n);
    }
  }
  if constexpr (FUSE) {            // block partials of sum_rows d/dstd, as the grad kernel
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < (AT > 0 ? AT : A); ++j) {
      const float sg = wave_sum(glv[j]);
      if (lane == 0) gls[wave][j] = sg;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < A; j += NT) {
      float sg = 0.f;
      for (int w = 0; w < NT / 64; ++w) sg += gls[w][j];
      a.lvpart[(int64_t)blockIdx.x * A + j] = sg;
    }
  }
  // all PS_N sums at once: wave butterflies, one barrier, fixed wave order
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < PS_N; ++k) {
    const double v = wave_sum_d(acc[k]);
    if (lane == 0) scr[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < PS_N) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) t += scr[w][threadIdx.x];
    a.part[(int64_t)blockIdx.x * PS_N + threadIdx.x] = t;
  }
}

// per-row gradient of the policy loss w.r.t. the tanh pre-activation (dz) and
// block partials of d loss / d log_var (ppo_net.py:29-72, ppo.py:209-217,
// 267-277): the row terms are pol_grad_row (pol_rows.hpp), shared with the
// fused head input-gradient chain's prologue
template <int NT, int AT>
__global__ void __launch_bounds__(NT)
policy_rows_grad_kernel(PolRowArgs a) {
  constexpr int AM = AT > 0 ? AT : 32;
  __shared__ PolGradShared sh;
  __shared__ float gls[NT / 64][32];
  const int A = AT > 0 ? AT : a.A;
  const int64_t N = (int64_t)a.E * a.B;
  // the thread's first row (clamped) in flight through the epoch's weights
  // and decision (the skip flag is read with the decision's scalars)
  const int64_t n0 = (int64_t)blockIdx.x * NT + threadIdx.x;
  PolGradRow<AT> x;
  x.load(a, n0 < N ? n0 : N - 1, A);
  float wsurr, wkl;
  PolGradPre pre;
  if (pol_grad_weights<8>(a, sh, wsurr, wkl, pre, a.skip)) return;
  const PolGradCols<AT> cols(pre, sh, A);
  float glv[AM];
#pragma unroll
  for (int j = 0; j < (AT > 0 ? AT : A); ++j) glv[j] = 0.f;
  const AdvNorm nadv(a, pre.mom);
  for (int64_t n = n0; n < N; n += (int64_t)gridDim.x * NT) {
    float dz[AM];
    if (n != n0) x.load(a, n, A);
    pol_grad_compute<AT>(a, cols, nadv, x, wsurr, wkl, dz, glv);
    st_row<AT>(a.dz + n * A, dz, A);
  }
  // block partials of sum_rows d/dstd (times std at the reduction: d/dlog_var)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < (AT > 0 ? AT : A); ++j) {
    const float s = wave_sum(glv[j]);
    if (lane == 0) gls[wave][j] = s;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < A; j += NT) {
    float s = 0.f;
    for (int w = 0; w < NT / 64; ++w) s += gls[w][j];
    a.lvpart[(int64_t)blockIdx.x * A + j] = s;
  }
}

__global__ void policy_decide_kernel(DecideArgs a) {
  if (threadIdx.x != 0) return;
  policy_decide_body(a, a.ps, true);
}

// single rank (no exchange between the two): the pstat reduction and the
// decision in one launch — one wave per sum, then thread 0 decides
__global__ void __launch_bounds__(kWG)
reduce_decide_kernel(const double* __restrict__ part, int nb, DecideArgs a, const int* skip) {
  if (skip && skip[0] != 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* out = const_cast<double*>(a.ps);
  for (int j = wave; j < PS_N; j += kNW) {
    double t = 0.0;
    for (int i = lane; i < nb; i += 64) t += part[(int64_t)i * PS_N + j];
    t = wave_sum_d(t);
    if (lane == 0) out[j] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) policy_decide_body(a, a.ps, true);
}

// value loss rows: V and the returns, both time-major [NE]; dV = 2 (V - R) / N
// and, in the last epoch, the sums of ppo.py:324-331.  A thread takes 4 rows
// per trip as float4s (V, R and dV are 16-byte aligned scratch rows), the
// NE % 4 tail one row per thread.
template <int NT>
__global__ void __launch_bounds__(NT)
value_rows_kernel(const float* __restrict__ V, const float* __restrict__ ret_tm, int B, int E,
                  float invN2, float* __restrict__ dV, double* part) {
  __shared__ double scr[NT / 64];
  double se = 0.0, d1 = 0.0, d2 = 0.0, r1 = 0.0, r2 = 0.0;
  auto acc = [&](float v, float r) {
    const float e = v - r;
    se += (double)(e * e);
    const double dd = (double)r - (double)v;
    d1 += dd; d2 += dd * dd;
    r1 += (double)r; r2 += (double)r * (double)r;
  };
  const int64_t N = (int64_t)E * B, N4 = N >> 2;
  const int64_t g0 = (int64_t)blockIdx.x * NT + threadIdx.x, gs = (int64_t)gridDim.x * NT;
  const float4* V4 = reinterpret_cast<const float4*>(V);
  const float4* R4 = reinterpret_cast<const float4*>(ret_tm);
  float4* D4 = reinterpret_cast<float4*>(dV);
  for (int64_t g = g0; g < N4; g += gs) {
    const float4 r = R4[g], v = V4[g];
    D4[g] = float4{invN2 * (v.x - r.x), invN2 * (v.y - r.y), invN2 * (v.z - r.z), invN2 * (v.w - r.w)};
    if (part) { acc(v.x, r.x); acc(v.y, r.y); acc(v.z, r.z); acc(v.w, r.w); }
  }
  for (int64_t n = 4 * N4 + g0; n < N; n += gs) {
    const float r = ret_tm[n], v = V[n];
    dV[n] = invN2 * (v - r);
    if (part) acc(v, r);
  }
  if (!part) return;
  const double sv[5] = {se, d1, d2, r1, r2};
  for (int k = 0; k < 5; ++k) {
    const double t = block_sum_d<NT>(sv[k], scr);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.x * 5 + k] = t;
  }
}

// column sums of obs_iter = obs[:, :E, :] (B*E rows) in fp64 -> partials
// part[gridDim.x][2][D].  Block blk takes a contiguous run of rows; a wave
// takes every 4th row of the run with lane = column (columns past 64 in a
// second pass), four rows in flight per wave (independent accumulators,
// summed in a fixed order), then the four waves meet in LDS in wave order.
// (A column per thread striding the whole batch issued one dependent load
// per row: 31 us at C3 for a 3.6 MB read.)
__global__ void __launch_bounds__(kWG)
obs_iter_colsum_kernel(const float* __restrict__ obs, int B, int T, int E, int D,
                       double* part) {
  __shared__ double red[kWG / 64][2][64];
  const int64_t N = (int64_t)B * E;
  const int64_t per = (N + gridDim.x - 1) / gridDim.x;
  const int64_t n0 = (int64_t)blockIdx.x * per, n1 = n0 + per < N ? n0 + per : N;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c0 = 0; c0 < D; c0 += 64) {
    const int c = c0 + lane;
    const bool ok = c < D;
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t n = n0 + wave; n < n1; n += 16) {
      // the four rows' loads unconditional (clamped row / column) and pinned
      // before the conditional adds (same additions): under `if (ok && m < n1)`
      // each load was its own branch with a wait, four round trips per trip
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t m = min(n + 4 * j, n1 - 1);
        const int b = (int)(m / E), t = (int)(m - (int64_t)b * E);
        v[j] = obs[((int64_t)b * T + t) * D + min(c, D - 1)];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(v[j]));
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (ok && n + 4 * j < n1) {
          s1[j] += (double)v[j];
          s2[j] += (double)(v[j] * v[j]);
        }
      }
    }
    red[wave][0][lane] = (s1[0] + s1[1]) + (s1[2] + s1[3]);
    red[wave][1][lane] = (s2[0] + s2[1]) + (s2[2] + s2[3]);
    __syncthreads();
    if (wave == 0 && ok) {
      double t1 = 0.0, t2 = 0.0;
#pragma unroll
      for (int w = 0; w < kWG / 64; ++w) {
        t1 += red[w][0][lane];
        t2 += red[w][1][lane];
      }
      part[((int64_t)blockIdx.x * 2) * D + c] = t1;
      part[((int64_t)blockIdx.x * 2 + 1) * D + c] = t2;
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kWG)
adam_split_kernel(AdamSplitArgs a) {
  if (a.skip && a.skip[0] != 0) return;
  __shared__ double red[kNW];
  __shared__ float s_coef;
  const int64_t n = a.n0 + a.n1;
  // the thread's first element (every one at the launch's grid size) is loaded
  // before the norm's partials are summed: its memory latency overlaps the sum
  const int64_t i_first = (int64_t)blockIdx.x * kWG + threadIdx.x;
  float* pf = i_first < a.n0 ? a.p0 + i_first : a.p1 + (i_first - a.n0);
  float gf = 0.f, pvf = 0.f, mf = 0.f, vf = 0.f;
  if (i_first < n) {
    gf = a.g[i_first];
    pvf = *pf;
    mf = a.m[i_first];
    vf = a.v[i_first];
  }
  const int np = a.np_dev ? a.np_dev[0] : a.np;
  // every partial of the thread in flight at once: one memory round trip for
  // np <= 16 * kWG (the dW reducer's ~2300 at C3 widths; four in flight per
  // trip took three), summed in a fixed order
  constexpr int U = 16;
  double s = 0.0;
  for (int i0 = threadIdx.x; i0 < np; i0 += U * kWG) {
    double v[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int i = i0 + k * kWG;
      v[k] = i < np ? a.part[i] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < U; ++k) s += v[k];
  }
  s = block_sum_d(s, red);
  const int t = a.step[0];      // already bumped (sumsq_part_kernel or the dW reducer's epilogue)
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(s);
    float coef = 1.f;
    if (a.max_norm > 0.f) {
      const float cc = a.max_norm / (norm + 1e-6f);
      coef = cc < 1.f ? cc : 1.f;
    }
    s_coef = coef;
    if (blockIdx.x == 0 && a.norm_out) a.norm_out[0] = norm;
  }
  __syncthreads();
  const float coef = s_coef;
  const double bc1 = 1.0 - pow((double)a.beta1, (double)t);
  const double bc2 = 1.0 - pow((double)a.beta2, (double)t);
  const float step_size = (float)((double)a.lr_ptr[0] / bc1);
  const float bc2_sqrt = (float)sqrt(bc2);
  const float w1 = (float)(1.0 - (double)a.beta1);
  const float w2 = (float)(1.0 - (double)a.beta2);
  for (int64_t i = i_first; i < n; i += (int64_t)gridDim.x * kWG) {
    const bool fst = i == i_first;
    float* pp = fst ? pf : i < a.n0 ? a.p0 + i : a.p1 + (i - a.n0);
    float g = (fst ? gf : a.g[i]) * coef;
    float p = fst ? pvf : *pp;
    if (a.wd != 0.f) g = g + a.wd * p;
    float mi = fst ? mf : a.m[i], vi = fst ? vf : a.v[i];
    mi = mi + w1 * (g - mi);
    vi = vi * a.beta2 + (w2 * g) * g;
    const float denom = sqrtf(vi) / bc2_sqrt + a.eps;
    *pp = p + (-step_size) * (mi / denom);
    a.m[i] = mi;
    a.v[i] = vi;
  }
  // The forward's weight image: the thread reads back the stem elements it
  // just wrote (W_ih, then W_hh, of layer 0 come first in p1) and stores each
  // at its transposed position.  A pass of its own, on purpose: with the store
  // inside the loop above the compiler contracted that loop's multiply-adds
  // differently, and every parameter moved in its last bit.
  if (a.wimg) {
    const int G4 = 4 * a.wH, nih = G4 * a.wdin, nw = nih + G4 * a.wH;
    for (int64_t i = i_first; i < n; i += (int64_t)gridDim.x * kWG) {
      const int64_t j = i - a.n0;
      if (j < (a.wih ? 0 : nih) || j >= nw) continue;
      const float pn = a.p1[j];
      if (j < nih) {
        const int r = (int)j / a.wdin, k = (int)j - r * a.wdin;
        a.wimg[k * G4 + r] = pn;
      } else {
        const int jh = (int)j - nih, r = jh / a.wH, k = jh - r * a.wH;
        a.wimg[nih + k * G4 + r] = pn;
      }
    }
  }
}

// also advances the optimizer's step counter (and the applied-epoch count):
// the Adam kernel that follows in the stream reads the bumped step
__global__ void __launch_bounds__(kWG)
sumsq_part_kernel(const float* __restrict__ g, int64_t n, double* part, const int* skip,
                  int* step, int* runs) {
  if (skip && skip[0] != 0) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    step[0] += 1;
    if (runs) runs[0] += 1;
  }
  __shared__ double scr[kNW];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kWG + threadIdx.x; i < n; i += (int64_t)gridDim.x * kWG) {
    const double v = (double)g[i];
    s += v * v;
  }
  s = block_sum_d(s, scr);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ void rnn_final_kernel(FinalArgs a) {
  const double n = (double)a.N;
  for (int c = threadIdx.x; c < a.D && a.use_zf; c += blockDim.x) {
    a.zs[c] += (float)a.fs[FS_Z + c];                 // z_filter.py:54-56
    a.zq[c] += (float)a.fs[FS_Z + a.D + c];
  }
  if (threadIdx.x != 0) return;
  if (a.use_zf) a.zc[0] += (float)n;
  a.stats[SMI_ST_VAL_LOSS] = (float)(a.fs[FS_SE] / n);
  const double md = a.fs[FS_D] / n, mr = a.fs[FS_R] / n;
  const float vd = (float)((a.fs[FS_D2] - n * md * md) / (n - 1.0));
  const float vr = (float)((a.fs[FS_R2] - n * mr * mr) / (n - 1.0));
  a.stats[SMI_ST_VAL_EXPL_VAR] = 1.f - vd / vr;              // ppo.py:325
  float s = 0.f;
  for (int j = 0; j < a.A; ++j) s += a.lv[j];
  a.stats[SMI_ST_AVG_LOG_SIG] = s / (float)a.A;             // ppo.py:571
  a.stats[SMI_ST_EPOCHS_RUN] = (float)a.ci[CI_RUNS];
  if (a.Ep > 0) {                                            // ppo.py:559
    const int k = a.kl_count[0];
    if (k < a.kl_capacity) a.kl_record[k] = a.stats[SMI_ST_POL_KL];
    a.kl_count[0] = k + 1;
  }
}

// ------------------------------------------------------------ launchers

// compile-time action widths 1..8 (registers); others generic (0): f is called
// with the width as a std::integral_constant
template <class F>
static void for_action_width(int A, F&& f) {
  switch (A) {
#define AW(K) case K: f(std::integral_constant<int, K>{}); break;
    AW(1) AW(2) AW(3) AW(4) AW(5) AW(6) AW(7) AW(8)
#undef AW
    default: f(std::integral_constant<int, 0>{}); break;
  }
}

int launch_row_pack(int A, int64_t rows, const PolRowArgs& p, float* rowin, float* ret_tm,
                    hipStream_t st) {
  const int g = (int)std::max<int64_t>(1, std::min<int64_t>(1024, (rows + kWG - 1) / kWG));
  for_action_width(A, [&](auto w) {
    hipLaunchKernelGGL(row_pack_kernel<decltype(w)::value>, dim3(g), dim3(kWG), 0, st, p, rowin,
                       ret_tm);
  });
  return check_launch("row_pack_kernel");
}

// workgroups of the statistics pass: at most one resident round (its register
// count leaves 3 one-wave blocks per SIMD, so the 4096-block cap of rnn_nblk
// ran a second, partly filled round: 0.34 of HBM at 65536 segments)
template <bool FUSE>
static int pol_stats_blocks_of(int A, int64_t rows) {
  static int cap[9] = {};
  const int ai = A >= 1 && A <= 8 ? A : 0;
  int& c = cap[ai];
  if (!c) {
    for_action_width(ai, [&](auto w) {
      c = resident_grid(policy_rows_stats_kernel<kRowNT, decltype(w)::value, FUSE>, kRowNT, 0);
    });
    if (c < 1) c = 1;
  }
  const int nb = rnn_nblk(rows, kRowNT);
  return nb < c ? nb : c;
}
int pol_stats_blocks(bool fuse, int A, int64_t rows) {
  return fuse ? pol_stats_blocks_of<true>(A, rows) : pol_stats_blocks_of<false>(A, rows);
}

template <bool FUSE>
static void pol_stats_launch(int nb, const PolRowArgs& p, hipStream_t st) {
  for_action_width(p.A, [&](auto w) {
    hipLaunchKernelGGL((policy_rows_stats_kernel<kRowNT, decltype(w)::value, FUSE>), dim3(nb),
                       dim3(kRowNT), 0, st, p);
  });
}
int launch_pol_stats(bool fuse, int nb, const PolRowArgs& p, hipStream_t st) {
  const int kt = ktime_begin(st);
  if (fuse) pol_stats_launch<true>(nb, p, st);     // + the clip gradient
  else pol_stats_launch<false>(nb, p, st);
  // per row: mu, refmu, actions (3A) + adv, ret, bl, rbd (4) floats read
  ktime_end(kt, KT_POLICY_STATS, 4.0 * (double)((int64_t)p.E * p.B) * (3 * p.A + 4), st);
  return check_launch("policy_rows_stats_kernel");
}

int launch_pol_grad(int nb, const PolRowArgs& p, hipStream_t st) {
  const int kt = ktime_begin(st);
  for_action_width(p.A, [&](auto w) {
    hipLaunchKernelGGL((policy_rows_grad_kernel<kRowNT, decltype(w)::value>), dim3(nb),
                       dim3(kRowNT), 0, st, p);
  });
  // per row: mu, refmu, actions (3A) + adv, bl (2) read, dz (A) written
  ktime_end(kt, KT_POLICY_GRAD, 4.0 * (double)((int64_t)p.E * p.B) * (4 * p.A + 2), st);
  return check_launch("policy_rows_grad_kernel");
}

int launch_tmajor_to_bmajor(const float* vt, int S, int B, float* v, int* ci, float* cf,
                            hipStream_t st) {
  hipLaunchKernelGGL(tmajor_to_bmajor_kernel, dim3(grid_of((int64_t)S * B)), dim3(kWG), 0, st, vt,
                     S, B, v, ci, cf);
  return check_launch("tmajor_to_bmajor_kernel");
}

int launch_reduce_partials(const double* part, int nb, int w, double* out, const int* skip,
                           double* cnt, double n, hipStream_t st) {
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(1), dim3(kWG), 0, st, part, nb, w, out, skip,
                     cnt, n);
  return check_launch("reduce_partials_kernel");
}

int launch_adv_export(const PolRowArgs& p, int64_t rows, float* adv_out, float* ret_out,
                      hipStream_t st) {
  hipLaunchKernelGGL(adv_export_kernel, dim3(grid_of(rows)), dim3(kWG), 0, st, p, adv_out,
                     ret_out);
  return check_launch("adv_export_kernel");
}

int launch_policy_decide(const DecideArgs& da, hipStream_t st) {
  hipLaunchKernelGGL(policy_decide_kernel, dim3(1), dim3(64), 0, st, da);
  return check_launch("policy_decide_kernel");
}

int launch_reduce_decide(const double* part, int nb, const DecideArgs& da, const int* skip,
                         hipStream_t st) {
  hipLaunchKernelGGL(reduce_decide_kernel, dim3(1), dim3(kWG), 0, st, part, nb, da, skip);
  return check_launch("reduce_decide_kernel");
}

int launch_value_rows(const float* V, const float* ret_tm, int B, int E, float invN2, float* dV,
                      double* part, int nb, hipStream_t st) {
  const int kt = ktime_begin(st);
  hipLaunchKernelGGL(value_rows_kernel<kRowNT>, dim3(nb), dim3(kRowNT), 0, st, V, ret_tm, B, E,
                     invN2, dV, part);
  ktime_end(kt, KT_VALUE_ROWS, 12.0 * (double)((int64_t)E * B), st);     // V, R read, dV written
  return check_launch("value_rows_kernel");
}

int launch_obs_iter_colsum(const float* obs, int B, int T, int E, int D, double* part, int nb,
                           hipStream_t st) {
  hipLaunchKernelGGL(obs_iter_colsum_kernel, dim3(nb), dim3(kWG), 0, st, obs, B, T, E, D, part);
  return check_launch("obs_iter_colsum_kernel");
}

int launch_adam_split(const AdamSplitArgs& a, int grid, double* sumsq_part, int* runs,
                      hipStream_t st) {
  const int64_t n = a.n0 + a.n1;
  const int kt = ktime_begin(st);
  if (sumsq_part) {
    hipLaunchKernelGGL(sumsq_part_kernel, dim3(grid), dim3(kWG), 0, st, a.g, n, sumsq_part, a.skip,
                       a.step, runs);
    RC_CHECK(check_launch("sumsq_part_kernel"));
  }
  hipLaunchKernelGGL(adam_split_kernel, dim3(grid), dim3(kWG), 0, st, a);
  // grad-norm pass (g: 4 B) + Adam (p, g, m, v read 16 B; p, m, v written 12 B)
  ktime_end(kt, KT_ADAM, 32.0 * (double)n, st);
  return check_launch("adam_split_kernel");
}

int launch_rnn_final(const FinalArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(rnn_final_kernel, dim3(1), dim3(64), 0, st, a);
  return check_launch("rnn_final_kernel");
}

// zf_tmajor_kernel: kZfRows (x rows per load) rows per wave and trip, 4 waves
// per block, at most 2048 blocks
static int zf_grid(int64_t rows) {
  int64_t g = (rows + 4 * kZfRows - 1) / (4 * kZfRows);
  if (g < 1) g = 1;
  return (int)(g < 2048 ? g : 2048);
}

// the time-major z-filtered copy of the batch's low-dim observations: the tile
// transpose where its shape conditions hold, else the row-per-wave kernel.
// form: 0 = that choice, 1 = the row kernel, 2 = the float2 tile, 3 = the
// float4 tile, 4 = the pipelined float4 tile writing whole padded rows (zeros
// in columns D..ldo-1; the learner's choice only with pad_ok: nothing else
// writes there), 5 = the one-shot float4 tile writing whole padded rows
// (smi_zfilter_tmajor's test / bench selection; a form whose shape conditions
// fail is SMI_E_ARG)
int launch_zf_tmajor(const float* obs, const float* obs_next, int B, int T, int S, int D,
                     int use_zf, const float* zs, const float* zq, const float* zc, float eps,
                     float* out, int ldo, hipStream_t st, int form, bool pad_ok) {
  if (D <= 0 || S <= 0) return SMI_OK;
  auto a8 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; };
  auto a16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const size_t tl = ((size_t)2 * round4(D) + (size_t)kZfSeg * S * D) * 4;
  const size_t tl4 = ((size_t)2 * round4(D) + round4(kZfSeg * T * D) + (size_t)kZfSeg * D) * 4;
  const bool tile_ok = D % 2 == 0 && D <= 128 && ldo % 2 == 0 && a8(obs) && a8(obs_next) &&
                       a8(out) && D / 2 * kZfSeg <= kWG && tl <= 64 * 1024;
  const bool tile4_ok = ldo % 4 == 0 && a16(obs) && a16(obs_next) && a16(out) && tl4 <= 64 * 1024;
  const bool pad4_ok = tile4_ok && ldo == round4(D) && kZfSeg * (ldo / 4) <= kWG;
  const size_t tlp = ((size_t)2 * round4(D) +
                      2 * ((size_t)round4(kZfSeg * T * D) + round4(kZfSeg * D))) * 4;
  const bool pipe_ok = pad4_ok && kZfSeg * T * D <= 4 * kZfNR * kWG && kZfSeg * D <= 4 * kWG &&
                       tlp <= 150 * 1024;
  if (form == 0) {
    // (from 4096 segments: at C3's 1024 the 128 tile workgroups took 14.5 us
    // against 9.7 for the row kernel; at 65536, 146 against 169 us)
    form = 1;
    if (B >= 4096) {
      if (pad_ok && pipe_ok) form = 4;
      else if (pad_ok && pad4_ok) form = 5;
      else if (tile_ok) form = 2;
      else if (tile4_ok) form = 3;
    }
  }
  const int nb = (B + kZfSeg - 1) / kZfSeg;
  if (form == 4) {
    if (!pipe_ok) return set_error(SMI_E_ARG, "zf_tmajor: pipelined padded rows do not fit");
    allow_lds(zf_pipe_kernel, tlp);
    static int cap = 0;
    if (!cap) cap = std::max(1, resident_grid(zf_pipe_kernel, kWG, tlp));
    hipLaunchKernelGGL(zf_pipe_kernel, dim3(std::min(nb, cap)), dim3(kWG), tlp, st, obs, obs_next,
                       B, T, S, D, use_zf, zs, zq, zc, eps, out, ldo);
    return check_launch("zf_pipe_kernel");
  }
  if (form == 3 || form == 5) {
    if (!tile4_ok) return set_error(SMI_E_ARG, "zf_tmajor: float4 tile needs 16-byte alignment");
    if (form == 5 && !pad4_ok) return set_error(SMI_E_ARG, "zf_tmajor: padded rows need ldo == round4(D)");
    allow_lds(zf_tile4_kernel, tl4);
    hipLaunchKernelGGL(zf_tile4_kernel, dim3(nb), dim3(kWG), tl4, st, obs, obs_next, B, T, S, D,
                       use_zf, zs, zq, zc, eps, out, ldo, form == 5 ? 1 : 0);
    return check_launch("zf_tile4_kernel");
  }
  if (form == 2) {
    if (!tile_ok) return set_error(SMI_E_ARG, "zf_tmajor: float2 tile needs even D, 8-byte alignment");
    allow_lds(zf_tile_kernel, tl);
    hipLaunchKernelGGL(zf_tile_kernel, dim3(nb), dim3(kWG), tl, st, obs, obs_next, B, T, S, D,
                       use_zf, zs, zq, zc, eps, out, ldo);
    return check_launch("zf_tile_kernel");
  }
  if (D > 128) return set_error(SMI_E_ARG, "zf_tmajor: D > 128");
  const size_t zlds = (size_t)2 * round4(D) * 4;
  hipLaunchKernelGGL(zf_tmajor_kernel, dim3(zf_grid((int64_t)S * B)), dim3(kWG), zlds, st, obs,
                     obs_next, B, T, S, D, use_zf, zs, zq, zc, eps, out, ldo);
  return check_launch("zf_tmajor_kernel");
}

int launch_zfilter_tmajor(const float* obs, const float* obs_next, int B, int T, int S, int D,
                          int use_zf, const float* zs, const float* zq, const float* zc, float eps,
                          float* out, int ldo, int form, hipStream_t st) {
  return launch_zf_tmajor(obs, obs_next, B, T, S, D, use_zf, zs, zq, zc, eps, out, ldo, st, form,
                          form >= 4);
}

}  // namespace smi
