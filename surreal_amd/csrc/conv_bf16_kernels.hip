// conv_bf16_kernels.hip — the general convolution layer of conv_kernels.hip with
// bf16 operands: the same NCHW tensors, geometry ranges, padding, uint8-or-fp32
// input read in place, div255, ReLU / mask epilogues, stop flag and in-kernel
// tile loop, as implicit GEMMs on v_mfma_f32_16x16x32_bf16 (8 times the
// multiply-adds of v_mfma_f32_16x16x4_f32 per instruction).  Parameters,
// activations and gradients stay fp32 in memory: an operand becomes bf16 on its
// way from the prefetch registers into LDS and nowhere else.
//
// Arithmetic: fp32 -> bf16 is round-to-nearest-even (v_cvt_pk_bf16_f32: NaN
// stays NaN, +-inf and -0.0 keep their bits), uint8 -> bf16 is exact (8
// significand bits), a product of two bf16 values is exact in fp32 and the MFMA
// accumulates in fp32: after staging the only rounding is that of the fp32
// sums.  Bias, / 255, ReLU and the dx mask act on the fp32 sums exactly as in
// conv_kernels.hip; db is the sum of dy as given (fp32, never rounded).
//
// All three kernels compute  C[R][Q] = sum_z A[R][z] * B[Q][z]  on the 64 x 64
// tiles of conv_plan.hpp, the reduction in chunks of 64 (conv_bf16_plan.hpp).
// A workgroup of 4 waves stages a 64 x 64 bf16 slice of A and of B in LDS and
// wave w owns the 32 x 32 quarter (w >> 1, w & 1) as 2 x 2 MFMA tiles: per
// k-step of 32, lane (row l & 15, group l >> 4) reads the 8 consecutive-z bf16
// of its row for two A and two B tiles (4 ds_read_b128) for 4 MFMAs on 4
// independent accumulator chains.  The next slice's global loads are issued
// into registers before the current slice's MFMAs.
//
// LDS: all traffic is in 16-byte vectors of 8 bf16, a row is 9 of them (8 of
// data + 1 of padding = 144 bytes = 36 dwords).  Operand read: the 16 lanes of
// a quarter wave hold rows 0..15 at one z group, so they start at dwords
// 36 r mod 64 = 0 36 8 44 16 52 24 60 32 4 40 12 48 20 56 28: 16 different
// multiples of 4, their 16-byte reads cover each of the 64 banks once (and any
// 8 consecutive lanes cover 32 banks once: 36 r mod 32 = 4 r).  The staging
// stores are 16-byte too: either the same pattern (one row per lane) or 8 lanes
// along a row and the next 8 on the next row, 2-way on 4 banks at worst.
//
//   forward          A = weights [cout][cin k k]: thread (row tid >> 3 (+ 32),
//                    z 8 (tid & 7) ..+7), two 16-byte loads where the pointer
//                    and row length allow it; B = patches, one output pixel per
//                    row: thread (pixel tid & 63, z 16 (tid >> 6) ..+15), so a
//                    wave's z is uniform and its lanes walk neighbouring pixels
//   backward input   per stride-parity class (blockIdx.y), as conv_dx_kernel:
//                    dense taps, no scatter, no atomics; the same two maps
//   backward weight  A = dy [cout][pixels], B = patches [cin k k][pixels]: both
//                    thread (row tid >> 3 (+ 32), pixels 8 (tid & 7) ..+7); the
//                    n Ho Wo reduction is cut into `splits` consecutive ranges
//                    (blockIdx.y), every workgroup writes its whole tile of
//                    partial sums into the caller's scratch and conv_dw_reduce
//                    (conv_kernels.hip) adds them in a fixed order.  db: every
//                    thread adds the fp32 dy values it fetched, the 8 threads
//                    of a row are added by 3 xor-shuffles: fixed order too.
#include "smi_device.hpp"
#include "smi_internal.hpp"
#include "smi_launch.hpp"
#include "bf16_stage.hpp"
#include "conv_bf16_plan.hpp"

namespace smi {

namespace {

constexpr int LDV = kConvBfLdv;
constexpr int NJ = kConvTile * kConvBfChunk / kWG;     // staged elements per thread and tile: 16
static_assert(NJ == 16 && kWG == 256 && kConvTile == 64 && kConvBfChunk == 64,
              "the staging maps below are written for 256 threads, 64 x 64 slices");

__device__ __forceinline__ float ldf(const float* p) { return *p; }
__device__ __forceinline__ float ldf(const unsigned char* p) { return (float)*p; }

// (pack8, mfma32: bf16_stage.hpp)

// one staged slice: acc[i][j] += A[rh 32 + i 16 ..][z] * B[qh 32 + j 16 ..][z]
__device__ __forceinline__ void conv_mma(const uint4* As, const uint4* Bs, f32x4 (&acc)[2][2],
                                         int w, int l) {
  const int lm = l & 15, lg = l >> 4;
  const uint4* ap = As + ((w >> 1) * 32 + lm) * LDV + lg;
  const uint4* bp = Bs + ((w & 1) * 32 + lm) * LDV + lg;
#pragma unroll
  for (int kk = 0; kk < kConvBfChunk / 32; ++kk) {
    const uint4 a0 = ap[kk * 4], a1 = ap[16 * LDV + kk * 4];
    const uint4 b0 = bp[kk * 4], b1 = bp[16 * LDV + kk * 4];
    acc[0][0] = mfma32(a0, b0, acc[0][0]);
    acc[0][1] = mfma32(a0, b1, acc[0][1]);
    acc[1][0] = mfma32(a1, b0, acc[1][0]);
    acc[1][1] = mfma32(a1, b1, acc[1][1]);
  }
}

// the two staging maps (file header) from the prefetch registers into LDS
__device__ __forceinline__ void stage_rows8(uint4* S, const float (&v)[NJ], int tid) {
  S[(tid >> 3) * LDV + (tid & 7)] = pack8(v);
  S[((tid >> 3) + 32) * LDV + (tid & 7)] = pack8(v + 8);
}
__device__ __forceinline__ void stage_row16(uint4* S, const float (&v)[NJ], int l, int w) {
  S[l * LDV + 2 * w] = pack8(v);
  S[l * LDV + 2 * w + 1] = pack8(v + 8);
}

// tile row of accumulator element e of acc[i][.], tile column of acc[.][j]
// (the 16x16 output map of the bf16 MFMA is that of the fp32 one)
__device__ __forceinline__ int acc_row(int w, int l, int i, int e) {
  return (w >> 1) * 32 + i * 16 + (l >> 4) * 4 + e;
}
__device__ __forceinline__ int acc_col(int w, int l, int j) { return (w & 1) * 32 + j * 16 + (l & 15); }

__device__ __forceinline__ void acc_zero(f32x4 (&acc)[2][2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// (c, y, x) of reduction index z over [.][ny][nx], and one step along it
struct KPos { int c, y, x; };
__device__ __forceinline__ KPos kpos_of(int z, int ny, int nx) {
  KPos q;
  q.c = z / (ny * nx);
  const int r = z - q.c * (ny * nx);
  q.y = r / nx;
  q.x = r - q.y * nx;
  return q;
}
__device__ __forceinline__ void kpos_step(KPos& q, int ny, int nx) {
  if (++q.x == nx) {
    q.x = 0;
    if (++q.y == ny) { q.y = 0; ++q.c; }
  }
}

}  // namespace

// ------------------------------------------------------------------ forward
template <typename T, bool VW>
__global__ void __launch_bounds__(kWG)
conv_fwd_bf16_kernel(const T* __restrict__ x, const float* __restrict__ wgt,
                     const float* __restrict__ bias, float* __restrict__ y, ConvGeom g, int64_t n,
                     int act, int div255, const int* skip) {
  if (skip && skip[0] != 0) return;
  __shared__ uint4 As[kConvTile * LDV];
  __shared__ uint4 Bs[kConvTile * LDV];
  const int tid = threadIdx.x, l = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t NP = n * g.P;
  const int rT = (g.cout + kConvTile - 1) / kConvTile;
  const int64_t tiles = ((NP + kConvTile - 1) / kConvTile) * rT;
  const int HW = g.h * g.w;

  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int r0 = (int)(t % rT) * kConvTile;
    const int64_t q0 = (t / rT) * kConvTile;
    // this thread's output pixel
    const int64_t q = q0 + l;
    const bool qok = q < NP;
    const int64_t nn = qok ? q / g.P : 0;
    const int pp = qok ? (int)(q - nn * g.P) : 0;
    const int oy = pp / g.wo, ox = pp - oy * g.wo;
    const int iy0 = oy * g.s - g.p, ix0 = ox * g.s - g.p;
    const T* xb = x + nn * (int64_t)g.cin * HW;

    float pa[NJ], pb[NJ];
    auto fetch = [&](int z0) {
      const int zz = z0 + 8 * (tid & 7);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int co = r0 + (tid >> 3) + 32 * h;
        const float* wr = wgt + (int64_t)co * g.K + zz;
        if constexpr (VW) {
#pragma unroll
          for (int v4 = 0; v4 < 2; ++v4) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (co < g.cout && zz + 4 * v4 < g.K)   // K % 4 == 0: the four are in or out together
              v = *reinterpret_cast<const float4*>(wr + 4 * v4);
            pa[8 * h + 4 * v4] = v.x; pa[8 * h + 4 * v4 + 1] = v.y;
            pa[8 * h + 4 * v4 + 2] = v.z; pa[8 * h + 4 * v4 + 3] = v.w;
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) pa[8 * h + e] = (co < g.cout && zz + e < g.K) ? wr[e] : 0.f;
        }
      }
      const int zb = z0 + 16 * w;
      KPos kp = kpos_of(zb, g.k, g.k);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int iy = iy0 + kp.y, ix = ix0 + kp.x;
        const bool ok = qok && zb + j < g.K && iy >= 0 && iy < g.h && ix >= 0 && ix < g.w;
        pb[j] = ok ? ldf(xb + kp.c * HW + iy * g.w + ix) : 0.f;
        kpos_step(kp, g.k, g.k);
      }
    };

    f32x4 acc[2][2];
    acc_zero(acc);
    fetch(0);
    for (int z0 = 0; z0 < g.K; z0 += kConvBfChunk) {
      stage_rows8(As, pa, tid);
      stage_row16(Bs, pb, l, w);
      __syncthreads();
      if (z0 + kConvBfChunk < g.K) fetch(z0 + kConvBfChunk);
      conv_mma(As, Bs, acc, w, l);
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t qq = q0 + acc_col(w, l, j);
      if (qq >= NP) continue;
      const int64_t n2 = qq / g.P;
      const int p2 = (int)(qq - n2 * g.P);
      float* yo = y + n2 * (int64_t)g.cout * g.P + p2;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int co = r0 + acc_row(w, l, i, e);
          if (co < g.cout) {
            float v = acc[i][j][e];
            if (div255) v = v / 255.0f;
            v += bias[co];
            yo[(int64_t)co * g.P] = act == ACT_RELU ? fmaxf(v, 0.f) : v;
          }
        }
    }
  }
}

// ----------------------------------------------------------- backward, input
// blockIdx.y = ry * s + rx.  A (taps of w): row = input channel, z = (co, ay, ax)
// over the class's taps; B (dy): row = the thread's input pixel of the class
__global__ void __launch_bounds__(kWG)
conv_dx_bf16_kernel(const float* __restrict__ dy, const float* __restrict__ wgt,
                    const float* __restrict__ mask, float* __restrict__ dx, ConvGeom g, int64_t n,
                    const int* skip) {
  if (skip && skip[0] != 0) return;
  __shared__ uint4 As[kConvTile * LDV];
  __shared__ uint4 Bs[kConvTile * LDV];
  const int tid = threadIdx.x, l = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ry = blockIdx.y / g.s, rx = blockIdx.y - ry * g.s;
  const int fy = conv_class_first(ry, g.s, g.p), fx = conv_class_first(rx, g.s, g.p);
  const int ny = conv_class_count(g.h, ry, g.s, g.p), nx = conv_class_count(g.w, rx, g.s, g.p);
  const int ty = conv_class_taps(g.k, ry, g.s), tx = conv_class_taps(g.k, rx, g.s);
  const int64_t Qc = n * ny * nx;
  if (Qc == 0) return;                                   // (uniform in the workgroup)
  const int kk2 = g.k * g.k, Z = g.cout * ty * tx, nyx = ny * nx;
  const int rT = (g.cin + kConvTile - 1) / kConvTile;
  const int64_t tiles = ((Qc + kConvTile - 1) / kConvTile) * rT;

  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int r0 = (int)(t % rT) * kConvTile;
    const int64_t q0 = (t / rT) * kConvTile;
    const int64_t q = q0 + l;
    const bool qok = q < Qc;
    const int64_t nn = qok ? q / nyx : 0;
    const int rem = qok ? (int)(q - nn * nyx) : 0;
    const int jy = rem / nx, jx = rem - jy * nx;
    // output position of tap (ay, ax) = (0, 0); tap (ay, ax) reads (oyb - ay, oxb - ax)
    const int oyb = (fy + g.s * jy + g.p - ry) / g.s, oxb = (fx + g.s * jx + g.p - rx) / g.s;
    const float* dyb = dy + nn * (int64_t)g.cout * g.P;

    float pa[NJ], pb[NJ];
    auto fetch = [&](int z0) {
      const int zz = z0 + 8 * (tid & 7);
      const int ci0 = r0 + (tid >> 3);
      KPos ka = kpos_of(zz, ty, tx);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        // w[co][ci][ry + s ay][rx + s ax]
        const float* wz = wgt + (int64_t)ka.c * g.cin * kk2 + (ry + g.s * ka.y) * g.k + rx + g.s * ka.x;
        pa[e] = (zz + e < Z && ci0 < g.cin) ? wz[ci0 * kk2] : 0.f;
        pa[8 + e] = (zz + e < Z && ci0 + 32 < g.cin) ? wz[(ci0 + 32) * kk2] : 0.f;
        kpos_step(ka, ty, tx);
      }
      const int zb = z0 + 16 * w;
      KPos kp = kpos_of(zb, ty, tx);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int oy = oyb - kp.y, ox = oxb - kp.x;
        const bool ok = qok && zb + j < Z && oy >= 0 && oy < g.ho && ox >= 0 && ox < g.wo;
        pb[j] = ok ? dyb[(int64_t)kp.c * g.P + oy * g.wo + ox] : 0.f;
        kpos_step(kp, ty, tx);
      }
    };

    f32x4 acc[2][2];
    acc_zero(acc);
    fetch(0);
    for (int z0 = 0; z0 < Z; z0 += kConvBfChunk) {
      stage_rows8(As, pa, tid);
      stage_row16(Bs, pb, l, w);
      __syncthreads();
      if (z0 + kConvBfChunk < Z) fetch(z0 + kConvBfChunk);
      conv_mma(As, Bs, acc, w, l);
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t qq = q0 + acc_col(w, l, j);
      if (qq >= Qc) continue;
      const int64_t n2 = qq / nyx;
      const int rem2 = (int)(qq - n2 * nyx);
      const int jy2 = rem2 / nx, jx2 = rem2 - jy2 * nx;
      const int64_t o = n2 * (int64_t)g.cin * g.h * g.w + (fy + g.s * jy2) * g.w + fx + g.s * jx2;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int ci = r0 + acc_row(w, l, i, e);
          if (ci < g.cin) {
            const int64_t idx = o + (int64_t)ci * g.h * g.w;
            float v = acc[i][j][e];
            if (mask) v = mask[idx] > 0.f ? v : 0.f;
            dx[idx] = v;
          }
        }
    }
  }
}

// ---------------------------------------------------------- backward, weight
// blockIdx.x = tile of dW [cout][K] (row tile fastest), blockIdx.y = split.
// The thread's two dy rows and two patch columns are fixed for the whole
// kernel, its 8 pixels move.
template <typename T>
__global__ void __launch_bounds__(kWG)
conv_dw_bf16_kernel(const float* __restrict__ dy, const T* __restrict__ x, float* __restrict__ part,
                    ConvGeom g, int64_t n, ConvDwPlan pl, const int* skip) {
  if (skip && skip[0] != 0) return;
  __shared__ uint4 As[kConvTile * LDV];
  __shared__ uint4 Bs[kConvTile * LDV];
  const int tid = threadIdx.x, l = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t NP = n * g.P;
  const int rT = (g.cout + kConvTile - 1) / kConvTile;
  const int r0 = (int)(blockIdx.x % rT) * kConvTile, k0 = (int)(blockIdx.x / rT) * kConvTile;
  const int kk2 = g.k * g.k, HW = g.h * g.w;
  int koff[2], ky[2], kx[2];             // ci H W + ky W + kx;  ky < 0: no such column
  bool cok[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int kc = k0 + (tid >> 3) + 32 * h;
    const int ci = kc / kk2, r = kc - ci * kk2;
    ky[h] = r / g.k;
    kx[h] = r - ky[h] * g.k;
    koff[h] = ci * HW + ky[h] * g.w + kx[h];
    if (kc >= g.K) ky[h] = -(1 << 20);
    cok[h] = r0 + (tid >> 3) + 32 * h < g.cout;
  }
  const int64_t c_begin = (int64_t)blockIdx.y * pl.per;
  const int64_t c_end = c_begin + pl.per < pl.chunks ? c_begin + pl.per : pl.chunks;
  const bool want_db = k0 == 0;

  float pa[NJ], pb[NJ];
  float dbs[2] = {0.f, 0.f};
  auto fetch = [&](int64_t c) {
    const int64_t m = c * kConvBfChunk + 8 * (tid & 7);
    int64_t nn = m / g.P;
    const int pp = (int)(m - nn * g.P);
    int oy = pp / g.wo, ox = pp - oy * g.wo;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool mok = m + e < NP;
      const float* dyp = dy + (nn * g.cout + r0 + (tid >> 3)) * (int64_t)g.P + oy * g.wo + ox;
      const int iy0 = oy * g.s - g.p, ix0 = ox * g.s - g.p;
      const T* xb = x + nn * (int64_t)g.cin * HW + iy0 * g.w + ix0;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        pa[8 * h + e] = (mok && cok[h]) ? dyp[(int64_t)32 * h * g.P] : 0.f;
        const int iy = iy0 + ky[h], ix = ix0 + kx[h];
        const bool ok = mok && iy >= 0 && iy < g.h && ix >= 0 && ix < g.w;
        pb[8 * h + e] = ok ? ldf(xb + koff[h]) : 0.f;
      }
      if (++ox == g.wo) {
        ox = 0;
        if (++oy == g.ho) { oy = 0; ++nn; }
      }
    }
    if (want_db) {
#pragma unroll
      for (int e = 0; e < 8; ++e) { dbs[0] += pa[e]; dbs[1] += pa[8 + e]; }
    }
  };

  f32x4 acc[2][2];
  acc_zero(acc);
  if (c_begin < c_end) fetch(c_begin);
  for (int64_t c = c_begin; c < c_end; ++c) {
    stage_rows8(As, pa, tid);
    stage_rows8(Bs, pb, tid);
    __syncthreads();
    if (c + 1 < c_end) fetch(c + 1);
    conv_mma(As, Bs, acc, w, l);
    __syncthreads();
  }
  // the whole tile of partial sums (zeros where the split met no pixel)
  float* out = part + (int64_t)blockIdx.y * pl.slab;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int kc = k0 + acc_col(w, l, j);
    if (kc >= g.K) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int co = r0 + acc_row(w, l, i, e);
        if (co < g.cout) out[(int64_t)co * g.K + kc] = acc[i][j][e];
      }
  }
  if (want_db) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float s = dbs[h];
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) s += __shfl_xor(s, o, 64);
      if ((tid & 7) == 0 && cok[h]) out[(int64_t)g.cout * g.K + r0 + (tid >> 3) + 32 * h] = s;
    }
  }
}

// ------------------------------------------------------------------- host
int conv2d_forward_bf16(const void* x, int x_u8, int div255, int64_t n, const ConvGeom& g,
                        const float* wgt, const float* bias, int act, float* y, hipStream_t st,
                        const int* skip) {
  if (n < 1) return SMI_OK;
  const bool vw = g.K % 4 == 0 && (reinterpret_cast<uintptr_t>(wgt) & 15) == 0;
  const int64_t tiles = conv_fwd_tiles(g, n);
  const int kt = ktime_begin(st);
#define SMI_CONV_FWD(T, VW)                                                                      \
  do {                                                                                           \
    auto k = conv_fwd_bf16_kernel<T, VW>;                                                        \
    const int64_t rg = resident_grid(k, kWG, 0);                                                 \
    hipLaunchKernelGGL(k, dim3((unsigned)(tiles < rg ? tiles : rg)), dim3(kWG), 0, st,           \
                       static_cast<const T*>(x), wgt, bias, y, g, n, act, div255, skip);         \
  } while (0)
  if (x_u8) { if (vw) SMI_CONV_FWD(unsigned char, true); else SMI_CONV_FWD(unsigned char, false); }
  else { if (vw) SMI_CONV_FWD(float, true); else SMI_CONV_FWD(float, false); }
#undef SMI_CONV_FWD
  ktime_end(kt, KT_CNN_FWD, 2.0 * (double)n * g.P * g.K * g.cout, st);
  return check_launch("conv_fwd_bf16_kernel");
}

int conv2d_backward_input_bf16(const float* dy, int64_t n, const ConvGeom& g, const float* wgt,
                               const float* mask, float* dx, hipStream_t st, const int* skip) {
  if (n < 1) return SMI_OK;
  const int64_t tiles = conv_dx_max_tiles(g, n);
  const int64_t rg = resident_grid(conv_dx_bf16_kernel, kWG, 0);
  const int64_t per = (rg + g.s * g.s - 1) / (g.s * g.s);          // resident workgroups per class
  const int kt = ktime_begin(st);
  hipLaunchKernelGGL(conv_dx_bf16_kernel, dim3((unsigned)(tiles < per ? tiles : per), g.s * g.s),
                     dim3(kWG), 0, st, dy, wgt, mask, dx, g, n, skip);
  ktime_end(kt, KT_CNN_BWD, 2.0 * (double)n * g.P * g.K * g.cout, st);
  return check_launch("conv_dx_bf16_kernel");
}

int conv2d_backward_weight_bf16(const float* dy, const void* x, int x_u8, int div255, int64_t n,
                                const ConvGeom& g, float* dw, float* db, float* part,
                                hipStream_t st, const int* skip) {
  if (n < 1) return SMI_OK;
  const ConvDwPlan pl = conv_bf16_dw_plan(g, n);
  const int kt = ktime_begin(st);
  if (x_u8)
    hipLaunchKernelGGL(conv_dw_bf16_kernel<unsigned char>, dim3(pl.tiles, pl.splits), dim3(kWG), 0,
                       st, dy, static_cast<const unsigned char*>(x), part, g, n, pl, skip);
  else
    hipLaunchKernelGGL(conv_dw_bf16_kernel<float>, dim3(pl.tiles, pl.splits), dim3(kWG), 0, st, dy,
                       static_cast<const float*>(x), part, g, n, pl, skip);
  ktime_end(kt, KT_CNN_BWD, 2.0 * (double)n * g.P * g.K * g.cout, st);
  RC_CHECK(check_launch("conv_dw_bf16_kernel"));
  return launch_conv_dw_reduce(part, pl.splits, pl.slab, (int64_t)g.cout * g.K, dw, db, div255, st,
                               skip);
}

}  // namespace smi
