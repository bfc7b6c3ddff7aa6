// conv_kernels.hip — one general convolution layer over NCHW tensors, the
// conv_layers of FFQfunc (surreal/model/q_net.py:82-102,112-119: SAME-padded,
// padding = k / 2, free shape), as implicit GEMMs on v_mfma_f32_16x16x4_f32.
// No im2col matrix exists in memory: every kernel gathers its patch operand
// from the tensor into LDS, and the zero halo is supplied by that gather.
//
// All three kernels compute  C[R][Q] = sum_z A[R][z] * B[Q][z]  on 64 x 64
// tiles (conv_plan.hpp).  A workgroup of 4 waves stages a 64 x 32 slice of A and
// of B in LDS (row stride 34 floats: the MFMA operand reads, lane (row l & 15,
// z l >> 4), touch 32 different banks per half wave, and the staging stores
// run along rows or 2-way at worst), wave w owns the 32 x 32 quarter (w >> 1,
// w & 1) as 2 x 2 MFMA tiles (4 independent accumulator chains, 4 LDS reads per
// 4 MFMAs), and the next slice's global loads are issued into registers before
// the current slice's MFMAs so their latency hides behind them.
//
//   forward          A = weights [cout][cin k k] (16-byte loads when the
//                    pointer and row length allow it, element loads otherwise),
//                    B = patches of x, one output pixel per row; epilogue
//                    act(sum (/ 255) + b) into y [n][cout][Ho][Wo]
//   backward input   per stride-parity class (blockIdx.y) of the INPUT pixels:
//                    A = the class's taps of w per input channel, B = dy at
//                    the output positions those taps reach: every tap is dense,
//                    nothing is scattered and there is no atomic; epilogue
//                    [mask > 0] into dx (each input pixel is in one class)
//   backward weight  A = dy [cout][pixels], B = patches [cin k k][pixels]; the
//                    reduction over n Ho Wo is cut into `splits` consecutive
//                    ranges (blockIdx.y), each workgroup writes its whole tile
//                    of partial sums into the caller's scratch, and
//                    conv_dw_reduce sums the partials in a fixed order: no float
//                    atomics, two runs are bit-identical.  db is the row sum
//                    of the A slices, by the k-tile-0 workgroups.
//
// Tiles beyond the resident grid are looped over inside the kernel.
//
// Pixel scaling: with div255 the kernels feed the unscaled values (raw bytes
// are exact in fp32) to the MFMAs and divide the SUMS by 255 (IEEE division):
// in the forward epilogue and in the weight-gradient reducer.  torch computes
// conv(fl(x / 255)); the two agree to fp32 rounding of the sum, as in
// cnn_kernels.hip.
#include "smi_device.hpp"
#include "smi_internal.hpp"
#include "conv_plan.hpp"

namespace smi {

namespace {

constexpr int LD = kConvLd;
constexpr int NJ = kConvTile * kConvChunk / kWG;       // staged elements per thread and tile: 8
static_assert(NJ == 8 && kWG == 256 && kConvTile == 64 && kConvChunk == 32,
              "the staging maps below are written for 256 threads, 64 x 32 slices");

__device__ __forceinline__ float ldf(const float* p) { return *p; }
__device__ __forceinline__ float ldf(const unsigned char* p) { return (float)*p; }

// one staged slice: acc[i][j] += A[rh 32 + i 16 ..][z] * B[qh 32 + j 16 ..][z]
__device__ __forceinline__ void conv_mma(const float* As, const float* Bs, f32x4 (&acc)[2][2],
                                         int w, int l) {
  const int lm = l & 15, lg = l >> 4;
  const float* ap = As + ((w >> 1) * 32 + lm) * LD + lg;
  const float* bp = Bs + ((w & 1) * 32 + lm) * LD + lg;
#pragma unroll
  for (int kk = 0; kk < kConvChunk / 4; ++kk) {
    const float a0 = ap[kk * 4], a1 = ap[16 * LD + kk * 4];
    const float b0 = bp[kk * 4], b1 = bp[16 * LD + kk * 4];
    acc[0][0] = mfma4(a0, b0, acc[0][0]);
    acc[0][1] = mfma4(a0, b1, acc[0][1]);
    acc[1][0] = mfma4(a1, b0, acc[1][0]);
    acc[1][1] = mfma4(a1, b1, acc[1][1]);
  }
}

// tile row of accumulator element e of acc[i][.], tile column of acc[.][j]
__device__ __forceinline__ int acc_row(int w, int l, int i, int e) {
  return (w >> 1) * 32 + i * 16 + (l >> 4) * 4 + e;
}
__device__ __forceinline__ int acc_col(int w, int l, int j) { return (w & 1) * 32 + j * 16 + (l & 15); }

// (ci, ky, kx) of a patch column, advanced by 4 (one step per wave of the
// staging map) without a division
struct KPos { int c, y, x; };
__device__ __forceinline__ void kpos_step4(KPos& q, int ny, int nx) {
  q.x += 4;
  while (q.x >= nx) { q.x -= nx; ++q.y; }
  while (q.y >= ny) { q.y -= ny; ++q.c; }
}

}  // namespace

// ------------------------------------------------------------------ forward
// staging maps: A (weights) element j of thread tid: VW ? row (tid >> 3) + 32 (j >> 2),
// z 4 (tid & 7) + (j & 3) : row (tid >> 5) + 8 j, z tid & 31;  B (patches): row
// tid & 63 (the thread's output pixel), z (tid >> 6) + 4 j (uniform in a wave)
//
// ROWS (uint8 input only): image nn is not at x + nn cin h w but where the
// learners' time-major row map puts it (pix_of: pix[b][t] | pix_next[b], 64-bit
// bases, element alignment); the base is all that changes.
// skip: device stop flag, read once per workgroup before any other load.
template <typename T, bool VW, bool ROWS>
__global__ void __launch_bounds__(kWG)
conv_fwd_kernel(const T* __restrict__ x, const float* __restrict__ wgt, const float* __restrict__ bias,
                float* __restrict__ y, ConvGeom g, int64_t n, int act, int div255, PixRows pr,
                const int* skip) {
  if (skip && skip[0] != 0) return;
  __shared__ __attribute__((aligned(16))) float As[kConvTile * LD];
  __shared__ __attribute__((aligned(16))) float Bs[kConvTile * LD];
  const int tid = threadIdx.x, l = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t NP = n * g.P;
  const int rT = (g.cout + kConvTile - 1) / kConvTile;
  const int64_t tiles = ((NP + kConvTile - 1) / kConvTile) * rT;
  const int kk2 = g.k * g.k, HW = g.h * g.w;

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
    const T* xb;
    if constexpr (ROWS) xb = pix_of(pr, nn);
    else xb = x + nn * (int64_t)g.cin * HW;
    KPos kp;
    kp.c = w / kk2;
    kp.y = (w - kp.c * kk2) / g.k;
    kp.x = w - kp.c * kk2 - kp.y * g.k;
    int kcur = w;

    float pa[NJ], pb[NJ];
    auto fetch = [&](int z0) {
      if constexpr (VW) {
        const int zz = z0 + 4 * (tid & 7);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int co = r0 + (tid >> 3) + 32 * h;
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (co < g.cout && zz < g.K)        // K % 4 == 0: the four are in or out together
            v = *reinterpret_cast<const float4*>(wgt + (int64_t)co * g.K + zz);
          pa[4 * h] = v.x; pa[4 * h + 1] = v.y; pa[4 * h + 2] = v.z; pa[4 * h + 3] = v.w;
        }
      } else {
        const int zz = z0 + (tid & 31);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int co = r0 + (tid >> 5) + 8 * j;
          pa[j] = (co < g.cout && zz < g.K) ? wgt[(int64_t)co * g.K + zz] : 0.f;
        }
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int iy = iy0 + kp.y, ix = ix0 + kp.x;
        const bool ok = qok && kcur < g.K && iy >= 0 && iy < g.h && ix >= 0 && ix < g.w;
        pb[j] = ok ? ldf(xb + kp.c * HW + iy * g.w + ix) : 0.f;
        kpos_step4(kp, g.k, g.k);
        kcur += 4;
      }
    };
    auto stage = [&]() {
      if constexpr (VW) {
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          As[((tid >> 3) + 32 * (j >> 2)) * LD + 4 * (tid & 7) + (j & 3)] = pa[j];
      } else {
#pragma unroll
        for (int j = 0; j < NJ; ++j) As[((tid >> 5) + 8 * j) * LD + (tid & 31)] = pa[j];
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) Bs[l * LD + w + 4 * j] = pb[j];
    };

    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    fetch(0);
    for (int z0 = 0; z0 < g.K; z0 += kConvChunk) {
      stage();
      __syncthreads();
      if (z0 + kConvChunk < g.K) fetch(z0 + kConvChunk);
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
// blockIdx.y = ry * s + rx.  Staging maps: A (taps of w) row (tid >> 5) + 8 j
// (input channel), z tid & 31;  B (dy) row tid & 63 (the thread's input pixel
// of the class), z (tid >> 6) + 4 j = (co, ay, ax), uniform in a wave
__global__ void __launch_bounds__(kWG)
conv_dx_kernel(const float* __restrict__ dy, const float* __restrict__ wgt,
               const float* __restrict__ mask, float* __restrict__ dx, ConvGeom g, int64_t n,
               const int* skip) {
  if (skip && skip[0] != 0) return;
  __shared__ __attribute__((aligned(16))) float As[kConvTile * LD];
  __shared__ __attribute__((aligned(16))) float Bs[kConvTile * LD];
  const int tid = threadIdx.x, l = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ry = blockIdx.y / g.s, rx = blockIdx.y - ry * g.s;
  const int fy = conv_class_first(ry, g.s, g.p), fx = conv_class_first(rx, g.s, g.p);
  const int ny = conv_class_count(g.h, ry, g.s, g.p), nx = conv_class_count(g.w, rx, g.s, g.p);
  const int ty = conv_class_taps(g.k, ry, g.s), tx = conv_class_taps(g.k, rx, g.s);
  const int64_t Qc = n * ny * nx;
  if (Qc == 0) return;                                   // (uniform in the workgroup)
  const int txy = ty * tx, Z = g.cout * txy, nyx = ny * nx;
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
    KPos kp;
    kp.c = w / txy;
    kp.y = (w - kp.c * txy) / tx;
    kp.x = w - kp.c * txy - kp.y * tx;
    int zcur = w;

    float pa[NJ], pb[NJ];
    auto fetch = [&](int z0) {
      const int z = z0 + (tid & 31);
      const int co = z / txy, r = z - co * txy;
      const int ay = r / tx, ax = r - ay * tx;
      const int wo_ = (ry + g.s * ay) * g.k + rx + g.s * ax;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int ci = r0 + (tid >> 5) + 8 * j;
        pa[j] = (ci < g.cin && z < Z) ? wgt[((int64_t)co * g.cin + ci) * (g.k * g.k) + wo_] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int oy = oyb - kp.y, ox = oxb - kp.x;
        const bool ok = qok && zcur < Z && oy >= 0 && oy < g.ho && ox >= 0 && ox < g.wo;
        pb[j] = ok ? dyb[(int64_t)kp.c * g.P + oy * g.wo + ox] : 0.f;
        kpos_step4(kp, ty, tx);
        zcur += 4;
      }
    };

    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    fetch(0);
    for (int z0 = 0; z0 < Z; z0 += kConvChunk) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) As[((tid >> 5) + 8 * j) * LD + (tid & 31)] = pa[j];
#pragma unroll
      for (int j = 0; j < NJ; ++j) Bs[l * LD + w + 4 * j] = pb[j];
      __syncthreads();
      if (z0 + kConvChunk < Z) fetch(z0 + kConvChunk);
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
// Staging maps: both operands row (tid >> 5) + 8 j, pixel (z) tid & 31: the
// thread's 8 patch columns are fixed for the whole kernel, its pixel moves.
// ROWS, skip: as in conv_fwd_kernel.
template <typename T, bool ROWS>
__global__ void __launch_bounds__(kWG)
conv_dw_kernel(const float* __restrict__ dy, const T* __restrict__ x, float* __restrict__ part,
               ConvGeom g, int64_t n, ConvDwPlan pl, PixRows pr, const int* skip) {
  if (skip && skip[0] != 0) return;
  __shared__ __attribute__((aligned(16))) float As[kConvTile * LD];
  __shared__ __attribute__((aligned(16))) float Bs[kConvTile * LD];
  const int tid = threadIdx.x, l = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t NP = n * g.P;
  const int rT = (g.cout + kConvTile - 1) / kConvTile;
  const int r0 = (int)(blockIdx.x % rT) * kConvTile, k0 = (int)(blockIdx.x / rT) * kConvTile;
  const int kk2 = g.k * g.k, HW = g.h * g.w;
  int koff[NJ], kyx[NJ];                 // ci H W + ky W + kx;  ky | kx << 4, -1: no such column
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int kc = k0 + (tid >> 5) + 8 * j;
    const int ci = kc / kk2, r = kc - ci * kk2;
    const int ky = r / g.k, kx = r - ky * g.k;
    koff[j] = ci * HW + ky * g.w + kx;
    kyx[j] = kc < g.K ? (ky | (kx << 4)) : -1;
  }
  const int64_t c_begin = (int64_t)blockIdx.y * pl.per;
  const int64_t c_end = c_begin + pl.per < pl.chunks ? c_begin + pl.per : pl.chunks;

  float pa[NJ], pb[NJ];
  auto fetch = [&](int64_t c) {
    const int64_t m = c * kConvChunk + (tid & 31);
    const bool mok = m < NP;
    const int64_t nn = mok ? m / g.P : 0;
    const int pp = mok ? (int)(m - nn * g.P) : 0;
    const int oy = pp / g.wo, ox = pp - oy * g.wo;
    const int iy0 = oy * g.s - g.p, ix0 = ox * g.s - g.p;
    const float* dyb = dy + nn * (int64_t)g.cout * g.P + pp;
    const T* xb;
    if constexpr (ROWS) xb = pix_of(pr, nn) + iy0 * g.w + ix0;
    else xb = x + nn * (int64_t)g.cin * HW + iy0 * g.w + ix0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int co = r0 + (tid >> 5) + 8 * j;
      pa[j] = (mok && co < g.cout) ? dyb[(int64_t)co * g.P] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int iy = iy0 + (kyx[j] & 15), ix = ix0 + (kyx[j] >> 4);
      const bool ok = mok && kyx[j] >= 0 && iy >= 0 && iy < g.h && ix >= 0 && ix < g.w;
      pb[j] = ok ? ldf(xb + koff[j]) : 0.f;
    }
  };

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dbs = 0.f;
  if (c_begin < c_end) fetch(c_begin);
  for (int64_t c = c_begin; c < c_end; ++c) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) As[((tid >> 5) + 8 * j) * LD + (tid & 31)] = pa[j];
#pragma unroll
    for (int j = 0; j < NJ; ++j) Bs[((tid >> 5) + 8 * j) * LD + (tid & 31)] = pb[j];
    __syncthreads();
    if (c + 1 < c_end) fetch(c + 1);
    conv_mma(As, Bs, acc, w, l);
    if (k0 == 0 && tid < kConvTile) {
#pragma unroll
      for (int z = 0; z < kConvChunk; ++z) dbs += As[tid * LD + z];
    }
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
  if (k0 == 0 && tid < kConvTile && r0 + tid < g.cout) out[(int64_t)g.cout * g.K + r0 + tid] = dbs;
}

// dw[i] = sum of the partials in a fixed order (/ 255 for dW when the patches
// were unscaled); the last cout entries of a slab are db.  A workgroup owns 64
// consecutive elements: wave w adds splits w, w + 4, ... in that order (four
// independent load streams per element instead of one serial chain over up to
// 256 partials), then the four wave sums are added 0 + 1 + 2 + 3.
__global__ void __launch_bounds__(kWG)
conv_dw_reduce(const float* __restrict__ part, int splits, int64_t slab, int64_t nw,
               float* __restrict__ dw, float* __restrict__ db, int div255, const int* skip) {
  if (skip && skip[0] != 0) return;
  __shared__ float red[kNW][64];
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int64_t i0 = (int64_t)blockIdx.x * 64; i0 < slab; i0 += (int64_t)gridDim.x * 64) {
    const int64_t i = i0 + l;
    float s = 0.f;
    if (i < slab)
      for (int sp = w; sp < splits; sp += kNW) s += part[(int64_t)sp * slab + i];
    red[w][l] = s;
    __syncthreads();
    if (w == 0 && i < slab) {
      const float t = ((red[0][l] + red[1][l]) + red[2][l]) + red[3][l];
      if (i < nw) dw[i] = div255 ? t / 255.0f : t;
      else db[i - nw] = t;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------- host
// rows (non-null: x is ignored, the uint8 images are those of the row map) and
// skip are the kernels' ROWS form and stop flag
int conv2d_forward(const void* x, int x_u8, int div255, int64_t n, const ConvGeom& g,
                   const float* wgt, const float* bias, int act, float* y, hipStream_t st,
                   const int* skip, const PixRows* rows) {
  if (n < 1) return SMI_OK;
  const bool vw = g.K % 4 == 0 && (reinterpret_cast<uintptr_t>(wgt) & 15) == 0;
  const int64_t tiles = conv_fwd_tiles(g, n);
  const double flops = 2.0 * (double)n * g.P * g.K * g.cout;
  const PixRows pr = rows ? *rows : PixRows{nullptr, nullptr, 1, 1, 0};
  const int kt = ktime_begin(st);
#define SMI_CONV_FWD(T, VW, ROWS)                                                                \
  do {                                                                                           \
    auto k = conv_fwd_kernel<T, VW, ROWS>;                                                       \
    const int64_t rg = resident_grid(k, kWG, 0);                                                 \
    hipLaunchKernelGGL(k, dim3((unsigned)(tiles < rg ? tiles : rg)), dim3(kWG), 0, st,           \
                       static_cast<const T*>(x), wgt, bias, y, g, n, act, div255, pr, skip);     \
  } while (0)
  if (rows) { if (vw) SMI_CONV_FWD(unsigned char, true, true); else SMI_CONV_FWD(unsigned char, false, true); }
  else if (x_u8) { if (vw) SMI_CONV_FWD(unsigned char, true, false); else SMI_CONV_FWD(unsigned char, false, false); }
  else { if (vw) SMI_CONV_FWD(float, true, false); else SMI_CONV_FWD(float, false, false); }
#undef SMI_CONV_FWD
  ktime_end(kt, KT_CNN_FWD, flops, st);
  return check_launch("conv_fwd_kernel");
}

int conv2d_backward_input(const float* dy, int64_t n, const ConvGeom& g, const float* wgt,
                          const float* mask, float* dx, hipStream_t st, const int* skip) {
  if (n < 1) return SMI_OK;
  const int64_t tiles = conv_dx_max_tiles(g, n);
  const int64_t rg = resident_grid(conv_dx_kernel, kWG, 0);
  const int64_t per = (rg + g.s * g.s - 1) / (g.s * g.s);          // resident workgroups per class
  const int kt = ktime_begin(st);
  hipLaunchKernelGGL(conv_dx_kernel, dim3((unsigned)(tiles < per ? tiles : per), g.s * g.s), dim3(kWG),
                     0, st, dy, wgt, mask, dx, g, n, skip);
  ktime_end(kt, KT_CNN_BWD, 2.0 * (double)n * g.P * g.K * g.cout, st);
  return check_launch("conv_dx_kernel");
}

int conv2d_backward_weight(const float* dy, const void* x, int x_u8, int div255, int64_t n,
                           const ConvGeom& g, float* dw, float* db, float* part, hipStream_t st,
                           const int* skip, const PixRows* rows) {
  if (n < 1) return SMI_OK;
  const ConvDwPlan pl = conv_dw_plan(g, n);
  const PixRows pr = rows ? *rows : PixRows{nullptr, nullptr, 1, 1, 0};
  const int kt = ktime_begin(st);
  if (rows)
    hipLaunchKernelGGL((conv_dw_kernel<unsigned char, true>), dim3(pl.tiles, pl.splits), dim3(kWG), 0,
                       st, dy, static_cast<const unsigned char*>(nullptr), part, g, n, pl, pr, skip);
  else if (x_u8)
    hipLaunchKernelGGL((conv_dw_kernel<unsigned char, false>), dim3(pl.tiles, pl.splits), dim3(kWG), 0,
                       st, dy, static_cast<const unsigned char*>(x), part, g, n, pl, pr, skip);
  else
    hipLaunchKernelGGL((conv_dw_kernel<float, false>), dim3(pl.tiles, pl.splits), dim3(kWG), 0, st, dy,
                       static_cast<const float*>(x), part, g, n, pl, pr, skip);
  ktime_end(kt, KT_CNN_BWD, 2.0 * (double)n * g.P * g.K * g.cout, st);
  RC_CHECK(check_launch("conv_dw_kernel"));
  const int64_t nb = (pl.slab + 63) / 64;
  hipLaunchKernelGGL(conv_dw_reduce, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(kWG), 0, st, part,
                     pl.splits, pl.slab, (int64_t)g.cout * g.K, dw, db, div255, skip);
  return check_launch("conv_dw_reduce");
}

}  // namespace smi
