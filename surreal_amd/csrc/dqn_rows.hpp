// dqn_rows.hpp — per-row helpers shared by dqn_kernels.hip (scalar heads),
// dqn_dist_kernels.hip (categorical heads), dqn_quant_kernels.hip (quantile
// heads) and dqn_iqn_kernels.hip (implicit quantile heads): the action index, the staging of one row's A N head outputs in LDS,
// the wave-scope LDS ordering and lane broadcast, the dueling mean over the
// actions, and the host rules both distributional launchers follow (the
// staging form, the rows of a workgroup).  The statistics launch the two
// distributional units share is launch_dqn_dist_stats (dqn_dist_kernels.hip).
#pragma once
#include <math.h>
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace smi {

// the action column's float as an index into [0, A): an action value outside
// the range is a caller error and is clamped into it (NaN -> 0, fractions
// truncated), so nothing outside the A actions is read or written
__device__ __forceinline__ int dqn_action_index(float af, int A) {
  if (!(af >= 0.f)) return 0;                     // negative or NaN
  return af < (float)A ? (int)af : A - 1;
}

// LDS traffic between the lanes of ONE wave: order the wave's own accesses
__device__ __forceinline__ void dqn_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// lane j's value in every lane; j is wave uniform (a v_readlane)
__device__ __forceinline__ float dqn_lane(float v, int j) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}

// one row's AN head outputs into an LDS slab by the NT threads of a team (a
// wave: NT = 64, t the lane; a workgroup: NT = its size, t the thread); the
// loads of a thread are issued 4 at a time before their LDS stores.  vec: 16
// byte loads (src 16-byte aligned) and dwords for the last AN % 4 outputs;
// otherwise dwords throughout.  The caller orders the team around the copy
// (dqn_wave_sync / __syncthreads before and after).
template <int NT>
__device__ __forceinline__ void dqn_copy_slab(const float* __restrict__ src, int AN, int vec,
                                              float* __restrict__ slab, int t) {
  int done = 0;
  if (vec) {
    const int n4 = AN >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(slab);
    for (int base = 0; base < n4; base += 4 * NT) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = base + u * NT + t;
        v[u] = e < n4 ? s4[e] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = base + u * NT + t;
        if (e < n4) d4[e] = v[u];
      }
    }
    done = n4 << 2;                              // the last AN % 4 outputs follow as dwords
  }
  for (int base = done; base < AN; base += 4 * NT) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = base + u * NT + t;
      v[u] = e < AN ? src[e] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = base + u * NT + t;
      if (e < AN) slab[e] = v[u];
    }
  }
}

// mean over the actions of column i (atom / quantile) of a staged slab, summed
// left to right (0 without dueling and past the last column)
template <bool DUELING>
__device__ __forceinline__ float dqn_col_mean(const float* __restrict__ slab, int A, int N, int i) {
#pragma clang fp contract(off)
  if (!DUELING || i >= N) return 0.f;
  float s = slab[i];
  for (int a = 1; a < A; ++a) s = s + slab[a * N + i];
  return s / (float)A;
}

// the quantile pair loss of dqn_quant_kernels.hip and dqn_iqn_kernels.hip (the
// specification: the former's header): one online quantile's sums over the N
// targets, j ascending; tj(j) is T_j in every lane (a readlane or an LDS
// broadcast); tau is the online quantile's fraction
constexpr int kQrRun = 8;                        // targets summed in fp32 before the fp64 add
struct QrSums { float S, G; };
template <bool HUBER, typename TJ>
__device__ __forceinline__ QrSums qr_pairs(float th, float tau, float kappa, int N, TJ tj) {
#pragma clang fp contract(off)
  const float omt = 1.f - tau, hk = 0.5f * kappa, nk = -kappa;
  double Sd = 0.0, Gd = 0.0;
  for (int j0 = 0; j0 < N; j0 += kQrRun) {
    const int j1 = j0 + kQrRun < N ? j0 + kQrRun : N;
    float s = 0.f, g = 0.f;
    for (int j = j0; j < j1; ++j) {
      const float u = tj(j) - th;
      const float c = u < 0.f ? omt : tau;
      const float au = fabsf(u);
      if (HUBER) {
        const float h = au <= kappa ? 0.5f * (u * u) : kappa * (au - hk);
        const float k = u < nk ? nk : (u > kappa ? kappa : u);
        s = s + c * h;
        g = g + c * k;
      } else {
        const float sg = u > 0.f ? 1.f : (u < 0.f ? -1.f : u);   // 0 and NaN stay
        s = s + c * au;
        g = g + c * sg;
      }
    }
    Sd += (double)s;
    Gd += (double)g;
  }
  float S = (float)Sd, G = (float)Gd;
  if (HUBER) { S = S / kappa; G = G / kappa; }
  return {S, G};
}

// ------------------------------------------------------------------- host
constexpr int kDistBlocksPerCU = 4;              // row blocks aimed at per CU

inline int dqn_cus() {
  int dev = 0, cus = 256;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  return cus < 1 ? 1 : cus;
}

// rows of one workgroup's block in the wave-per-row forms: the quads of 4 rows
// dealt evenly to kDistBlocksPerCU blocks per CU (from B and the CU count only,
// so the statistics partials have one fixed owner per slot)
inline int64_t dqn_rows_per_block(int64_t B, int cus) {
  const int64_t quads = (B + 3) / 4, blocks = (int64_t)kDistBlocksPerCU * cus;
  return 4 * ((quads + blocks - 1) / blocks);
}

// a slab the 16-byte staging may read: 16-byte aligned base, ld % 4 == 0 (a
// NULL slab, one the form does not read, has no say)
inline bool dqn_aligned16(const void* p, int64_t ld) {
  return !p || ((reinterpret_cast<uintptr_t>(p) & 15) == 0 && (ld & 3) == 0);
}

}  // namespace smi
