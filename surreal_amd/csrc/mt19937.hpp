// mt19937.hpp — the MT19937 pieces (Matsumoto & Nishimura 1998) shared by the
// CPython-exact samplers: the uniform index draw (sampler_kernels.hip) and the
// prioritized draw (per_kernels.hip).  State: 624 words + position (625 uint32).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace smi {

constexpr int kMtN = 624, kMtM = 397;
constexpr uint32_t kMatA = 0x9908b0dfU, kUpper = 0x80000000U, kLower = 0x7fffffffU;
constexpr int kMtWG = 1024;        // threads of the single sampler workgroup

__host__ __device__ inline uint32_t mt_temper(uint32_t y) {
  y ^= (y >> 11);
  y ^= (y << 7) & 0x9d2c5680U;
  y ^= (y << 15) & 0xefc60000U;
  y ^= (y >> 18);
  return y;
}
__host__ __device__ inline uint32_t mt_mix(uint32_t hi, uint32_t lo, uint32_t far) {
  const uint32_t y = (hi & kUpper) | (lo & kLower);
  return far ^ (y >> 1) ^ ((y & 1U) ? kMatA : 0U);
}

// host: the next tempered word (genrand_uint32), twisting when the position
// has run out (sampler_kernels.hip)
uint32_t mt_next_host(uint32_t* st);

// The 624-word twist by one workgroup of kMtWG threads over the LDS copy `mt`,
// in its three dependency phases ([0,227) from old words, [227,454) and
// [454,623) from freshly twisted words 227 back, then word 623 by thread 0).
// Every thread of the workgroup calls it; the caller resets its position and
// synchronises before the new words are read.
__device__ __forceinline__ void mt_twist_wg(uint32_t* mt, int tid) {
  // phase 1: [0, 227) from old words
  uint32_t nv = 0;
  if (tid < kMtN - kMtM) nv = mt_mix(mt[tid], mt[tid + 1], mt[tid + kMtM]);
  __syncthreads();
  if (tid < kMtN - kMtM) mt[tid] = nv;
  __syncthreads();
  // phase 2: [227, 454) and phase 3: [454, 623) read words 227 back
  for (int base = kMtN - kMtM; base < kMtN - 1; base += kMtN - kMtM) {
    const int kk = base + tid;
    const int end = (base + (kMtN - kMtM) < kMtN - 1) ? base + (kMtN - kMtM) : kMtN - 1;
    nv = 0;
    if (kk < end) nv = mt_mix(mt[kk], mt[kk + 1], mt[kk + (kMtM - kMtN)]);
    __syncthreads();
    if (kk < end) mt[kk] = nv;
    __syncthreads();
  }
  if (tid == 0) mt[kMtN - 1] = mt_mix(mt[kMtN - 1], mt[0], mt[kMtM - 1]);
}

}  // namespace smi
