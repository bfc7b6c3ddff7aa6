// philox.hpp — Philox4x32-10 (Salmon et al. 2011), the stateless counter-based
// generator of the device draws: the quantile fractions of dqn_iqn_kernels.hip
// (word 0) and the factorised noise of noisy_kernels.hip (words 0 and 1).
// key = {k0, k1}, counter = {c0, c1, c2, c3}; the ten rounds below are the
// reference's, so a host restatement (tests/iqn_ref.py) gives the same words.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace smi {

// word 0 of the output block
__device__ __forceinline__ uint32_t iqn_philox(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1,
                                               uint32_t c2, uint32_t c3) {
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}

// words 0 and 1 of the same block (the same rounds; w0 == iqn_philox(...)).  Kept
// as a second copy of the rounds: with both on one shared core the IQN unit's
// gfx950 code came out with two instructions in another order, and that unit's
// code is to stay exactly as it was.
__device__ __forceinline__ void philox_w01(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1,
                                           uint32_t c2, uint32_t c3, uint32_t& w0, uint32_t& w1) {
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  w0 = c0; w1 = c1;
}

}  // namespace smi
