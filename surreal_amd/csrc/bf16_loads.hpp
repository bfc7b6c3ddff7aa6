// bf16_loads.hpp — the global loads of the bf16 GEMM units
// (linear_bf16_kernels.hip, noisy_bf16_kernels.hip) into fp32 prefetch
// registers.  Every load has a clamped address and its value is zeroed
// afterwards by a select: no predicated loads, and padding never enters a sum
// as anything but +0.  `vec` (16-byte loads) is decided once per launch and
// operand by the caller.
#pragma once
#include "smi_device.hpp"

namespace smi {

// v[0..7] = P[row][z .. z + 7] of a z-contiguous operand with `rows` rows and
// reduction range [.., ze); rows past the end and z >= ze read as zero
__device__ __forceinline__ void load_z8(const float* __restrict__ P, int64_t ld, int row, int rows,
                                        int z, int ze, bool vec, float* v) {
  const bool rok = row < rows;
  const float* pr = P + (int64_t)(rok ? row : rows - 1) * ld;
  if (vec) {                               // ze % 4 == 0: a quad is in or out as a whole
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int zz = z + 4 * q;
      const float4 x = *reinterpret_cast<const float4*>(pr + (zz < ze ? zz : ze - 4));
      const bool ok = rok && zz < ze;
      v[4 * q] = ok ? x.x : 0.f; v[4 * q + 1] = ok ? x.y : 0.f;
      v[4 * q + 2] = ok ? x.z : 0.f; v[4 * q + 3] = ok ? x.w : 0.f;
    }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int zz = z + e;
      const float x = pr[zz < ze ? zz : ze - 1];
      v[e] = (rok && zz < ze) ? x : 0.f;
    }
  }
}

// v[4 e + c] = P[z + e][j + c], e < 8, c < 4, of an operand whose rows are the
// reduction (W in the input gradient): J columns, reduction range [.., ze)
__device__ __forceinline__ void load_t4x8(const float* __restrict__ P, int64_t ld, int z, int ze,
                                          int j, int J, bool vec, float* v) {
  if (vec) {                               // J % 4 == 0
    const int jc = j < J ? j : J - 4;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int zz = z + e;
      const float4 x = *reinterpret_cast<const float4*>(P + (int64_t)(zz < ze ? zz : ze - 1) * ld + jc);
      const bool ok = zz < ze && j < J;
      v[4 * e] = ok ? x.x : 0.f; v[4 * e + 1] = ok ? x.y : 0.f;
      v[4 * e + 2] = ok ? x.z : 0.f; v[4 * e + 3] = ok ? x.w : 0.f;
    }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int zz = z + e;
      const float* pr = P + (int64_t)(zz < ze ? zz : ze - 1) * ld;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float x = pr[j + c < J ? j + c : J - 1];
        v[4 * e + c] = (zz < ze && j + c < J) ? x : 0.f;
      }
    }
  }
}

}  // namespace smi
