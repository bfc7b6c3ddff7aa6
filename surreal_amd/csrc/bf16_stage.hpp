// bf16_stage.hpp — what the bf16 MFMA units (conv_bf16_kernels.hip,
// linear_bf16_kernels.hip) share: the rounding of fp32 prefetch registers into
// the 16-byte LDS vectors of 8 bf16, and the v_mfma_f32_16x16x32_bf16 wrapper.
// fp32 -> bf16 is round-to-nearest-even (v_cvt_pk_bf16_f32: NaN stays NaN,
// +-inf and -0.0 keep their bits).
//
// Operand map of the instruction: lane (i = l & 15, g = l >> 4) holds
// A[i][8 g .. 8 g + 7] and B[8 g .. 8 g + 7][j = i]; D[row = 4 g + e][col = i]
// (the output map of the fp32 16x16x4 MFMA).
#pragma once
#include "smi_device.hpp"

namespace smi {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// 8 fp32 -> 8 bf16 (round to nearest even), element 0 in the low half of .x
__device__ __forceinline__ uint4 pack8(const float* v) {
  uint32_t u[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bf16x2 h = {(__bf16)v[2 * i], (__bf16)v[2 * i + 1]};
    u[i] = __builtin_bit_cast(uint32_t, h);
  }
  return make_uint4(u[0], u[1], u[2], u[3]);
}

__device__ __forceinline__ f32x4 mfma32(const uint4& a, const uint4& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a),
                                                 __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

}  // namespace smi
