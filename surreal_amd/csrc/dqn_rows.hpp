// dqn_rows.hpp — per-row device helpers shared by dqn_kernels.hip (scalar
// heads) and dqn_dist_kernels.hip (categorical heads).
#pragma once

namespace smi {

// the action column's float as an index into [0, A): an action value outside
// the range is a caller error and is clamped into it (NaN -> 0, fractions
// truncated), so nothing outside the A actions is read or written
__device__ __forceinline__ int dqn_action_index(float af, int A) {
  if (!(af >= 0.f)) return 0;                     // negative or NaN
  return af < (float)A ? (int)af : A - 1;
}

}  // namespace smi
