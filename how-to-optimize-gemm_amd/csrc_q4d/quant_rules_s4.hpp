// quant_rules_s4.hpp -- symmetric 4-bit quantisation, per element: csrc/quant_rules_s8.hpp's rules with 7 for 127 (which
// elements take part in the abs-max is its finite_abs, unchanged).  include/mmult_hip_q4d.h has the contract, tests/q4_ref.py
// the numpy restatement.
#pragma once
#include <hip/hip_runtime.h>

#include "quant_rules_s8.hpp"   // finite_abs

namespace mmh {

// 7 / max|x| over the finite elements; 1 when that maximum is 0; clamped to FLT_MAX where the quotient overflows
__device__ __forceinline__ float scale4_of_amax(float amax) {
  if (!(amax > 0.0f)) return 1.0f;
  const float s = 7.0f / amax;
  return s <= 3.402823466e+38f ? s : 3.402823466e+38f;
}

// -7 .. 7, never -8; NaN -> 0, +-inf -> +-7
__device__ __forceinline__ int quantize4_one(float x, float scale) {
  const float y = x == x ? x * scale : 0.0f;   // NaN -> 0 (0 * inf cannot occur: scale is finite)
  return (int)fminf(fmaxf(rintf(y), -7.0f), 7.0f);
}

}  // namespace mmh
