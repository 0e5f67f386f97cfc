// quant_rules_s8.hpp -- symmetric int8 quantisation, per element: which elements take part in the abs-max, the scale of a
// maximum, the rounding.  No kernel: shared by the per-tensor passes (quant_s8.hpp, whose header has the contract) and the
// per-row passes of the int8 linear layer (csrc_q8/quant_rows_s8.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mmh {

typedef float qf32x4 __attribute__((ext_vector_type(4)));
typedef int qi32x4 __attribute__((ext_vector_type(4)));

// |x| for the abs-max: non-finite elements do not take part (NaN never wins an fmaxf; inf is dropped)
__device__ __forceinline__ float finite_abs(float x) {
  const float a = fabsf(x);
  return a <= 3.402823466e+38f ? a : 0.0f;
}
__device__ __forceinline__ float abs4(qf32x4 v) {
  return fmaxf(fmaxf(finite_abs(v[0]), finite_abs(v[1])), fmaxf(finite_abs(v[2]), finite_abs(v[3])));
}

// 127 / max|x| over the finite elements; 1 when that maximum is 0; clamped to FLT_MAX where the quotient overflows
__device__ __forceinline__ float scale_of_amax(float amax) {
  if (!(amax > 0.0f)) return 1.0f;
  const float s = 127.0f / amax;
  return s <= 3.402823466e+38f ? s : 3.402823466e+38f;
}

__device__ __forceinline__ int quantize_one(float x, float scale) {
  const float y = x == x ? x * scale : 0.0f;   // NaN -> 0 (0 * inf cannot occur: scale is finite)
  return (int)fminf(fmaxf(rintf(y), -127.0f), 127.0f);
}

// one dword of four int8 per float4 (q 4-byte aligned and ldq % 4 == 0)
__device__ __forceinline__ unsigned quantize4(qf32x4 v, float scale) {
  return (unsigned)(quantize_one(v[0], scale) & 255) | ((unsigned)(quantize_one(v[1], scale) & 255) << 8) |
         ((unsigned)(quantize_one(v[2], scale) & 255) << 16) | ((unsigned)(quantize_one(v[3], scale) & 255) << 24);
}

}  // namespace mmh
