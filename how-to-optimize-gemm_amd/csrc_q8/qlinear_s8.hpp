// qlinear_s8.hpp -- the GEMM of libmmult_hip_q8.so, the int8 linear layer (include/mmult_hip_q8.h has the contract,
// tests/qlinear_ref.py restates it in numpy, tests/test_gpu_qlinear.py holds every instantiation to it bit for bit):
//   qlinear_s8_kernel<BM,BN,TM,EDGE,BIAS,RELU>   igemm_s8_dma_tile (csrc/igemm_s8.hpp, K3t: both operands by LDS-DMA, B
//                                   gathered by the transposing LDS read) with the layer's epilogue behind its C transposer
// The activations' rows and the weight image come from quant_rows_s8.hpp's kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "igemm_s8.hpp"

namespace mmh {

// ---- the GEMM --------------------------------------------------------------------------------------------------------------
// The layer's epilogue behind igemm_s8_dma_tile's C transposer, where a lane holds four consecutive columns of one row:
//   y = act(fl(fl(fl((float)acc * rx[row]) * rw[col]) + bias[col]))
// three roundings, nothing contracted; no bias: no add; ReLU as mmh_sgemm_ex's (> 0 or NaN stays, -0 and negatives give +0).
// The column factors and biases are loaded once per tile, one row factor per row vector; a guarded instantiation reads
// none of rx, rw, bias at or beyond m / n.
template <bool EDGE, bool BIAS, bool RELU>
struct QlinearEpilogue {
  static constexpr bool kFused = true;
  const float *rx, *rw, *bias;
  float cw[4], cb[4];
  __device__ __forceinline__ void columns(int col, int n, bool whole) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool in = !EDGE || whole || col + u < n;
      cw[u] = in ? rw[col + u] : 0.0f;
      cb[u] = BIAS && in ? bias[col + u] : 0.0f;
    }
  }
  __device__ __forceinline__ i32x4 row(i32x4 v, int row, int m, bool whole) const {
#pragma clang fp contract(off)
    const float r = (!EDGE || whole || row < m) ? rx[row] : 0.0f;
    typedef float f32x4_t __attribute__((ext_vector_type(4)));
    f32x4_t f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      // plain operators under the pragma: each line rounds once (__fmul_rn / __fadd_rn are inline functions compiled
      // under their own contraction mode: inlined here, their product and sum were fused)
      float y = (float)v[u] * r;
      y = y * cw[u];
      if (BIAS) y = y + cb[u];
      if (RELU) y = !(y <= 0.0f) ? y : 0.0f;   // (NaN: not <= 0, stays)
      f[u] = y;
    }
    return __builtin_bit_cast(i32x4, f);
  }
};

// m x n = rows x out, k = in; xq: the activations' int8 rows (pitch ldq), wq: the weight image (in x pitch_n), read in place as B
template <int BM, int BN, int TM, bool EDGE, bool BIAS, bool RELU>
__global__ void __launch_bounds__(BM / (16 * TM) * (BN / 64) * 64, (BM == 128 && BN == 128) ? 2 : 1)
qlinear_s8_kernel(int m, int n, int k, const int8_t *__restrict__ xq, int ldq, const int8_t *__restrict__ wq, int pitch_n,
                  const float *__restrict__ rx, const float *__restrict__ rw, const float *__restrict__ bias,
                  float *__restrict__ y, int ldy, int nbm, int nbn) {
  QlinearEpilogue<EDGE, BIAS, RELU> ep{rx, rw, bias};
  igemm_s8_dma_tile<BM, BN, TM, EDGE, 0, true>(m, n, k, xq, ldq, wq, pitch_n, n, reinterpret_cast<int32_t *>(y), ldy, 0, nbm, nbn,
                                               nullptr, ep);
}

}  // namespace mmh
