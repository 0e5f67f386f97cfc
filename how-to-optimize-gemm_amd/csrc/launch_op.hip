// launch_op.hip -- launches of the transposed-operand forms (mmh_sgemm_op, GemmArgs::ta / tb): the K2W tiles with op forms
// (k2w_tiles, internal.hpp; sgemm_dma5.hpp, OP) as launch_dma5.hpp's OpForm through its launcher, and the naive kernel with
// two index swaps.  A translation unit of its own so that build.py compiles the op instantiations beside launch_dma5.hip's NN ones.
// Part of libmmult_hip.so (see internal.hpp).
#include "launch_dma5.hpp"

namespace mmh {

// K0 for op(A) op(B): A(i, p) at A[i lda + p] (N) or A[p lda + i] (T), B(p, j) at B[p ldb + j] (N) or B[j ldb + p] (T).
// Like sgemm_naive_kernel, one fmaf chain over ascending k per element: the independent reference of tools/fuzz.py --ops.
__global__ void __launch_bounds__(256)
sgemm_naive_op_kernel(int transa, int transb, int m, int n, int k, const float *__restrict__ A, int lda,
                      const float *__restrict__ B, int ldb, float *__restrict__ C, int ldc, int accumulate) {
  const int col = blockIdx.x * 64 + (threadIdx.x & 63);
  const int row = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (row >= m || col >= n) return;
  const size_t a_i = transa ? 1 : (size_t)lda, a_p = transa ? (size_t)lda : 1;
  const size_t b_p = transb ? 1 : (size_t)ldb, b_j = transb ? (size_t)ldb : 1;
  float acc = accumulate ? C[(size_t)row * ldc + col] : 0.0f;
  for (int p = 0; p < k; ++p) acc = __builtin_fmaf(A[row * a_i + p * a_p], B[p * b_p + col * b_j], acc);
  C[(size_t)row * ldc + col] = acc;
}

int launch_dma5_op(mmh_context *ctx, int kernel, const GemmArgs &g) {
  return launch_form<OpForm, 1, 2, 3>(kernel, g, [&](auto f) { return launch_dma5_tile<decltype(f)>(ctx, g); });
}

int launch_naive_op(const GemmArgs &g) {
  dim3 grid((unsigned)((g.n + 63) / 64), (unsigned)((g.m + 3) / 4)), block(256);
  hipLaunchKernelGGL(sgemm_naive_op_kernel, grid, block, 0, g.s, g.ta, g.tb, g.m, g.n, g.k, g.A, g.lda, g.B, g.ldb, g.C, g.ldc, g.acc);
  HIP_TRY(hipGetLastError());
  set_last_launch(std::string("sgemm_naive_op_kernel") + op_tag(g));
  return MMH_OK;
}

// the op kernels' LDS opt-ins (> 64 KiB), so that a first op launch can be captured into a graph like an NN one
int warm_dma5_op() { return warm_form<OpForm, 1, 2, 3>(); }

}  // namespace mmh
