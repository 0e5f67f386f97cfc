// launch_batched.hip -- launches of mmh_sgemm_batched's one-launch form: the K2W tiles with op forms (k2w_tiles,
// internal.hpp; sgemm_dma5.hpp, sgemm_mfma_dma5_batched_kernel) over batch x tiles, whole-tile and guarded, every op pair,
// as launch_dma5.hpp's launch_batched_tile on a BatchedForm; and the naive batched kernel, through launch_naive_chunks.  A
// translation unit of its own, like launch_op.hip, so that build.py compiles its 24 instantiations in parallel.  Part of
// libmmult_hip.so (see internal.hpp).
#include "launch_dma5.hpp"

namespace mmh {

// K0 batched: sgemm_naive_op_kernel with the matrix in blockIdx.z (+ z0 of the launch's chunk).  One fmaf chain over
// ascending k per element: the independent reference of tools/fuzz.py --batched.  k == 0 writes 0 (or leaves C) and
// reads neither A nor B.
__global__ void __launch_bounds__(256)
sgemm_naive_batched_kernel(int transa, int transb, int m, int n, int k, const float *__restrict__ A, int lda, long long sA,
                           const float *__restrict__ B, int ldb, long long sB, float *__restrict__ C, int ldc, long long sC,
                           int accumulate) {
  const int col = blockIdx.x * 64 + (threadIdx.x & 63);
  const int row = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (row >= m || col >= n) return;
  A += (long long)blockIdx.z * sA;
  B += (long long)blockIdx.z * sB;
  C += (long long)blockIdx.z * sC;
  const size_t a_i = transa ? 1 : (size_t)lda, a_p = transa ? (size_t)lda : 1;
  const size_t b_p = transb ? 1 : (size_t)ldb, b_j = transb ? (size_t)ldb : 1;
  float acc = accumulate ? C[(size_t)row * ldc + col] : 0.0f;
  for (int p = 0; p < k; ++p) acc = __builtin_fmaf(A[row * a_i + p * a_p], B[p * b_p + col * b_j], acc);
  C[(size_t)row * ldc + col] = acc;
}

int launch_dma5_batched(mmh_context *ctx, int kernel, const GemmArgs &g, const BatchArgs &b) {
  return launch_form<BatchedForm, 0, 1, 2, 3>(kernel, g, [&](auto f) { return launch_batched_tile<decltype(f)>(ctx, g, b); });
}

int launch_naive_batched(const GemmArgs &g, const BatchArgs &b) {
  return launch_naive_chunks(g, b, std::string("sgemm_naive_batched_kernel") + op_tag(g),
                             [&](dim3 grid, const float *A, const float *B, float *C, long) {
    hipLaunchKernelGGL(sgemm_naive_batched_kernel, grid, dim3(256), 0, g.s, g.ta, g.tb, g.m, g.n, g.k, A, g.lda, b.sA, B, g.ldb, b.sB,
                       C, g.ldc, b.sC, g.acc);
  });
}

// the batched kernels' LDS opt-ins (> 64 KiB), so that a first batched launch can be captured into a graph
int warm_dma5_batched() { return warm_form<BatchedForm, 0, 1, 2, 3>(); }

}  // namespace mmh
