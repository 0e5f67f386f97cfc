// launch_batched_ex.hip -- launches of mmh_sgemm_batched_ex's one-launch form: the K2W tiles with op forms (k2w_tiles,
// internal.hpp; sgemm_dma5.hpp, sgemm_mfma_dma5_batched_ex_kernel) over batch x tiles with the fused epilogue (GemmArgs::ex,
// BatchArgs::sBias), whole-tile and guarded, every op pair, as launch_dma5.hpp's launch_batched_tile on a BatchedExForm; and
// the naive batched kernel with the epilogue written out, through launch_naive_chunks -- the independent reference on the
// device, what MMH_KERNEL_NAIVE runs and what an empty contraction (k == 0) runs.  A translation unit of its own, like
// launch_batched.hip, so that build.py compiles its 24 instantiations beside the others.  Part of libmmult_hip.so.
#include "launch_dma5.hpp"

namespace mmh {

// K0 batched with the epilogue: sgemm_naive_ex_kernel with the matrix in blockIdx.z (+ the launch's chunk, whose pointers the
// launcher advanced).  One fmaf chain from +0 over ascending k per element, then DESIGN.md section 2's epilogue, one rounding
// per operation.  beta == 0: C is not read.  k == 0: A and B are not read.
__global__ void __launch_bounds__(256)
sgemm_naive_batched_ex_kernel(int transa, int transb, int m, int n, int k, const float *__restrict__ A, int lda, long long sA,
                              const float *__restrict__ B, int ldb, long long sB, float *__restrict__ C, int ldc, long long sC,
                              const Dma5Epilogue ep, long long sBias) {
  const int col = blockIdx.x * 64 + (threadIdx.x & 63);
  const int row = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (row >= m || col >= n) return;
  A += (long long)blockIdx.z * sA;
  B += (long long)blockIdx.z * sB;
  C += (long long)blockIdx.z * sC;
  const size_t a_i = transa ? 1 : (size_t)lda, a_p = transa ? (size_t)lda : 1;
  const size_t b_p = transb ? 1 : (size_t)ldb, b_j = transb ? (size_t)ldb : 1;
  float acc = 0.0f;
  for (int p = 0; p < k; ++p) acc = __builtin_fmaf(A[row * a_i + p * a_p], B[p * b_p + col * b_j], acc);
  float v[1] = {acc}, c[1] = {0.0f}, b[1] = {0.0f};
  if (ep.beta != 0.0f) c[0] = C[(size_t)row * ldc + col];
  if (ep.bias_mode == MMH_BIAS_COL) b[0] = ep.bias[(long long)blockIdx.z * sBias + col];
  if (ep.bias_mode == MMH_BIAS_ROW) b[0] = ep.bias[(long long)blockIdx.z * sBias + row];
  dma5_epilogue_apply(ep, v, c, b);
  C[(size_t)row * ldc + col] = v[0];
}

int launch_dma5_batched_ex(mmh_context *ctx, int kernel, const GemmArgs &g, const BatchArgs &b) {
  return launch_form<BatchedExForm, 0, 1, 2, 3>(kernel, g, [&](auto f) { return launch_batched_tile<decltype(f)>(ctx, g, b); });
}

int launch_naive_batched_ex(const GemmArgs &g, const BatchArgs &b) {
  return launch_naive_chunks(g, b, std::string("sgemm_naive_batched_ex_kernel") + ex_tag(g),
                             [&](dim3 grid, const float *A, const float *B, float *C, long b0) {
    const auto [ep, sBias] = ex_chunk_args(g, b, b0);
    hipLaunchKernelGGL(sgemm_naive_batched_ex_kernel, grid, dim3(256), 0, g.s, g.ta, g.tb, g.m, g.n, g.k, A, g.lda, b.sA, B, g.ldb,
                       b.sB, C, g.ldc, b.sC, ep, sBias);
  });
}

// the batched `ex` kernels' LDS opt-ins (> 64 KiB), so that a first launch can be captured into a graph
int warm_dma5_batched_ex() { return warm_form<BatchedExForm, 0, 1, 2, 3>(); }

}  // namespace mmh
