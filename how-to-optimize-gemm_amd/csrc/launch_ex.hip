// launch_ex.hip -- launches of the fused-epilogue forms (mmh_sgemm_ex: C = act(alpha op(A) op(B) + beta C + bias), GemmArgs::ex)
// with A stored m x k (NN, NT) on the K2W tiles with op forms, and the naive kernel with the epilogue written out the same
// way -- the independent reference on the device, what MMH_KERNEL_NAIVE runs and what an empty contraction (k == 0) runs.
// launch_ex_t.hip holds the forms with A stored k x m (24 kernels per unit, so that build.py compiles them side by side) and
// is reached through this unit's two entry points.  Part of libmmult_hip.so (see internal.hpp).
#include "launch_dma5.hpp"

namespace mmh {

// K0 with the epilogue: one fmaf chain from +0 over ascending k per element (sgemm_naive_op_kernel's), then DESIGN.md section
// 2's epilogue, one rounding per operation and nothing contracted.  beta == 0: C is not read.  k == 0: A and B are not read.
__global__ void __launch_bounds__(256)
sgemm_naive_ex_kernel(int transa, int transb, int m, int n, int k, const float *__restrict__ A, int lda,
                      const float *__restrict__ B, int ldb, float *__restrict__ C, int ldc, const Dma5Epilogue ep) {
  const int col = blockIdx.x * 64 + (threadIdx.x & 63);
  const int row = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (row >= m || col >= n) return;
  const size_t a_i = transa ? 1 : (size_t)lda, a_p = transa ? (size_t)lda : 1;
  const size_t b_p = transb ? 1 : (size_t)ldb, b_j = transb ? (size_t)ldb : 1;
  float acc = 0.0f;
  for (int p = 0; p < k; ++p) acc = __builtin_fmaf(A[row * a_i + p * a_p], B[p * b_p + col * b_j], acc);
  float v[1] = {acc}, c[1] = {0.0f}, b[1] = {0.0f};
  if (ep.beta != 0.0f) c[0] = C[(size_t)row * ldc + col];
  if (ep.bias_mode == MMH_BIAS_COL) b[0] = ep.bias[col];
  if (ep.bias_mode == MMH_BIAS_ROW) b[0] = ep.bias[row];
  dma5_epilogue_apply(ep, v, c, b);
  C[(size_t)row * ldc + col] = v[0];
}

int launch_dma5_ex(mmh_context *ctx, int kernel, const GemmArgs &g) {
  if (g.ta) return launch_dma5_ex_ta(ctx, kernel, g);
  return launch_form<ExForm, 0, 2>(kernel, g, [&](auto f) { return launch_dma5_tile<decltype(f)>(ctx, g); });
}

int launch_naive_ex(const GemmArgs &g) {
  dim3 grid((unsigned)((g.n + 63) / 64), (unsigned)((g.m + 3) / 4)), block(256);
  hipLaunchKernelGGL(sgemm_naive_ex_kernel, grid, block, 0, g.s, g.ta, g.tb, g.m, g.n, g.k, g.A, g.lda, g.B, g.ldb, g.C, g.ldc,
                     ex_args(g));
  HIP_TRY(hipGetLastError());
  set_last_launch(std::string("sgemm_naive_ex_kernel") + ex_tag(g));
  return MMH_OK;
}

// the ex kernels' LDS opt-ins (> 64 KiB), so that a first ex launch can be captured into a graph like an op one
int warm_dma5_ex() {
  const int rc = warm_form<ExForm, 0, 2>();
  return rc != MMH_OK ? rc : warm_dma5_ex_ta();
}

}  // namespace mmh
