// launch_op.hip -- launches of the transposed-operand forms (mmh_sgemm_op, GemmArgs::ta / tb): the K2W tiles with op forms
// (k2w_tiles, internal.hpp; sgemm_dma5.hpp, OP) through launch_dma5.hpp's launcher, and the naive kernel with two index
// swaps.  A translation unit of its own so that build.py compiles the op instantiations beside launch_dma5.hip's NN ones.
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

namespace {

template <int OP>
int launch_op_family(mmh_context *ctx, int kernel, const GemmArgs &g) {
  return k2w_tiles::with(kernel, [&](auto t) {
    using K = decltype(t);
    if constexpr (K::OPS) return launch_dma5_tile<K, OP>(ctx, g);
    return 1;
  }, 1);
}

// the LDS opt-ins of one op pair's instantiations, tile by tile
template <int OP>
int warm_op_families() {
  return k2w_tiles::each([](auto t) {
    using K = decltype(t);
    if constexpr (K::OPS) {
      constexpr int BM = K::BM, BN = K::BN, KB = 32, WTM = K::WTM, WTN = K::WTN, NBUF = K::NBUF, NL = K::NL, D = K::D;
      constexpr size_t lds = Dma5Tile<BM, BN, KB, WTM, WTN, NBUF, NL>::LDS_BYTES;
      int rc;
      if ((rc = allow_big_lds(sgemm_mfma_dma5_op_kernel<BM, BN, KB, WTM, WTN, NBUF, false, NL, D, OP>, lds)) != MMH_OK) return rc;
      if ((rc = allow_big_lds(sgemm_mfma_dma5_op_kernel<BM, BN, KB, WTM, WTN, NBUF, true, NL, D, OP>, lds)) != MMH_OK) return rc;
      // (persistent launches may ask for up to 160 KiB: launch_streamk's residency pin)
      if ((rc = allow_big_lds(sgemm_dma5_op_streamk_kernel<BM, BN, KB, WTM, WTN, NBUF, false, NL, D, OP>, 160 * 1024)) != MMH_OK)
        return rc;
      return allow_big_lds(sgemm_dma5_op_streamk_kernel<BM, BN, KB, WTM, WTN, NBUF, true, NL, D, OP>, 160 * 1024);
    } else {
      return (int)MMH_OK;
    }
  });
}

}  // namespace

int launch_dma5_op(mmh_context *ctx, int kernel, const GemmArgs &g) {
  switch (g.ta | (g.tb << 1)) {
    case 1: return launch_op_family<1>(ctx, kernel, g);
    case 2: return launch_op_family<2>(ctx, kernel, g);
    case 3: return launch_op_family<3>(ctx, kernel, g);
    default: return 1;
  }
}

int launch_naive_op(const GemmArgs &g) {
  dim3 grid((unsigned)((g.n + 63) / 64), (unsigned)((g.m + 3) / 4)), block(256);
  hipLaunchKernelGGL(sgemm_naive_op_kernel, grid, block, 0, g.s, g.ta, g.tb, g.m, g.n, g.k, g.A, g.lda, g.B, g.ldb, g.C, g.ldc, g.acc);
  HIP_TRY(hipGetLastError());
  set_last_launch(std::string("sgemm_naive_op_kernel") + op_tag(g));
  return MMH_OK;
}

// the op kernels' LDS opt-ins (> 64 KiB), so that a first op launch can be captured into a graph like an NN one
int warm_dma5_op(mmh_context *ctx) {
  (void)ctx;
  int rc;
  if ((rc = warm_op_families<1>()) != MMH_OK) return rc;
  if ((rc = warm_op_families<2>()) != MMH_OK) return rc;
  return warm_op_families<3>();
}

}  // namespace mmh
