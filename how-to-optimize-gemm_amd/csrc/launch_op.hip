// launch_op.hip -- launchers of the transposed-operand forms (mmh_sgemm_op, GemmArgs::ta / tb): the 64x64, 128x64 and
// 128x128 K2W tiles (sgemm_dma5.hpp, OP) as one workgroup per tile or as the chained stream-K launch, each whole-tile and
// guarded, and the naive kernel with two index swaps.  A translation unit of its own: launch_dma5.hip's NN
// instantiations are compiled exactly as before, and build.py compiles the two in parallel.
// Part of libmmult_hip.so (see internal.hpp).
#include "launch_common.hpp"
#include "sgemm_dma5.hpp"

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

const char *op_tag(const GemmArgs &g) { return g.ta ? (g.tb ? ", operands TT" : ", operands TN") : ", operands NT"; }

// The op form of launch_dma5_tile (launch_dma5.hip) for one tile: the same decisions -- whole or guarded, plain or chained
// stream-K, the tail split -- taken on the residency of the NN twin's instantiations, so that an op launch has the grid
// and the rounds of the NN launch of its shape (tests/test_op_kernel_resources.py holds the op kernels' registers to
// at least the NN twins' co-residency).  No unchained stream-K and no RIM form.
template <int BM, int BN, int WTM, int WTN, int NBUF, int NL, int D, int OP>
int launch_op_tile(mmh_context *ctx, int kernel, const GemmArgs &g) {
  constexpr int KB = 32;
  using T = Dma5Tile<BM, BN, KB, WTM, WTN, NBUF, NL>;
  if (!dma5_shape_ok(ctx, kernel, g)) return 1;   // the stored layouts' descriptor window; guarded shapes allowed
  const bool edge = !fast_shape(BM, BN, KB, g);
  char what[320];
  if (ctx && ctx->streamk) {
    auto kern = edge ? sgemm_dma5_op_streamk_kernel<BM, BN, KB, WTM, WTN, NBUF, true, NL, D, OP>
                     : sgemm_dma5_op_streamk_kernel<BM, BN, KB, WTM, WTN, NBUF, false, NL, D, OP>;
    auto occ = sgemm_dma5_streamk_kernel<BM, BN, KB, WTM, WTN, NBUF, true, true, NL, D, 1>;   // (the NN launch's bound)
    (void)allow_big_lds(occ, T::LDS_BYTES);
    snprintf(what, sizeof what,
             "sgemm_dma5_op_streamk_kernel<%d,%d> wave tile %dx%d, K-slice %d x %d ring buffers by %d loader waves' LDS-DMA, "
             "fragments %d k-steps ahead, chained parts%s",
             BM, BN, 16 * WTM, 16 * WTN, KB, NBUF, NL, D, edge ? ", guarded" : "");
    long decide = 0;   // (thin last tile row / column: launch_dma5_tile)
    if (edge) {
      const int nbm = (g.m + BM - 1) / BM, nbn = (g.n + BN - 1) / BN;
      const int thin_row = (nbm > 1 && g.m - (nbm - 1) * BM <= 16) ? 1 : 0, thin_col = (nbn > 1 && g.n - (nbn - 1) * BN <= 16) ? 1 : 0;
      if (thin_row || thin_col) decide = (long)(nbm - thin_row) * (nbn - thin_col);
    }
    const int sk = launch_streamk(ctx, kern, occ, BM, BN, KB, T::THREADS, T::LDS_BYTES, what, g, decide,
                                  (BM == 128 && BN == 128) ? 10 : 0);
    if (sk == MMH_OK) set_last_launch(last_launch_ref() + op_tag(g));
    if (sk <= 0) return sk;
  }
  const int nbm = (g.m + BM - 1) / BM, nbn = (g.n + BN - 1) / BN;
  auto kern = edge ? sgemm_mfma_dma5_op_kernel<BM, BN, KB, WTM, WTN, NBUF, true, NL, D, OP>
                   : sgemm_mfma_dma5_op_kernel<BM, BN, KB, WTM, WTN, NBUF, false, NL, D, OP>;
  auto twin = edge ? sgemm_mfma_dma5_kernel<BM, BN, KB, WTM, WTN, NBUF, true, NL, D, 1>
                   : sgemm_mfma_dma5_kernel<BM, BN, KB, WTM, WTN, NBUF, false, NL, D, 1>;
  const int ok = allow_big_lds(kern, T::LDS_BYTES);
  if (ok != MMH_OK) return ok;
  const long tiles = (long)nbm * nbn;
  long first = tiles;
  if (ctx && ctx->split_tail) {   // the tail split of launch_dma5_tile
    (void)allow_big_lds(twin, T::LDS_BYTES);
    const long cus = ctx->cu_count > 0 ? ctx->cu_count : 256;
    const long w = std::min(resident_per_cu(ctx, twin, T::THREADS, T::LDS_BYTES), 3);
    if (dma5_tail_split(tiles, w, cus, g.k) && (w * cus) % 8 == 0) first = w * cus;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)first), dim3(T::THREADS), T::LDS_BYTES, g.s, g.m, g.n, g.k, g.A, g.lda, g.B, g.ldb, g.C,
                     g.ldc, g.acc, nbm, nbn);
  if (first < tiles)
    hipLaunchKernelGGL(kern, dim3((unsigned)(tiles - first)), dim3(T::THREADS), T::LDS_BYTES, g.s, g.m, g.n, g.k, g.A, g.lda, g.B,
                       g.ldb, g.C, g.ldc, g.acc | (int)((unsigned)(first >> 3) << 16), nbm, nbn);
  HIP_TRY(hipGetLastError());
  snprintf(what, sizeof what,
           "sgemm_mfma_dma5_op_kernel<%d,%d> wave tile %dx%d, K-slice %d x %d ring buffers by %d loader waves' LDS-DMA, fragments %d "
           "k-steps ahead, %s%ld workgroups of %d threads%s%s",
           BM, BN, 16 * WTM, 16 * WTN, KB, NBUF, NL, D, edge ? "guarded, " : "", tiles, T::THREADS,
           first < tiles ? " (the last round as a launch of its own)" : "", op_tag(g));
  set_last_launch(what);
  return MMH_OK;
}

// (the NN configurations of launch_dma5: BM BN WTM WTN NBUF NL D)
template <int OP>
int launch_op_family(mmh_context *ctx, int kernel, const GemmArgs &g) {
  switch (kernel) {
    case MMH_KERNEL_MFMA_64X64_DMA5: return launch_op_tile<64, 64, 2, 2, 3, 2, 2, OP>(ctx, kernel, g);
    case MMH_KERNEL_MFMA_128X64_DMA5: return launch_op_tile<128, 64, 4, 2, 3, 4, 2, OP>(ctx, kernel, g);
    case MMH_KERNEL_MFMA_128X128_DMA5: return launch_op_tile<128, 128, 4, 4, 3, 4, 2, OP>(ctx, kernel, g);
    default: return 1;
  }
}

template <int BM, int BN, int WTM, int WTN, int NBUF, int NL, int D, int OP>
int warm_op_tile() {
  constexpr int KB = 32;
  using T = Dma5Tile<BM, BN, KB, WTM, WTN, NBUF, NL>;
  int rc;
  if ((rc = allow_big_lds(sgemm_mfma_dma5_op_kernel<BM, BN, KB, WTM, WTN, NBUF, false, NL, D, OP>, T::LDS_BYTES)) != MMH_OK) return rc;
  if ((rc = allow_big_lds(sgemm_mfma_dma5_op_kernel<BM, BN, KB, WTM, WTN, NBUF, true, NL, D, OP>, T::LDS_BYTES)) != MMH_OK) return rc;
  // (persistent launches may ask for up to 160 KiB: launch_streamk's residency pin)
  if ((rc = allow_big_lds(sgemm_dma5_op_streamk_kernel<BM, BN, KB, WTM, WTN, NBUF, false, NL, D, OP>, 160 * 1024)) != MMH_OK) return rc;
  return allow_big_lds(sgemm_dma5_op_streamk_kernel<BM, BN, KB, WTM, WTN, NBUF, true, NL, D, OP>, 160 * 1024);
}

template <int OP>
int warm_op_families() {
  int rc;
  if ((rc = warm_op_tile<64, 64, 2, 2, 3, 2, 2, OP>()) != MMH_OK) return rc;
  if ((rc = warm_op_tile<128, 64, 4, 2, 3, 4, 2, OP>()) != MMH_OK) return rc;
  return warm_op_tile<128, 128, 4, 4, 3, 4, 2, OP>();
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
