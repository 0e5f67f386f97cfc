// launch_batched.hip -- launches of mmh_sgemm_batched's one-launch form: the K2W tiles with op forms (k2w_tiles,
// internal.hpp; sgemm_dma5.hpp, sgemm_mfma_dma5_batched_kernel) over batch x tiles, whole-tile and guarded, every op pair,
// as a BatchedForm through launch_dma5.hpp's launch_form, tail split and description; and the naive batched kernel.  A translation unit of its own,
// like launch_op.hip, so that build.py compiles its instantiations in parallel.  Part of libmmult_hip.so (see internal.hpp).
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

namespace {

// the batched kernels of tile K, operand form OP (0 = NN included): plain launches only; `first` is an argument of its own
template <class K_, int OP>
struct BatchedForm {
  using K = K_;
  static constexpr bool SK = false;
  static auto plain(bool edge) {
    return edge ? sgemm_mfma_dma5_batched_kernel<MMH_K2W_ARGS(K), true, K::NL, K::D, OP>
                : sgemm_mfma_dma5_batched_kernel<MMH_K2W_ARGS(K), false, K::NL, K::D, OP>;
  }
};

// One launch (or several of at most kBatchedMaxWorkgroups workgroups each: whole matrices per launch, the pointers
// advanced to the chunk's first matrix) of tile F::K over every matrix.  Whole-tile or guarded for the whole matrix set
// (dma5_form with the strides); the tail split of launch_dma5_tile on the residency of the NN twin.
template <class F>
int launch_batched_tile(mmh_context *ctx, const GemmArgs &g, const BatchArgs &bt) {
  using K = typename F::K;
  using T = Dma5Tile<MMH_K2W_ARGS(K), K::NL>;
  const int form = dma5_form(ctx, K::BM, K::BN, g, bt);
  if (form < 0) return 1;
  const bool edge = form == 1;
  auto kern = F::plain(edge);
  const int ok = allow_big_lds(kern, T::LDS_BYTES);
  if (ok != MMH_OK) return ok;
  const int nbm = (g.m + K::BM - 1) / K::BM, nbn = (g.n + K::BN - 1) / K::BN;
  const long per = (long)nbm * nbn;   // (<= 2^17: a matrix inside the descriptor window)
  const long mats = std::max(1L, kBatchedMaxWorkgroups / per);   // matrices per launch
  int acc = g.acc;
  if constexpr (kAbBuild) acc |= (ctx && ctx->ab_batch_major) ? 2 : 0;
  long launches = 0;
  bool split = false;
  for (long b0 = 0; b0 < bt.batch; b0 += mats) {
    const long tiles = std::min(mats, bt.batch - b0) * per;
    const float *A = g.A + b0 * bt.sA, *B = g.B + b0 * bt.sB;
    float *C = g.C + b0 * bt.sC;
    const long first = dma5_split_first(ctx, NnForm<K>::plain(edge), T::THREADS, T::LDS_BYTES, tiles, g.k);
    dma5_launch_rounds(first, tiles, [&](long workgroups, long id0) {
      hipLaunchKernelGGL(kern, dim3((unsigned)workgroups), dim3(T::THREADS), T::LDS_BYTES, g.s, g.m, g.n, g.k, A, g.lda, bt.sA, B, g.ldb,
                         bt.sB, C, g.ldc, bt.sC, acc, nbm, nbn, (unsigned)id0);
      ++launches;
    });
    split |= first < tiles;
    HIP_TRY(hipGetLastError());
  }
  char what[kTextSize];
  int at = dma5_plain_text<K>(what, "sgemm_mfma_dma5_batched_kernel", edge, bt.batch * per, split);
  at = text_add(what, at, "%s, batch %ld", op_tag(g), bt.batch);
  if (launches > 1) text_add(what, at, " as %ld launches", launches);
  set_last_launch(what);
  return MMH_OK;
}

}  // namespace

int launch_dma5_batched(mmh_context *ctx, int kernel, const GemmArgs &g, const BatchArgs &b) {
  return launch_form<BatchedForm, 0, 1, 2, 3>(kernel, g, [&](auto f) { return launch_batched_tile<decltype(f)>(ctx, g, b); });
}

int launch_naive_batched(const GemmArgs &g, const BatchArgs &b) {
  const long gx = (g.n + 63) / 64, gy = (g.m + 3) / 4;
  const long mats = std::max(1L, std::min(65535L, kBatchedMaxWorkgroups / (gx * gy)));   // matrices per launch
  long launches = 0;
  for (long b0 = 0; b0 < b.batch; b0 += mats) {
    const long nb = std::min(mats, b.batch - b0);
    hipLaunchKernelGGL(sgemm_naive_batched_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)nb), dim3(256), 0, g.s, g.ta, g.tb, g.m,
                       g.n, g.k, g.A ? g.A + b0 * b.sA : nullptr, g.lda, b.sA, g.B ? g.B + b0 * b.sB : nullptr, g.ldb, b.sB,
                       g.C + b0 * b.sC, g.ldc, b.sC, g.acc);
    ++launches;
    HIP_TRY(hipGetLastError());
  }
  char what[160];
  snprintf(what, sizeof what, "sgemm_naive_batched_kernel%s, batch %ld", op_tag(g), b.batch);
  std::string s = what;
  if (launches > 1) s += " as " + std::to_string(launches) + " launches";
  set_last_launch(s);
  return MMH_OK;
}

// the batched kernels' LDS opt-ins (> 64 KiB), so that a first batched launch can be captured into a graph
int warm_dma5_batched() { return warm_form<BatchedForm, 0, 1, 2, 3>(); }

}  // namespace mmh
