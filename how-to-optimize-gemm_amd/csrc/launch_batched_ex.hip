// launch_batched_ex.hip -- launches of mmh_sgemm_batched_ex's one-launch form: the K2W tiles with op forms (k2w_tiles,
// internal.hpp; sgemm_dma5.hpp, sgemm_mfma_dma5_batched_ex_kernel) over batch x tiles with the fused epilogue (GemmArgs::ex,
// BatchArgs::sBias), whole-tile and guarded, every op pair, as a BatchedExForm through launch_dma5.hpp's launch_form, tail
// split and description; and the naive batched kernel with the epilogue written out -- the independent reference on the
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

namespace {

// the batched `ex` kernels of tile K, operand form OP (0 = NN included): plain launches only; `first` is an argument of its own
template <class K_, int OP>
struct BatchedExForm {
  using K = K_;
  static constexpr bool SK = false;
  static auto plain(bool edge) {
    return edge ? sgemm_mfma_dma5_batched_ex_kernel<MMH_K2W_ARGS(K), true, K::NL, K::D, OP>
                : sgemm_mfma_dma5_batched_ex_kernel<MMH_K2W_ARGS(K), false, K::NL, K::D, OP>;
  }
};

// the bias of the launch's chunk that starts at matrix b0 (no bias: NULL, whatever came)
const float *bias_at(const GemmArgs &g, const BatchArgs &bt, long b0) {
  return g.bias_mode == MMH_BIAS_NONE ? nullptr : g.bias + b0 * bt.sBias;
}

// launch_batched_tile (launch_batched.hip) for the `ex` kernels: chunks of at most kBatchedMaxWorkgroups workgroups -- the
// operands' and the bias's pointers advanced to the chunk's first matrix --, whole-tile or guarded for the whole matrix set,
// the tail split on the residency of the NN twin.
template <class F>
int launch_batched_ex_tile(mmh_context *ctx, const GemmArgs &g, const BatchArgs &bt) {
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
  const long long sBias = g.bias_mode == MMH_BIAS_NONE ? 0 : bt.sBias;
  long launches = 0;
  bool split = false;
  for (long b0 = 0; b0 < bt.batch; b0 += mats) {
    const long tiles = std::min(mats, bt.batch - b0) * per;
    const float *A = g.A + b0 * bt.sA, *B = g.B + b0 * bt.sB;
    float *C = g.C + b0 * bt.sC;
    Dma5Epilogue ep = ex_args(g);
    ep.bias = bias_at(g, bt, b0);
    const long first = dma5_split_first(ctx, NnForm<K>::plain(edge), T::THREADS, T::LDS_BYTES, tiles, g.k);
    dma5_launch_rounds(first, tiles, [&](long workgroups, long id0) {
      hipLaunchKernelGGL(kern, dim3((unsigned)workgroups), dim3(T::THREADS), T::LDS_BYTES, g.s, g.m, g.n, g.k, A, g.lda, bt.sA, B, g.ldb,
                         bt.sB, C, g.ldc, bt.sC, nbm, nbn, (unsigned)id0, ep, sBias);
      ++launches;
    });
    split |= first < tiles;
    HIP_TRY(hipGetLastError());
  }
  char what[kTextSize];
  int at = dma5_plain_text<K>(what, "sgemm_mfma_dma5_batched_ex_kernel", edge, bt.batch * per, split);
  at = text_add(what, at, "%s, batch %ld", ex_tag(g).c_str(), bt.batch);
  if (launches > 1) text_add(what, at, " as %ld launches", launches);
  set_last_launch(what);
  return MMH_OK;
}

}  // namespace

int launch_dma5_batched_ex(mmh_context *ctx, int kernel, const GemmArgs &g, const BatchArgs &b) {
  return launch_form<BatchedExForm, 0, 1, 2, 3>(kernel, g, [&](auto f) { return launch_batched_ex_tile<decltype(f)>(ctx, g, b); });
}

int launch_naive_batched_ex(const GemmArgs &g, const BatchArgs &b) {
  const long gx = (g.n + 63) / 64, gy = (g.m + 3) / 4;
  const long mats = std::max(1L, std::min(65535L, kBatchedMaxWorkgroups / (gx * gy)));   // matrices per launch
  const long long sBias = g.bias_mode == MMH_BIAS_NONE ? 0 : b.sBias;
  long launches = 0;
  for (long b0 = 0; b0 < b.batch; b0 += mats) {
    const long nb = std::min(mats, b.batch - b0);
    Dma5Epilogue ep = ex_args(g);
    ep.bias = bias_at(g, b, b0);
    hipLaunchKernelGGL(sgemm_naive_batched_ex_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)nb), dim3(256), 0, g.s, g.ta, g.tb, g.m,
                       g.n, g.k, g.A ? g.A + b0 * b.sA : nullptr, g.lda, b.sA, g.B ? g.B + b0 * b.sB : nullptr, g.ldb, b.sB,
                       g.C + b0 * b.sC, g.ldc, b.sC, ep, sBias);
    ++launches;
    HIP_TRY(hipGetLastError());
  }
  std::string s = std::string("sgemm_naive_batched_ex_kernel") + ex_tag(g) + ", batch " + std::to_string(b.batch);
  if (launches > 1) s += " as " + std::to_string(launches) + " launches";
  set_last_launch(s);
  return MMH_OK;
}

// the batched `ex` kernels' LDS opt-ins (> 64 KiB), so that a first launch can be captured into a graph
int warm_dma5_batched_ex() { return warm_form<BatchedExForm, 0, 1, 2, 3>(); }

}  // namespace mmh
