// launch_dma5.hpp -- the one launcher of the K2W tiles (sgemm_dma5.hpp) that launch_dma5.hip (NN), launch_op.hip (op forms)
// and launch_batched.hip (its tail split and descriptions) instantiate for their own kernels: whole or guarded, plain or
// chained stream-K, the tail split.  A tile is a K2wTile (internal.hpp).
#pragma once
#include "ab_build.hpp"
#include "launch_common.hpp"
#include "sgemm_dma5.hpp"

namespace mmh {

inline const char *op_tag(const GemmArgs &g) {
  return g.ta ? (g.tb ? ", operands TT" : ", operands TN") : (g.tb ? ", operands NT" : "");
}
// what an `ex` launch's description ends in: ", operands NT, epilogue alpha beta bias(col) relu" (", epilogue identity")
inline std::string ex_tag(const GemmArgs &g) {
  std::string t = std::string(g.ta ? (g.tb ? ", operands TT" : ", operands TN") : (g.tb ? ", operands NT" : ", operands NN")) + ", epilogue";
  const size_t bare = t.size();
  if (g.alpha != 1.0f) t += " alpha";
  if (g.beta != 0.0f) t += " beta";
  if (g.bias_mode == MMH_BIAS_COL) t += " bias(col)";
  if (g.bias_mode == MMH_BIAS_ROW) t += " bias(row)";
  if (g.act == MMH_ACT_RELU) t += " relu";
  if (t.size() == bare) t += " identity";
  return t;
}
inline Dma5Epilogue ex_args(const GemmArgs &g) { return Dma5Epilogue{g.alpha, g.beta, g.bias, g.bias_mode, g.act}; }

// The tail split (sgemm_mfma_dma5_kernel): ONE whole round and a last round of JUST UNDER one tile per CU -- 0.85 CUs <
// tiles - w CUs <= CUs: where the dispatcher was seen to pack (229 .. 256 of 256; a smaller last round spreads by itself,
// and after two or more rounds the slots of a CU have drifted apart: splitting then only costs the overlap of the rounds,
// -3 .. -15 % when forced) -- and K-slices enough that a second launch is small beside a tile (k >= 512): the last round
// goes out as a launch of its own behind the whole one (dma5_tail_split, internal.hpp: the cost table prices it).  The
// size of the first launch (`tiles`: no split), on the residency of `twin`: the NN plain instantiation of the tile.
template <typename K>
long dma5_split_first(mmh_context *ctx, K twin, int threads, size_t lds, long tiles, int k) {
  if (!ctx || !ctx->split_tail) return tiles;
  (void)allow_big_lds(twin, lds);
  const long cus = ctx->cu_count > 0 ? ctx->cu_count : 256;
  const long w = std::min(resident_per_cu(ctx, twin, threads, lds), 3);
  return dma5_tail_split(tiles, w, cus, k) ? w * cus : tiles;
}

// One launch of tile K: OP == 0 the NN instantiations (and unchained stream-K, and the tools build's A/B option bits), OP = 1 / 2 / 3 (g.ta | g.tb << 1) the op instantiations -- bounded by the NN twins' residency, so that an
// op launch has the grid and the rounds of the NN launch of its shape (tests/test_op_kernel_resources.py holds the op
// kernels' registers to at least the NN twins' co-residency).  Returns MMH_OK, an error, or 1: the shape does not qualify.
// EX: the epilogue kernels (mmh_sgemm_ex, g.alpha .. g.act) of operand form OP, 0 = NN included: the launch an op form of the
// shape gets -- the same bounds, grid, rounds, tail split and stream-K decision (tests/test_ex_kernel_resources.py holds
// their registers to the NN twins' co-residency too) -- with the epilogue behind the common arguments.
template <class K, int OP, bool EX = false>
int launch_dma5_tile(mmh_context *ctx, const GemmArgs &g) {
  constexpr int BM = K::BM, BN = K::BN, KB = 32, WTM = K::WTM, WTN = K::WTN, NBUF = K::NBUF, NL = K::NL, D = K::D, RS = K::RS;
  using T = Dma5Tile<BM, BN, KB, WTM, WTN, NBUF, NL>;
  const int form = dma5_form(ctx, BM, BN, g);
  if (form < 0) return 1;
  const bool edge = form == 1;
  char what[320];
  GemmArgs ga = g;   // (tools build: A/B switches ride in the upper bits of `accumulate`, sgemm_dma5.hpp)
  if (kAbBuild && OP == 0 && !EX && ctx) ga.acc |= (ctx->ab_nodefer ? 2 : 0) | (ctx->ab_whole_ranges ? 4 : 0) | ((ctx->ab_group_m & 0xff) << 8);
  if constexpr (K::SK) {
    if (ctx && ctx->streamk) {
      // the parts of a range as ONE stream of slices (MMH_OPT_STREAMK_CHAIN, default on), or each with a prologue of its own
      // (NN only: the op forms have the chained kernels alone, which keep the bits)
      const bool chained = OP != 0 || EX || ctx->sk_chain != 0;
      auto occ = sgemm_dma5_streamk_kernel<BM, BN, KB, WTM, WTN, NBUF, true, true, NL, D, RS>;   // (the NN launch's bound)
      auto kern = occ;
      if constexpr (EX) {
        (void)kern;
        (void)allow_big_lds(occ, T::LDS_BYTES);
      } else if constexpr (OP == 0) {
        kern = edge ? (chained ? occ : sgemm_dma5_streamk_kernel<BM, BN, KB, WTM, WTN, NBUF, true, false, NL, D, RS>)
                    : (chained ? sgemm_dma5_streamk_kernel<BM, BN, KB, WTM, WTN, NBUF, false, true, NL, D, RS>
                               : sgemm_dma5_streamk_kernel<BM, BN, KB, WTM, WTN, NBUF, false, false, NL, D, RS>);
        // (tools build, option 103: the residency of the instantiation that is launched -- DESIGN.md section 8, found on the CPU)
        if (kAbBuild && ctx->ab_own_occ && !edge) occ = kern;
      } else {
        kern = edge ? sgemm_dma5_op_streamk_kernel<BM, BN, KB, WTM, WTN, NBUF, true, NL, D, OP>
                    : sgemm_dma5_op_streamk_kernel<BM, BN, KB, WTM, WTN, NBUF, false, NL, D, OP>;
        (void)allow_big_lds(occ, T::LDS_BYTES);
      }
      snprintf(what, sizeof what,
               "%s<%d,%d> wave tile %dx%d, K-slice %d x %d ring buffers by %d loader wave%s' LDS-DMA, fragments %d k-steps ahead%s%s",
               EX ? "sgemm_dma5_ex_streamk_kernel" : OP ? "sgemm_dma5_op_streamk_kernel" : "sgemm_dma5_streamk_kernel", BM, BN, 16 * WTM,
               16 * WTN, KB, NBUF, NL, NL > 1 ? "s" : "", D, chained ? ", chained parts" : "", edge ? ", guarded" : "");
      // a thin last tile row / column (dma5_raster dispatches those last, at a fraction of a tile's cost) does not make a
      // tile count ragged: plain or persistent is decided on the whole tiles alone
      const int order_min10 = (BM == 128 && BN == 128) ? 10 : 0;   // (phase-ordered tables from one 128x128 tile per workgroup)
      int sk;
      if constexpr (EX) {
        auto kx = edge ? sgemm_dma5_ex_streamk_kernel<BM, BN, KB, WTM, WTN, NBUF, true, NL, D, OP>
                       : sgemm_dma5_ex_streamk_kernel<BM, BN, KB, WTM, WTN, NBUF, false, NL, D, OP>;
        sk = launch_streamk(ctx, kx, occ, BM, BN, KB, T::THREADS, T::LDS_BYTES, what, ga, full_tiles(g.m, g.n, BM, BN), order_min10,
                            ex_args(g));
        if (sk == MMH_OK) set_last_launch(last_launch_ref() + ex_tag(g));
      } else {
        sk = launch_streamk(ctx, kern, occ, BM, BN, KB, T::THREADS, T::LDS_BYTES, what, ga, full_tiles(g.m, g.n, BM, BN), order_min10);
        if (OP && sk == MMH_OK) set_last_launch(last_launch_ref() + op_tag(g));
      }
      if (sk <= 0) return sk;
    }
  }
  const int nbm = (g.m + BM - 1) / BM, nbn = (g.n + BN - 1) / BN;
  auto twin = edge ? sgemm_mfma_dma5_kernel<BM, BN, KB, WTM, WTN, NBUF, true, NL, D, RS>
                   : sgemm_mfma_dma5_kernel<BM, BN, KB, WTM, WTN, NBUF, false, NL, D, RS>;
  const long tiles = (long)nbm * nbn;
  const long first = dma5_split_first(ctx, twin, T::THREADS, T::LDS_BYTES, tiles, g.k);
  const int acc_bits = edge ? g.acc : ga.acc;
  if constexpr (EX) {
    auto kx = edge ? sgemm_mfma_dma5_ex_kernel<BM, BN, KB, WTM, WTN, NBUF, true, NL, D, OP>
                   : sgemm_mfma_dma5_ex_kernel<BM, BN, KB, WTM, WTN, NBUF, false, NL, D, OP>;
    const int ok = allow_big_lds(kx, T::LDS_BYTES);
    if (ok != MMH_OK) return ok;
    hipLaunchKernelGGL(kx, dim3((unsigned)first), dim3(T::THREADS), T::LDS_BYTES, g.s, g.m, g.n, g.k, g.A, g.lda, g.B, g.ldb, g.C,
                       g.ldc, 0, nbm, nbn, ex_args(g));
    if (first < tiles)
      hipLaunchKernelGGL(kx, dim3((unsigned)(tiles - first)), dim3(T::THREADS), T::LDS_BYTES, g.s, g.m, g.n, g.k, g.A, g.lda, g.B,
                         g.ldb, g.C, g.ldc, (int)((unsigned)(first >> 3) << 16), nbm, nbn, ex_args(g));
  } else {
  auto kern = twin;
  if constexpr (OP != 0)
    kern = edge ? sgemm_mfma_dma5_op_kernel<BM, BN, KB, WTM, WTN, NBUF, true, NL, D, OP>
                : sgemm_mfma_dma5_op_kernel<BM, BN, KB, WTM, WTN, NBUF, false, NL, D, OP>;
  const int ok = allow_big_lds(kern, T::LDS_BYTES);
  if (ok != MMH_OK) return ok;
  hipLaunchKernelGGL(kern, dim3((unsigned)first), dim3(T::THREADS), T::LDS_BYTES, g.s, g.m, g.n, g.k, g.A, g.lda, g.B, g.ldb, g.C,
                     g.ldc, acc_bits, nbm, nbn);
  if (first < tiles)
    hipLaunchKernelGGL(kern, dim3((unsigned)(tiles - first)), dim3(T::THREADS), T::LDS_BYTES, g.s, g.m, g.n, g.k, g.A, g.lda, g.B,
                       g.ldb, g.C, g.ldc, acc_bits | (int)((unsigned)(first >> 3) << 16), nbm, nbn);
  }
  HIP_TRY(hipGetLastError());
  snprintf(what, sizeof what,
           "%s<%d,%d> wave tile %dx%d, K-slice %d x %d ring buffers by %d loader wave%s' LDS-DMA, fragments %d k-steps ahead, "
           "%s%ld workgroups of %d threads%s%s",
           EX ? "sgemm_mfma_dma5_ex_kernel" : OP ? "sgemm_mfma_dma5_op_kernel" : "sgemm_mfma_dma5_kernel", BM, BN, 16 * WTM, 16 * WTN, KB,
           NBUF, NL, NL > 1 ? "s" : "", D, edge ? "guarded, " : "", tiles, T::THREADS,
           first < tiles ? " (the last round as a launch of its own)" : "", EX ? "" : op_tag(g));
  set_last_launch(EX ? what + ex_tag(g) : std::string(what));
  return MMH_OK;
}

}  // namespace mmh
