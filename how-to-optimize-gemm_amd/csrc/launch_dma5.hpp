// launch_dma5.hpp -- the one launcher of the K2W tiles (sgemm_dma5.hpp): whole or guarded, plain or chained stream-K, the
// tail split.  A tile is a K2wTile (internal.hpp); the kernels of a call FORM on it -- NN, transposed operands, the fused
// epilogue, and the two strided batched forms -- are a NnForm / OpForm / ExForm / BatchedForm / BatchedExForm below.
// launch_dma5.hip instantiates launch_dma5_tile<NnForm<tile>> (and has the NN warm-up, which launches); launch_op.hip,
// launch_ex.hip and launch_ex_t.hip instantiate it for their own forms through launch_form / warm_form; launch_batched.hip and
// launch_batched_ex.hip instantiate launch_batched_tile -- the batch in chunks, each with the tail split -- the same way, and
// run their naive kernels through launch_naive_chunks.
#pragma once
#include <stdarg.h>

#include <tuple>

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

// ---- the kernels of a form ----
// What launch_dma5_tile needs to know of a call form on tile K, operand form OP = g.ta | g.tb << 1: the plain kernel (whole-tile
// / guarded) and, where K::SK, the stream-K kernel (... x unchained / chained parts), their names in the launch descriptions,
// the tag a description ends in, what the kernels take behind the common arguments (a tuple) and the value of `accumulate`.
// The two kernels of a pair have one function type; those of another form have another: this is where that difference lives.
template <class K_>
struct NnForm {   // mmh_sgemm: the only form with unchained stream-K and the tools build's A/B option bits
  using K = K_;
  static constexpr bool NN = true, SK = K::SK;
  static constexpr const char *plain_name = "sgemm_mfma_dma5_kernel", *streamk_name = "sgemm_dma5_streamk_kernel";
  static auto plain(bool edge) {
    return edge ? sgemm_mfma_dma5_kernel<MMH_K2W_ARGS(K), true, K::NL, K::D, K::RS>
                : sgemm_mfma_dma5_kernel<MMH_K2W_ARGS(K), false, K::NL, K::D, K::RS>;
  }
  // the guarded chained stream-K kernel: its residency bounds the persistent grid of every form (a function of its own, so
  // that the other forms' units instantiate this kernel alone)
  static auto streamk_bound() { return sgemm_dma5_streamk_kernel<MMH_K2W_ARGS(K), true, true, K::NL, K::D, K::RS>; }
  static auto streamk(bool edge, bool chained) {
    return edge ? (chained ? streamk_bound() : sgemm_dma5_streamk_kernel<MMH_K2W_ARGS(K), true, false, K::NL, K::D, K::RS>)
                : (chained ? sgemm_dma5_streamk_kernel<MMH_K2W_ARGS(K), false, true, K::NL, K::D, K::RS>
                           : sgemm_dma5_streamk_kernel<MMH_K2W_ARGS(K), false, false, K::NL, K::D, K::RS>);
  }
  static std::string tag(const GemmArgs &) { return {}; }
  static std::tuple<> extra(const GemmArgs &) { return {}; }
  static int acc(const mmh_context *ctx, const GemmArgs &g) {   // (tools build: A/B switches ride in the upper bits, sgemm_dma5.hpp)
    if (kAbBuild && ctx) return g.acc | (ctx->ab_nodefer ? 2 : 0) | (ctx->ab_whole_ranges ? 4 : 0) | ((ctx->ab_group_m & 0xff) << 8);
    return g.acc;
  }
};
template <class K_, int OP>
struct OpForm {   // mmh_sgemm_op, OP = 1 / 2 / 3: the chained stream-K kernels alone, which keep the bits
  using K = K_;
  static constexpr bool NN = false, SK = K::SK;
  static constexpr const char *plain_name = "sgemm_mfma_dma5_op_kernel", *streamk_name = "sgemm_dma5_op_streamk_kernel";
  static auto plain(bool edge) {
    return edge ? sgemm_mfma_dma5_op_kernel<MMH_K2W_ARGS(K), true, K::NL, K::D, OP>
                : sgemm_mfma_dma5_op_kernel<MMH_K2W_ARGS(K), false, K::NL, K::D, OP>;
  }
  static auto streamk(bool edge, bool) {
    return edge ? sgemm_dma5_op_streamk_kernel<MMH_K2W_ARGS(K), true, K::NL, K::D, OP>
                : sgemm_dma5_op_streamk_kernel<MMH_K2W_ARGS(K), false, K::NL, K::D, OP>;
  }
  static std::string tag(const GemmArgs &g) { return op_tag(g); }   // (no allocation: the small-string buffer holds it)
  static std::tuple<> extra(const GemmArgs &) { return {}; }
  static int acc(const mmh_context *, const GemmArgs &g) { return g.acc; }
};
template <class K_, int OP>
struct ExForm {   // mmh_sgemm_ex (g.alpha .. g.act), OP = 0 .. 3, NN included: the epilogue behind the common arguments
  using K = K_;
  static constexpr bool NN = false, SK = K::SK;
  static constexpr const char *plain_name = "sgemm_mfma_dma5_ex_kernel", *streamk_name = "sgemm_dma5_ex_streamk_kernel";
  static auto plain(bool edge) {
    return edge ? sgemm_mfma_dma5_ex_kernel<MMH_K2W_ARGS(K), true, K::NL, K::D, OP>
                : sgemm_mfma_dma5_ex_kernel<MMH_K2W_ARGS(K), false, K::NL, K::D, OP>;
  }
  static auto streamk(bool edge, bool) {
    return edge ? sgemm_dma5_ex_streamk_kernel<MMH_K2W_ARGS(K), true, K::NL, K::D, OP>
                : sgemm_dma5_ex_streamk_kernel<MMH_K2W_ARGS(K), false, K::NL, K::D, OP>;
  }
  static std::string tag(const GemmArgs &g) { return ex_tag(g); }
  static std::tuple<Dma5Epilogue> extra(const GemmArgs &g) { return {ex_args(g)}; }
  static int acc(const mmh_context *, const GemmArgs &) { return 0; }   // (the chain starts at +0: beta C is the epilogue's)
};

// ---- the kernels of a batched form ----
// The strided batched kernels of tile K, operand form OP (0 = NN included): plain launches only, and `first` -- the id of a
// launch's first workgroup -- an argument of its own.  What launch_batched_tile needs to know of the two: the kernel pair, its
// name and the tag of the description, and what differs in the arguments -- front(): what the kernels take in front of `nbm,
// nbn, first`; back(): what they take behind it, for the launches of the chunk that starts at matrix b0.
template <class K_, int OP>
struct BatchedForm {   // mmh_sgemm_batched: `accumulate` in front (tools build: option 108 rides in its bit 1), nothing behind
  using K = K_;
  static constexpr bool SK = false;
  static constexpr const char *plain_name = "sgemm_mfma_dma5_batched_kernel";
  static auto plain(bool edge) {
    return edge ? sgemm_mfma_dma5_batched_kernel<MMH_K2W_ARGS(K), true, K::NL, K::D, OP>
                : sgemm_mfma_dma5_batched_kernel<MMH_K2W_ARGS(K), false, K::NL, K::D, OP>;
  }
  static std::string tag(const GemmArgs &g) { return op_tag(g); }
  static std::tuple<int> front(const mmh_context *ctx, const GemmArgs &g) {
    return {g.acc | ((kAbBuild && ctx && ctx->ab_batch_major) ? 2 : 0)};
  }
  static std::tuple<> back(const GemmArgs &, const BatchArgs &, long) { return {}; }
};
// the epilogue of the matrices from b0 on, and the stride of their biases: the bias pointer advanced to matrix b0's (no bias:
// NULL and stride 0, whatever came) -- what the batched `ex` kernels, the naive one included, take behind their other arguments
inline std::tuple<Dma5Epilogue, long long> ex_chunk_args(const GemmArgs &g, const BatchArgs &bt, long b0) {
  const bool none = g.bias_mode == MMH_BIAS_NONE;
  Dma5Epilogue ep = ex_args(g);
  ep.bias = none ? nullptr : g.bias + b0 * bt.sBias;
  return {ep, none ? 0 : bt.sBias};
}
template <class K_, int OP>
struct BatchedExForm {   // mmh_sgemm_batched_ex: no `accumulate` (the chain starts at +0); the epilogue and the bias stride behind
  using K = K_;
  static constexpr bool SK = false;
  static constexpr const char *plain_name = "sgemm_mfma_dma5_batched_ex_kernel";
  static auto plain(bool edge) {
    return edge ? sgemm_mfma_dma5_batched_ex_kernel<MMH_K2W_ARGS(K), true, K::NL, K::D, OP>
                : sgemm_mfma_dma5_batched_ex_kernel<MMH_K2W_ARGS(K), false, K::NL, K::D, OP>;
  }
  static std::string tag(const GemmArgs &g) { return ex_tag(g); }
  static std::tuple<> front(const mmh_context *, const GemmArgs &) { return {}; }
  static std::tuple<Dma5Epilogue, long long> back(const GemmArgs &g, const BatchArgs &bt, long b0) { return ex_chunk_args(g, bt, b0); }
};

// A launch description is written into a char[kTextSize] (the longest is under 300 characters) piece by piece: text_add
// appends at `at` and returns where the next piece goes -- never past the buffer: a longer text is cut, as by one snprintf.
constexpr int kTextSize = 448;
inline int text_add(char *what, int at, const char *format, ...) __attribute__((format(printf, 3, 4)));
inline int text_add(char *what, int at, const char *format, ...) {
  va_list args;
  va_start(args, format);
  const int n = vsnprintf(what + at, kTextSize - at, format, args);
  va_end(args);
  return std::min(at + std::max(n, 0), kTextSize - 1);
}
// How every description of a launch on tile K starts ...
template <class K>
int dma5_tile_text(char *what, const char *kernel) {
  return text_add(what, 0, "%s<%d,%d> wave tile %dx%d, K-slice %d x %d ring buffers by %d loader wave%s' LDS-DMA, fragments %d k-steps ahead",
                  kernel, K::BM, K::BN, 16 * K::WTM, 16 * K::WTN, 32, K::NBUF, K::NL, K::NL > 1 ? "s" : "", K::D);
}
// ... and the description of a plain launch (one workgroup per tile), up to its tag
template <class K>
int dma5_plain_text(char *what, const char *kernel, bool edge, long workgroups, bool split) {
  return text_add(what, dma5_tile_text<K>(what, kernel), ", %s%ld workgroups of %d threads%s", edge ? "guarded, " : "", workgroups,
                  Dma5Tile<MMH_K2W_ARGS(K), K::NL>::THREADS, split ? " (the last round as a launch of its own)" : "");
}
// The first launch, and the last round as a launch of its own (dma5_split_first): launch(workgroups, id of the first one)
template <class L>
void dma5_launch_rounds(long first, long tiles, L launch) {
  launch(first, 0L);
  if (first < tiles) launch(tiles - first, first);
}

// One launch of tile F::K in form F -- bounded by the NN twins' residency whatever the form, so that an op or `ex` launch has
// the grid, the rounds, the tail split and the stream-K decision of the NN launch of its shape (tests/test_op_kernel_resources.py
// and tests/test_ex_kernel_resources.py hold those kernels' registers to at least the NN twins' co-residency).  Returns MMH_OK,
// an error, or 1: the shape does not qualify.
template <class F>
int launch_dma5_tile(mmh_context *ctx, const GemmArgs &g) {
  using K = typename F::K;
  constexpr int BM = K::BM, BN = K::BN, KB = 32;
  using T = Dma5Tile<MMH_K2W_ARGS(K), K::NL>;
  const int form = dma5_form(ctx, BM, BN, g);
  if (form < 0) return 1;
  const bool edge = form == 1;
  GemmArgs ga = g;
  ga.acc = F::acc(ctx, g);
  if constexpr (F::SK) {
    if (ctx && ctx->streamk) {
      // the parts of a range as ONE stream of slices (MMH_OPT_STREAMK_CHAIN, default on), or each with a prologue of its own (NN only)
      const bool chained = !F::NN || ctx->sk_chain != 0;
      auto occ = NnForm<K>::streamk_bound();
      auto kern = F::streamk(edge, chained);
      // (tools build, option 103: the residency of the instantiation that is launched -- DESIGN.md section 8, found on the CPU)
      if constexpr (F::NN) {
        if (kAbBuild && ctx->ab_own_occ && !edge) occ = kern;
      } else {
        (void)allow_big_lds(occ, T::LDS_BYTES);
      }
      char what[kTextSize];
      text_add(what, dma5_tile_text<K>(what, F::streamk_name), "%s%s", chained ? ", chained parts" : "", edge ? ", guarded" : "");
      // a thin last tile row / column (dma5_raster dispatches those last, at a fraction of a tile's cost) does not make a
      // tile count ragged: plain or persistent is decided on the whole tiles alone
      const int order_min10 = (BM == 128 && BN == 128) ? 10 : 0;   // (phase-ordered tables from one 128x128 tile per workgroup)
      const int sk = std::apply([&](auto... x) {
        return launch_streamk(ctx, kern, occ, BM, BN, KB, T::THREADS, T::LDS_BYTES, what, ga, full_tiles(g.m, g.n, BM, BN), order_min10, x...);
      }, F::extra(g));
      if (!F::NN && sk == MMH_OK) set_last_launch(last_launch_ref() + F::tag(g));
      if (sk <= 0) return sk;
    }
  }
  const int nbm = (g.m + BM - 1) / BM, nbn = (g.n + BN - 1) / BN;
  const long tiles = (long)nbm * nbn;
  const long first = dma5_split_first(ctx, NnForm<K>::plain(edge), T::THREADS, T::LDS_BYTES, tiles, g.k);
  const int acc_bits = edge ? F::acc(nullptr, g) : ga.acc;   // (the guarded plain kernels take no A/B bits)
  auto kern = F::plain(edge);
  const int ok = allow_big_lds(kern, T::LDS_BYTES);
  if (ok != MMH_OK) return ok;
  dma5_launch_rounds(first, tiles, [&](long workgroups, long id0) {
    std::apply([&](auto... x) {
      hipLaunchKernelGGL(kern, dim3((unsigned)workgroups), dim3(T::THREADS), T::LDS_BYTES, g.s, g.m, g.n, g.k, g.A, g.lda, g.B, g.ldb, g.C,
                         g.ldc, acc_bits | (int)((unsigned)(id0 >> 3) << 16), nbm, nbn, x...);
    }, F::extra(g));
  });
  HIP_TRY(hipGetLastError());
  char what[kTextSize];
  text_add(what, dma5_plain_text<K>(what, F::plain_name, edge, tiles, first < tiles), "%s", F::tag(g).c_str());
  set_last_launch(what);
  return MMH_OK;
}

// One launch (or several of at most kBatchedMaxWorkgroups workgroups each: whole matrices per launch, the pointers
// advanced to the chunk's first matrix) of tile F::K in batched form F over every matrix.  Whole-tile or guarded for the whole
// matrix set (dma5_form with the strides); the tail split of launch_dma5_tile on the residency of the NN twin, chunk by chunk.
// Returns MMH_OK, an error, or 1: the matrices do not qualify.
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
  long launches = 0;
  bool split = false;
  for (long b0 = 0; b0 < bt.batch; b0 += mats) {
    const long tiles = std::min(mats, bt.batch - b0) * per;
    const float *A = g.A + b0 * bt.sA, *B = g.B + b0 * bt.sB;
    float *C = g.C + b0 * bt.sC;
    const long first = dma5_split_first(ctx, NnForm<K>::plain(edge), T::THREADS, T::LDS_BYTES, tiles, g.k);
    dma5_launch_rounds(first, tiles, [&](long workgroups, long id0) {
      std::apply([&](auto... x) {
        hipLaunchKernelGGL(kern, dim3((unsigned)workgroups), dim3(T::THREADS), T::LDS_BYTES, g.s, g.m, g.n, g.k, A, g.lda, bt.sA, B, g.ldb,
                           bt.sB, C, g.ldc, bt.sC, x...);
      }, std::tuple_cat(F::front(ctx, g), std::make_tuple(nbm, nbn, (unsigned)id0), F::back(g, bt, b0)));
      ++launches;
    });
    split |= first < tiles;
    HIP_TRY(hipGetLastError());
  }
  char what[kTextSize];
  int at = dma5_plain_text<K>(what, F::plain_name, edge, bt.batch * per, split);
  at = text_add(what, at, "%s, batch %ld", F::tag(g).c_str(), bt.batch);
  if (launches > 1) text_add(what, at, " as %ld launches", launches);
  set_last_launch(what);
  return MMH_OK;
}

// The chunk loop of the two naive batched kernels (the matrix in blockIdx.z): at most 65535 matrices and kBatchedMaxWorkgroups
// workgroups per launch, launch(grid, A, B, C, b0) with the pointers advanced to the chunk's first matrix b0 (A and B may be
// NULL: an empty contraction reads neither), and the description: `what`, the batch and, for more than one, the launches.
template <class L>
int launch_naive_chunks(const GemmArgs &g, const BatchArgs &b, std::string what, L launch) {
  const long gx = (g.n + 63) / 64, gy = (g.m + 3) / 4;
  const long mats = std::max(1L, std::min(65535L, kBatchedMaxWorkgroups / (gx * gy)));   // matrices per launch
  long launches = 0;
  for (long b0 = 0; b0 < b.batch; b0 += mats) {
    launch(dim3((unsigned)gx, (unsigned)gy, (unsigned)std::min(mats, b.batch - b0)), g.A ? g.A + b0 * b.sA : nullptr,
           g.B ? g.B + b0 * b.sB : nullptr, g.C + b0 * b.sC, b0);
    ++launches;
    HIP_TRY(hipGetLastError());
  }
  what += ", batch " + std::to_string(b.batch);
  if (launches > 1) what += " as " + std::to_string(launches) + " launches";
  set_last_launch(what);
  return MMH_OK;
}

// launch(F<tile of `kernel`, g.ta | g.tb << 1>{}) for the operand forms OPS a translation unit instantiates of form F, on the
// tiles with op forms; 1 (does not qualify) for every other tile and operand form
template <template <class, int> class F, int... OPS, class L>
int launch_form(int kernel, const GemmArgs &g, L launch) {
  const int op = g.ta | (g.tb << 1);
  return k2w_tiles::with(kernel, [&](auto t) {
    using K = decltype(t);
    int rc = 1;
    if constexpr (K::OPS) {
      auto launch_if = [&](auto form, int form_op) {
        if (op == form_op) rc = launch(form);
      };
      (launch_if(F<K, OPS>{}, OPS), ...);
    }
    return rc;
  }, 1);
}
// the LDS opt-ins (> 64 KiB) of the same instantiations, operand form by operand form and tile by tile, so that a first launch
// can be captured into a graph like an NN one (persistent launches may ask for up to 160 KiB: launch_streamk's residency pin)
template <class F>
int warm_form_tile() {
  constexpr size_t lds = Dma5Tile<MMH_K2W_ARGS(F::K), F::K::NL>::LDS_BYTES;
  int rc;
  if ((rc = allow_big_lds(F::plain(false), lds)) != MMH_OK || (rc = allow_big_lds(F::plain(true), lds)) != MMH_OK) return rc;
  if constexpr (F::SK)
    if ((rc = allow_big_lds(F::streamk(false, true), 160 * 1024)) == MMH_OK) rc = allow_big_lds(F::streamk(true, true), 160 * 1024);
  return rc;
}
template <template <class, int> class F, int... OPS>
int warm_form() {
  int rc = MMH_OK;
  auto warm_op = [&](auto op) {   // one operand form on every tile with op forms, unless an earlier one failed
    if (rc != MMH_OK) return;
    rc = k2w_tiles::each([](auto t) {
      using K = decltype(t);
      if constexpr (K::OPS) return warm_form_tile<F<K, decltype(op)::value>>();
      else return (int)MMH_OK;
    });
  };
  (warm_op(std::integral_constant<int, OPS>{}), ...);
  return rc;
}

}  // namespace mmh
