// launch_dma5.hip -- the NN launches of the LDS-DMA tiles with loader waves (sgemm_dma5.hpp, K2W): the tiles of k2w_tiles
// (internal.hpp: 64x64, 128x64, 128x128 and the whole-round tiles 96x96 / 96x64 / 160x160; the tools build's A/B ids below),
// each as one workgroup per tile or as the persistent stream-K form (chained parts), each in a whole-tile and a guarded
// (EDGE: any m, n, k, 4-byte aligned operands) instantiation -- through launch_dma5.hpp's launcher.
// Part of libmmult_hip.so (see internal.hpp).
#include "launch_dma5.hpp"
#ifdef MMH_AB_BUILD
#include "sgemm_dma5_rim.hpp"   // tools/ab/: round 4's fused rim (measured: 2.2x slower per edge tile)
#endif

namespace mmh {
namespace {

template <class K>
int warm_dma5_tile(mmh_context *ctx, float *scratch, hipStream_t s) {
  constexpr int BM = K::BM, BN = K::BN, KB = 32, WTM = K::WTM, WTN = K::WTN, NBUF = K::NBUF, NL = K::NL, D = K::D;
  using T = Dma5Tile<BM, BN, KB, WTM, WTN, NBUF, NL>;
  int rc;
  auto plain = [&](auto kern) { return warm_plain_kernel(kern, BM, BN, KB, T::THREADS, T::LDS_BYTES, scratch, s); };
  if ((rc = plain(sgemm_mfma_dma5_kernel<BM, BN, KB, WTM, WTN, NBUF, false, NL, D>)) != MMH_OK) return rc;
  if ((rc = plain(sgemm_mfma_dma5_kernel<BM, BN, KB, WTM, WTN, NBUF, true, NL, D>)) != MMH_OK) return rc;
  if constexpr (K::SK) {
    auto sk = sgemm_dma5_streamk_kernel<BM, BN, KB, WTM, WTN, NBUF, false, true, NL, D>;
    auto ske = sgemm_dma5_streamk_kernel<BM, BN, KB, WTM, WTN, NBUF, true, true, NL, D>;
    (void)resident_per_cu(ctx, ske, T::THREADS, T::LDS_BYTES);
    if ((rc = warm_streamk_kernel(sk, BM, BN, KB, T::THREADS, 160 * 1024, scratch, s)) != MMH_OK) return rc;
    return warm_streamk_kernel(ske, BM, BN, KB, T::THREADS, 160 * 1024, scratch, s);
  }
  return MMH_OK;
}

// The NN launch of tile K.  Tools build: the RIM launch of the 64x64 tiles first (measured slower than the thin edge
// tiles, sgemm_dma5.hpp rim_wave): one row and / or column past a 64-boundary rides on the trimmed shape's tiles -- where
// the caller (MMH_KERNEL_AUTO's table, or the forced kernel's own rule on the TRIMMED tile count) wants one workgroup per tile.
template <class K>
int launch_nn(mmh_context *ctx, const GemmArgs &g) {
#ifdef MMH_AB_BUILD
  if constexpr (K::BM == 64 && K::BN == 64 && K::NL == 2 && K::SK) {
    constexpr int BM = K::BM, BN = K::BN, KB = 32, WTM = K::WTM, WTN = K::WTN, NBUF = K::NBUF, NL = K::NL, D = K::D;
    using T = Dma5Tile<BM, BN, KB, WTM, WTN, NBUF, NL>;
    int r_m = 0, r_n = 0;
    if (ctx && ctx->rim5 && dma5_form(ctx, BM, BN, g) == 1 && dma5_rim_dims(g.m, g.n, &r_m, &r_n)) {
      const int nbm0 = (g.m - r_m) / 64 + ((g.m - r_m) % 64 ? 1 : 0), nbn0 = (g.n - r_n) / 64 + ((g.n - r_n) % 64 ? 1 : 0);
      const long tiles0 = (long)nbm0 * nbn0;
      bool plain = g.form == 1;
      if (g.form == 0) {
        auto occ = sgemm_dma5_streamk_kernel<BM, BN, KB, WTM, WTN, NBUF, true, true, NL, D>;
        plain = !ctx->streamk || streamk_wanted(ctx, tiles0, BM, BN, resident_per_cu(ctx, occ, T::THREADS, T::LDS_BYTES)) == 0;
      }
      if (plain) {
        using SR = Dma5Segment<BM, BN, KB, WTM, WTN, NBUF, false, true, false, NL, D, true>;
        auto kern = sgemm_mfma_dma5_rim_kernel<BM, BN, KB, WTM, WTN, NBUF, NL, D>;
        const int ok = allow_big_lds(kern, SR::RIM_LDS_BYTES);
        if (ok != MMH_OK) return ok;
        hipLaunchKernelGGL(kern, dim3((unsigned)tiles0), dim3(T::THREADS + 64), SR::RIM_LDS_BYTES, g.s, g.m, g.n, g.k, g.A, g.lda, g.B,
                           g.ldb, g.C, g.ldc, g.acc, nbm0, nbn0, r_m, r_n);
        HIP_TRY(hipGetLastError());
        char what[320];
        snprintf(what, sizeof what,
                 "sgemm_mfma_dma5_rim_kernel<%d,%d> wave tile %dx%d, K-slice %d x %d ring buffers by %d loader waves' LDS-DMA, guarded, "
                 "%ld workgroups of %d threads on %d x %d + a rim wave for %d row(s), %d column(s) (vector ALU, out of the tiles' LDS)",
                 BM, BN, 16 * WTM, 16 * WTN, KB, NBUF, NL, tiles0, T::THREADS + 64, g.m - r_m, g.n - r_n, r_m, r_n);
        set_last_launch(what);
        return MMH_OK;
      }
    }
  }
#endif
  return launch_dma5_tile<NnForm<K>>(ctx, g);
}

#ifdef MMH_AB_BUILD
// A/B ids of the tools build (valid results): their own configurations, as K2wTile<id, BM BN WTM WTN NBUF NL D SK OPS RS>
template <int ID, int BM, int BN, int WTM, int WTN, int NBUF, int NL, bool SK = true, int RS = 1>
int launch_ab(mmh_context *ctx, const GemmArgs &g) {
  return launch_nn<K2wTile<ID, BM, BN, WTM, WTN, NBUF, NL, 2, SK, false, RS>>(ctx, g) <= 0 ? MMH_OK : MMH_ERR_UNSUPPORTED;
}
int launch_dma5_ab(mmh_context *ctx, int kernel, const GemmArgs &g) {
  switch (kernel) {
    //                               BM   BN WTM WTN NBUF NL
    // ONE loader wave (round 4's first form), and the 160-wide whole-round tiles that lost to the chained stream-K launch
    // of the 128-wide ones (N = 2560: 140.8 against 145.2; N = 1920 on 160x96: 130.9 against 137.5)
    case 64: return launch_ab<64, 64, 64, 2, 2, 3, 1>(ctx, g);
    // ring depth: one 64x64 workgroup per CU runs 0.43 us slices -- two slices of look-ahead are less than a DMA's latency
    case 65: return launch_ab<65, 64, 64, 2, 2, 6, 2>(ctx, g);
    case 66: return launch_ab<66, 64, 64, 2, 2, 4, 2>(ctx, g);
    case 67: return launch_ab<67, 64, 64, 2, 2, 6, 4>(ctx, g);
    case 68: return launch_ab<68, 128, 64, 4, 2, 3, 1>(ctx, g);
    case 69: return launch_ab<69, 128, 64, 4, 2, 4, 4>(ctx, g);
    case 72: return launch_ab<72, 128, 128, 4, 4, 3, 1>(ctx, g);
    case 79: return launch_ab<79, 160, 96, 5, 3, 3, 1, false>(ctx, g);
    case 80: return launch_ab<80, 160, 160, 5, 5, 3, 1, false>(ctx, g);
    // (rounds 4-5, fragment reads as a block: 1 / 2 / 4 loaders at N = 2560 -- 256 tiles, one whole round -- 139.9 / 139.8 /
    // 140.6 against the 128x128 tile's chained stream-K 144.6; four whole rounds at N = 5120: 143.9 against 150.2.  It was
    // the ten ds_read instructions per k-step leaving in one block (id 95 keeps that form); the four-loader form with
    // the reads spread is the product's MMH_KERNEL_MFMA_160X160_DMA5)
    case 82: return launch_ab<82, 160, 160, 5, 5, 3, 2, false>(ctx, g);
    // round 5: 96x64 / 64x96 (N = 1152: 216 tiles -- one round of 256 CUs at 84 % -- instead of 324 tiles of 64x64 under stream-K)
    case 83: return launch_ab<83, 96, 64, 3, 2, 3, 4>(ctx, g);   // (with a stream-K form: never ahead)
    case 84: return launch_ab<84, 96, 64, 3, 2, 3, 2>(ctx, g);
    case 85: return launch_ab<85, 64, 96, 2, 3, 3, 2, false>(ctx, g);
    // round 6 (second session): the fragment reads as a BLOCK in front of the k-step's MFMAs (RS = 0: rounds 4-6's form) --
    // what every tile here ran until the reads were spread behind the first MFMAs (sgemm_dma5.hpp, RS)
    case 95: return launch_ab<95, 160, 160, 5, 5, 3, 4, false, 0>(ctx, g);
    case 96: return launch_ab<96, 128, 128, 4, 4, 3, 4, true, 0>(ctx, g);
    case 97: return launch_ab<97, 128, 64, 4, 2, 3, 4, true, 0>(ctx, g);
    case 98: return launch_ab<98, 64, 64, 2, 2, 3, 2, true, 0>(ctx, g);
    case 99: return launch_ab<99, 96, 96, 3, 3, 3, 1, false, 0>(ctx, g);
    // (with the reads spread, the prefetch distance D = 1 / 2 / 3 k-steps measures the same on the 64x64, 96x64 and 128x64
    // tiles, N = 1024 .. 2048, 3072, 4096: +-0.3 % -- profiles/r06_prefetch_distance_ab.md)
    // (RS = 2, measured and dropped: the slice's barrier BEHIND the k-step's first MFMA, its wait in that instruction's 32
    // cycles of matrix-pipe time -- +-0.2 % on every tile and size: the barrier is not what the loop waits for)
    default:
      set_last_error("unknown kernel variant");
      return MMH_ERR_INVALID_ARG;
  }
}
#endif

}  // namespace

int launch_dma5(mmh_context *ctx, int kernel, const GemmArgs &g) {
  constexpr int kNone = 1 << 30;
  const int rc = k2w_tiles::with(kernel, [&](auto t) { return launch_nn<decltype(t)>(ctx, g); }, kNone);
  if (rc != kNone) return rc;
#ifdef MMH_AB_BUILD
  return launch_dma5_ab(ctx, kernel, g);
#else
  set_last_error("unknown kernel variant");
  return MMH_ERR_INVALID_ARG;
#endif
}

int warm_dma5(mmh_context *ctx, float *scratch, hipStream_t s) {
#ifdef MMH_AB_BUILD
  {   // the RIM launch of the 64x64 tile: one tile + its rim (65 x 65 x 32 on scratch)
    using SR = Dma5Segment<64, 64, 32, 2, 2, 3, false, true, false, 2, 2, true>;
    auto kern = sgemm_mfma_dma5_rim_kernel<64, 64, 32, 2, 2, 3, 2, 2>;
    if (const int rc = allow_big_lds(kern, SR::RIM_LDS_BYTES); rc != MMH_OK) return rc;
    hipLaunchKernelGGL(kern, dim3(1), dim3(448), SR::RIM_LDS_BYTES, s, 65, 65, 32, scratch, 32, scratch, 68, scratch + 65536, 68, 0, 1, 1,
                       1, 1);
    HIP_TRY(hipGetLastError());
  }
#endif
  return k2w_tiles::each([&](auto t) { return warm_dma5_tile<decltype(t)>(ctx, scratch, s); });
}

#ifdef MMH_DMA_TIMELINE
// timeline build only: where the plain K2W kernels write their timeline stamps (this translation unit's copy of
// g_dma_stamps; 4 x uint64 per workgroup; NULL switches them off).  tools/dma5_timeline.py.
extern "C" int mmh_ab_set_stamps5(mmh_handle_t h, void *stamps) {
  if (!h) return MMH_ERR_INVALID_ARG;
  ENTER(h);
  HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_dma_stamps), &stamps, sizeof(void *)));
  return MMH_OK;
}
// 4 = the plain kernels' layout; 32 = the stream-K kernels' (sgemm_dma5.hpp, streamk5_body; tools/sk_timeline.py)
extern "C" int mmh_ab_set_stamp_stride5(mmh_handle_t h, int stride) {
  if (!h || (stride != 4 && stride != 32)) return MMH_ERR_INVALID_ARG;
  ENTER(h);
  HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_dma_stamp_stride), &stride, sizeof(int)));
  return MMH_OK;
}
#endif

}  // namespace mmh
