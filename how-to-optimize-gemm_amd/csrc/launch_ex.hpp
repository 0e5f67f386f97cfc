// launch_ex.hpp -- what the two translation units of the fused-epilogue forms (mmh_sgemm_ex: launch_ex.hip, A stored m x k;
// launch_ex_t.hip, A stored k x m) share: the launch and the LDS opt-ins of one operand form's `ex` instantiations
// (sgemm_dma5.hpp, EP) on the K2W tiles with op forms, through launch_dma5.hpp's launcher.  24 kernels per unit, so that
// build.py compiles them side by side.
#pragma once
#include "launch_dma5.hpp"

namespace mmh {
namespace {

template <int OP>
int launch_ex_family(mmh_context *ctx, int kernel, const GemmArgs &g) {
  return k2w_tiles::with(kernel, [&](auto t) {
    using K = decltype(t);
    if constexpr (K::OPS) return launch_dma5_tile<K, OP, true>(ctx, g);
    return 1;
  }, 1);
}

template <int OP>
int warm_ex_families() {
  return k2w_tiles::each([](auto t) {
    using K = decltype(t);
    if constexpr (K::OPS) {
      constexpr int BM = K::BM, BN = K::BN, KB = 32, WTM = K::WTM, WTN = K::WTN, NBUF = K::NBUF, NL = K::NL, D = K::D;
      constexpr size_t lds = Dma5Tile<BM, BN, KB, WTM, WTN, NBUF, NL>::LDS_BYTES;
      int rc;
      if ((rc = allow_big_lds(sgemm_mfma_dma5_ex_kernel<BM, BN, KB, WTM, WTN, NBUF, false, NL, D, OP>, lds)) != MMH_OK) return rc;
      if ((rc = allow_big_lds(sgemm_mfma_dma5_ex_kernel<BM, BN, KB, WTM, WTN, NBUF, true, NL, D, OP>, lds)) != MMH_OK) return rc;
      // (persistent launches may ask for up to 160 KiB: launch_streamk's residency pin)
      if ((rc = allow_big_lds(sgemm_dma5_ex_streamk_kernel<BM, BN, KB, WTM, WTN, NBUF, false, NL, D, OP>, 160 * 1024)) != MMH_OK)
        return rc;
      return allow_big_lds(sgemm_dma5_ex_streamk_kernel<BM, BN, KB, WTM, WTN, NBUF, true, NL, D, OP>, 160 * 1024);
    } else {
      return (int)MMH_OK;
    }
  });
}

}  // namespace
}  // namespace mmh
