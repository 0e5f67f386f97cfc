// launch_ex_t.hip -- the fused-epilogue forms (mmh_sgemm_ex, launch_ex.hip) with A stored k x m (TN, TT): a translation unit of
// its own so that build.py compiles these 24 instantiations beside launch_ex.hip's.  Part of libmmult_hip.so (see internal.hpp).
#include "launch_ex.hpp"

namespace mmh {

int launch_dma5_ex_ta(mmh_context *ctx, int kernel, const GemmArgs &g) {
  return g.tb ? launch_ex_family<3>(ctx, kernel, g) : launch_ex_family<1>(ctx, kernel, g);
}

int warm_dma5_ex_ta(mmh_context *ctx) {
  (void)ctx;
  const int rc = warm_ex_families<1>();
  return rc != MMH_OK ? rc : warm_ex_families<3>();
}

}  // namespace mmh
