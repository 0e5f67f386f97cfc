// launch_ex_t.hip -- the fused-epilogue forms (mmh_sgemm_ex, launch_ex.hip) with A stored k x m (TN, TT): a translation unit of
// its own so that build.py compiles these 24 instantiations beside launch_ex.hip's.  Part of libmmult_hip.so (see internal.hpp).
#include "launch_dma5.hpp"

namespace mmh {

int launch_dma5_ex_ta(mmh_context *ctx, int kernel, const GemmArgs &g) {
  return launch_form<ExForm, 1, 3>(kernel, g, [&](auto f) { return launch_dma5_tile<decltype(f)>(ctx, g); });
}

int warm_dma5_ex_ta() { return warm_form<ExForm, 1, 3>(); }

}  // namespace mmh
