// qlinear_s8o_256_edge.hip -- qlinear_s8o_kernel<256,256,8,true> (see qlinear_s8o.hpp).  Part of libmmult_hip_q8o.so.
#include "qlinear_s8o.hpp"

namespace mmh {
hipError_t launch_qlinear_s8o_256_edge(const QlinearS8oArgs &a, hipStream_t s) { return launch_qlinear_s8o_tile<256, true>(a, s); }
}  // namespace mmh
