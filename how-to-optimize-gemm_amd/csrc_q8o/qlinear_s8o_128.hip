// qlinear_s8o_128.hip -- qlinear_s8o_kernel<128,128,4,false> (see qlinear_s8o.hpp).  Part of libmmult_hip_q8o.so.
#include "qlinear_s8o.hpp"

namespace mmh {
hipError_t launch_qlinear_s8o_128(const QlinearS8oArgs &a, hipStream_t s) { return launch_qlinear_s8o_tile<128, false>(a, s); }
}  // namespace mmh
