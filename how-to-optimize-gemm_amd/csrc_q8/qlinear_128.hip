// qlinear_128.hip -- qlinear_s8_kernel<128,128,4,false,*,*> (see qlinear_launch.hpp).  Part of libmmult_hip_q8.so.
#include "qlinear_launch.hpp"

namespace mmh {
hipError_t launch_qlinear_128(const QlinearArgs &a, hipStream_t s) { return launch_qlinear_tile<128, false>(a, s); }
}  // namespace mmh
