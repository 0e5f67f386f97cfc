// Host stand-ins for the few HIP constructs csrc/relu_grad.hpp uses, for tools/host_check/relu_grad_host_check.cpp only: the
// kernels compile as plain functions and run one thread at a time, with the built-in indices as thread-local variables.
#pragma once
#include <stddef.h>
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __restrict__
struct dim3 {
  unsigned x = 1, y = 1, z = 1;
};
extern thread_local dim3 blockIdx, threadIdx, gridDim, blockDim;
