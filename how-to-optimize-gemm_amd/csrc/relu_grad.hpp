// relu_grad.hpp -- the memory-bound pass of the linear layer's backward (mmh_relu_grad_colsum): the ReLU gate on the incoming
// gradient and the bias gradient, in one sweep over rows x cols floats.
//
// Contract (include/mmult_hip.h has the full text; tests/relu_grad_ref.py restates it in numpy), per element (i, j):
//   z          = g                       without a gate (y == NULL)
//   z          = y <= 0 ? +0 : g         with one: a SELECT on g's bits -- a closed gate gives +0 for g = NaN / Inf too, an open
//                                        one passes -0 and subnormals untouched; y = NaN leaves it open (!(y <= 0), the forward
//                                        ReLU's predicate)
//   p_b[j]     = z(bR, j), then fl(p_b + z(r, j)) for r ascending inside block b = rows [bR, min(bR + R, rows))
//   colsum[j]  = p_0, then fl(s + p_b) for b ascending          (colsum_finish_kernel; one block: written by the pass itself)
// No float atomics: every block STORES its partial row to the handle's workspace and the finish kernel sums the rows in
// block order, so the bits depend on rows and R alone -- not on the grid, the path or the arrival order.
//
// Shape of the pass: a column's chain inside a block is serial, so the parallelism is (rows / R) x cols chains.  A thread owns
// W consecutive columns (W = 4: one 16-byte load per operand and row; W = 1: operands that are only 4-byte aligned, and the
// cols % 4 columns past the last whole quad) and walks
// its block's rows U at a time with the loads of the next U rows issued before the current ones are stored (g and z carry
// no __restrict__: dZ == dG is allowed, and without the explicit batches the compiler must keep every load behind the store
// before it).  A wave reads 1 KiB of one row per instruction.  Row blocks lie on grid.x (rows / R may pass 65535), column
// chunks of 256 W on grid.y (strided when there are more than 65535 of them); every offset is 64-bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// (tools/host_check/relu_grad_host_check.cpp runs these kernels as host functions and defines it away)
#ifndef MMH_RG_PER_LANE
#define MMH_RG_PER_LANE(offset, stride) asm volatile("" : "+v"(offset), "+v"(stride))
#endif

namespace mmh {

typedef float rg_f32x4 __attribute__((ext_vector_type(4)));

constexpr int RG_THREADS = 256;
constexpr int RG_U = 8;   // rows in flight per thread and batch (twice that with the batch being loaded)

struct ReluGradArgs {
  const float *g;    // rows x cols, ldg
  const float *y;    // the forward output (GATE), ldy
  float *z;          // the gated gradient (DZ), ldz -- may be g itself
  float *out;        // SUM: the partial rows (nblocks x ldo floats), or the column sums themselves when there is one block
  long long ldg, ldy, ldz, ldo;
  int rows, cols;
  int block_rows;    // R
  int direct;        // 0: out is the workspace; 1: out[j] = s; 2: out[j] = fl(out[j] + s)
};

template <int W>
struct RgVec;
template <>
struct RgVec<4> {
  typedef rg_f32x4 type;
};
template <>
struct RgVec<1> {
  typedef float type;
};

__device__ __forceinline__ float rg_gate(float y, float g) { return y <= 0.0f ? 0.0f : g; }
__device__ __forceinline__ rg_f32x4 rg_gate(rg_f32x4 y, rg_f32x4 g) {
  return rg_f32x4{rg_gate(y[0], g[0]), rg_gate(y[1], g[1]), rg_gate(y[2], g[2]), rg_gate(y[3], g[3])};
}

// Columns [c0, c0 + W) of row block blockIdx.x: nr rows from row r0 on.
template <int W, bool GATE, bool DZ, bool SUM>
__device__ __forceinline__ void rg_walk(const ReluGradArgs &a, int r0, int nr, int c0) {
  typedef typename RgVec<W>::type V;
  // The three row cursors and strides are kept per-lane values (the empty asm statements): left to itself the compiler
  // splits every row's address into a uniform row base in a scalar register pair plus the lane's column, and 3 x 2 U such
  // pairs, or u x stride for every u and operand, do not fit the scalar file -- they spill.
  long long ldg = a.ldg, ldy = a.ldy, ldz = a.ldz;
  long long og = (long long)r0 * ldg + c0, oy = (long long)r0 * ldy + c0, oz = (long long)r0 * ldz + c0;
  MMH_RG_PER_LANE(og, ldg);
  if (GATE) MMH_RG_PER_LANE(oy, ldy);
  if (DZ) MMH_RG_PER_LANE(oz, ldz);
  const float *g = a.g + og;
  const float *y = GATE ? a.y + oy : nullptr;
  float *z = DZ ? a.z + oz : nullptr;
  // whole batches of U rows, the next one loaded before the current one is stored; then the nr % U rows left, as one
  // guarded batch (the only one of a block shorter than U rows)
  V cg[RG_U], cy[RG_U], ng[RG_U], ny[RG_U];
  V acc;
  const int nfull = nr / RG_U, rem = nr - nfull * RG_U;
  if (nfull > 0) {
#pragma unroll
    for (int u = 0; u < RG_U; ++u) {
      cg[u] = *reinterpret_cast<const V *>(g + u * ldg);
      if (GATE) cy[u] = *reinterpret_cast<const V *>(y + u * ldy);
    }
  }
#pragma unroll 1
  for (int b = 0; b < nfull; ++b) {
    g += RG_U * ldg;
    if (GATE) y += RG_U * ldy;
    if (b + 1 < nfull) {
#pragma unroll
      for (int u = 0; u < RG_U; ++u) {
        ng[u] = *reinterpret_cast<const V *>(g + u * ldg);
        if (GATE) ny[u] = *reinterpret_cast<const V *>(y + u * ldy);
      }
    }
#pragma unroll
    for (int u = 0; u < RG_U; ++u) {
      V zv = cg[u];
      if (GATE) zv = rg_gate(cy[u], cg[u]);
      if (DZ) *reinterpret_cast<V *>(z + u * ldz) = zv;
      if (SUM) {
        if (u == 0 && b == 0) acc = zv;      // the chain STARTS at z(bR, j): +0 + (-0) would lose the sign
        else acc += zv;
      }
    }
    if (DZ) z += RG_U * ldz;
    if (b + 1 < nfull) {
#pragma unroll
      for (int u = 0; u < RG_U; ++u) {
        cg[u] = ng[u];
        if (GATE) cy[u] = ny[u];
      }
    }
  }
  if (rem > 0) {
#pragma unroll
    for (int u = 0; u < RG_U - 1; ++u)
      if (u < rem) {
        cg[u] = *reinterpret_cast<const V *>(g + u * ldg);
        if (GATE) cy[u] = *reinterpret_cast<const V *>(y + u * ldy);
      }
#pragma unroll
    for (int u = 0; u < RG_U - 1; ++u)
      if (u < rem) {
        V zv = cg[u];
        if (GATE) zv = rg_gate(cy[u], cg[u]);
        if (DZ) *reinterpret_cast<V *>(z + u * ldz) = zv;
        if (SUM) {
          if (u == 0 && nfull == 0) acc = zv;
          else acc += zv;
        }
      }
  }
  if (SUM) {
    if (a.direct == 0) {
      *reinterpret_cast<V *>(a.out + (size_t)blockIdx.x * a.ldo + c0) = acc;   // the workspace's rows are 16-byte aligned
    } else if constexpr (W == 1) {
      a.out[c0] = a.direct == 2 ? a.out[c0] + acc : acc;
    } else {
#pragma unroll
      for (int i = 0; i < W; ++i) a.out[c0 + i] = a.direct == 2 ? a.out[c0 + i] + acc[i] : acc[i];
    }
  }
}

// W = 4 (every operand's rows 16-byte aligned): the work items are the cols / 4 whole column quads, then the cols % 4 columns
// past them, one thread each on the W = 1 walk.  W = 1: one item per column.
template <int W, bool GATE, bool DZ, bool SUM>
__global__ void __launch_bounds__(RG_THREADS) relu_grad_colsum_kernel(ReluGradArgs a) {
  const int whole = a.cols / W, items = whole + a.cols % W;
  const int r0 = (int)((long long)blockIdx.x * a.block_rows);
  const int nr = a.rows - r0 < a.block_rows ? a.rows - r0 : a.block_rows;   // >= 1: grid.x = ceil(rows / R)
#pragma unroll 1
  for (long long it = (long long)blockIdx.y * RG_THREADS + threadIdx.x; it < items; it += (long long)gridDim.y * RG_THREADS) {
    if (W == 1 || it < whole) rg_walk<W, GATE, DZ, SUM>(a, r0, nr, (int)it * W);
    else rg_walk<1, GATE, DZ, SUM>(a, r0, nr, whole * W + (int)(it - whole));
  }
}

// colsum[j] = p_0[j], then fl(s + p_b[j]) for b = 1 .. nblocks - 1; accumulate: colsum[j] = fl(colsum[j] + s).
// One thread per column (consecutive lanes on consecutive columns), FU partial rows in flight.
constexpr int RG_FIN_THREADS = 64;
constexpr int RG_FU = 16;
__global__ void __launch_bounds__(RG_FIN_THREADS) colsum_finish_kernel(const float *__restrict__ parts, int nblocks, long long ldo, int cols,
                                                                       float *__restrict__ colsum, int accumulate) {
  const long long j = (long long)blockIdx.x * RG_FIN_THREADS + threadIdx.x;
  if (j >= cols) return;
  const float *p = parts + j;
  float s = p[0];
  for (int b = 1; b < nblocks; b += RG_FU) {
    float v[RG_FU];
#pragma unroll
    for (int u = 0; u < RG_FU; ++u)
      if (b + u < nblocks) v[u] = p[(size_t)(b + u) * ldo];
#pragma unroll
    for (int u = 0; u < RG_FU; ++u)
      if (b + u < nblocks) s += v[u];
  }
  colsum[j] = accumulate ? colsum[j] + s : s;
}

}  // namespace mmh
