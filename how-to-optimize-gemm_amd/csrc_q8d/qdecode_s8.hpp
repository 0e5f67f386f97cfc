// qdecode_s8.hpp -- the kernels of libmmult_hip_q8d.so, the int8 linear layer for 1 - 16 rows (include/mmult_hip_q8d.h has the
// contract, tests/qchain_ref.py is its numpy reference, tests/test_gpu_qdecode.py holds both kernels to it bit for bit):
//   qdecode_partial_kernel        grid = column strips x K ranges.  A workgroup streams its 128-column strip of the weight image
//                                 over one contiguous K range exactly once (LDS-DMA, 128-byte k slices in a ring), gathers the
//                                 MFMA's B fragments with the transposing LDS read as K3t does (csrc/igemm_s8.hpp), multiplies
//                                 them against the <= 16 activation rows and writes an int32 block [split][row][column].
//   qdecode_finish_kernel<OUT8>   elementwise over rows x out: the partials of a column added in split order in int32 -- exact
//                                 in any order, so the sum IS the tile path's accumulator --, then QlinearEpilogue's arithmetic
//                                 (csrc_q8/qlinear_s8.hpp) and, with OUT8, q8o's requantisation (csrc_q8o/qlinear_s8o.hpp).
// No atomics, no counters, no state that must be zero: every int32 the finish reads was written by the partial kernel of the
// same call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "igemm_s8.hpp"         // IK, LdsDma, i32x4
#include "quant_rules_s8.hpp"   // quantize_one

namespace mmh {

constexpr int QD_STRIP = 128;    // columns of a workgroup: one 128-byte line of every image row
constexpr int QD_WAVES = 4;      // each 32 columns: two 16-column MFMA tiles
constexpr int QD_STAGES = 2;     // slices of the ring (16 KiB each)
constexpr int QD_ROWS = 16;      // one MFMA row block
constexpr int QD_FINISH_THREADS = 256, QD_FINISH_COLS = 4 * QD_FINISH_THREADS;

// One slice of the ring is the strip's [128 k rows][128 bytes] as it lies in memory; the 16-byte slot of row r is XORed with
// qd_swz(r) on the SOURCE side (K3t's BN = 128 rule: the 16 + 16 pieces a transposing read serves together fall on 16 slots).
__device__ __forceinline__ int qd_swz(int r) { return ((r >> 1) & 3) | (((r >> 4) & 1) << 2); }

// Per wave and slice: 4 LDS-DMA chunks of the weight (1 KiB = 8 image rows each) and 2 register loads of the activations'
// fragments (16 consecutive k of row `lane & 15` per 64-deep MFMA step, straight from global memory: the rows are 2 KiB per slice
// and every wave wants all of them).  Both go through buffer descriptors:
//   weight   base = the strip's first column in the range's first k row; extent = the last valid k row's last strip byte, so
//            rows at or beyond min(range end, in) arrive as ZEROS and fetch nothing;
//   x        extent = the last row's last dword of `in`: rows >= rows arrive as zeros.  Bytes of a row beyond `in` (and the
//            next row's, which an offset past `in` reaches) may hold anything: the weight's zeros multiply them.
// Columns >= out of the last strip read the image's neighbouring bytes and feed accumulators that are never stored.
struct QdecodeLoader {
  static __device__ __forceinline__ void weight(__amdgpu_buffer_rsrc_t rsrc, int8_t *stage, const uint32_t (&voff)[4], int soff) {
    LdsDma<4>::chunks(rsrc, stage, voff, soff);
  }
  static __device__ __forceinline__ i32x4 rows(__amdgpu_buffer_rsrc_t rsrc, uint32_t voff, int soff) {
    return __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, 0));
  }
};

// rows in 1..16, out, in > 0; k_len: the K range's length, a multiple of IK; gridDim = (strips, splits); work: [split][rows][wp]
// int32 with wp = out rounded up to 4 (a lane stores four columns as one vector: the pad columns inside wp are written too).
__global__ void __launch_bounds__(QD_WAVES * 64, 2)
qdecode_partial_kernel(int rows, int out, int in, int k_len, const int8_t *__restrict__ xq, int ldq, const int8_t *__restrict__ wq,
                       int pitch_n, int32_t *__restrict__ work, int wp) {
  constexpr int S = QD_STAGES, STAGE = IK * QD_STRIP;
  constexpr int VM = 6;   // vector-memory operations per wave and slice: 4 chunks + 2 fragment loads, issued in this order
  __shared__ __attribute__((aligned(16))) int8_t ring[S * STAGE];

  const int col0 = blockIdx.x * QD_STRIP, split = blockIdx.y;
  const int k_begin = split * k_len;
  const int kr = min(k_len, in - k_begin);   // valid k rows of this range (> 0: the plan leaves no range empty)
  const int nk = (kr + IK - 1) / IK;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, g = lane >> 4;

  const uint32_t ext_w = (uint32_t)((kr - 1) * pitch_n + ((min(QD_STRIP, out - col0) + 3) & ~3));
  const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<int8_t *>(wq + (size_t)k_begin * pitch_n + col0), 0, ext_w, 0x00020000);
  const uint32_t ext_x = (uint32_t)((rows - 1) * ldq + ((in + 3) & ~3));
  const __amdgpu_buffer_rsrc_t rsrc_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t *>(xq), 0, ext_x, 0x00020000);

  // wave w moves chunks 4 w .. 4 w + 3 of a slice: image rows 32 w .. 32 w + 31, eight lanes per row
  uint32_t voff_w[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = 8 * (4 * wave + j) + (lane >> 3);
    voff_w[j] = (uint32_t)(r * pitch_n + 16 * ((lane & 7) ^ qd_swz(r)));
  }
  const uint32_t voff_x = (uint32_t)(li * ldq + k_begin + 16 * g);
  // this lane's piece of rows 16 g + (li >> 1) of tile u (+ 64 st + 8 h rows as immediates): K3t's bt_off
  uint32_t b_off[2];
  {
    const int r = 16 * g + (li >> 1);
#pragma unroll
    for (int u = 0; u < 2; ++u) b_off[u] = (uint32_t)(r * QD_STRIP + 16 * ((2 * wave + u) ^ qd_swz(r)) + 8 * (li & 1));
  }

  i32x4 xa[S][2], acc[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  // slice kt >= nk: every weight offset lies beyond the extent -- zeros land in LDS, nothing is fetched
  auto issue = [&](auto c_c, int kt) {
    constexpr int C = decltype(c_c)::value;
    QdecodeLoader::weight(rsrc_w, ring + C * STAGE + 4 * wave * 1024, voff_w, kt * IK * pitch_n);
    xa[C][0] = QdecodeLoader::rows(rsrc_x, voff_x, kt * IK);
    xa[C][1] = QdecodeLoader::rows(rsrc_x, voff_x, kt * IK + 64);
    asm volatile("" ::: "memory");   // (the wait below counts whole slices: no operation of the next one moves in front of these)
  };
  static_for<S>([&](auto c) { issue(c, decltype(c)::value); });

  typedef int i32x2 __attribute__((ext_vector_type(2)));
  typedef __attribute__((address_space(3))) i32x2 *lds_v2;
  for (int kt = 0; kt < nk; kt += S) {
    static_for<S>([&](auto c_c) {
      constexpr int C = decltype(c_c)::value;
      // the S - 1 younger slices may still be in flight; this one has landed in every wave's part of the stage
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"((S - 1) * VM) : "memory");
      __syncthreads();
      const int8_t *stage = ring + C * STAGE;
      i32x4 fb[2][2];
#pragma unroll
      for (int st = 0; st < 2; ++st)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const i32x2 lo = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_v2)(stage + b_off[u] + 64 * st * QD_STRIP));
          const i32x2 hi = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_v2)(stage + b_off[u] + (64 * st + 8) * QD_STRIP));
          fb[st][u] = i32x4{lo[0], lo[1], hi[0], hi[1]};
        }
      // operands swapped as in K3t (D = tile^T): the lane holds partial[row li][tile u's columns 4 g .. 4 g + 3]
#pragma unroll
      for (int st = 0; st < 2; ++st)
#pragma unroll
        for (int u = 0; u < 2; ++u) acc[u] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fb[st][u], xa[C][st], acc[u], 0, 0, 0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __syncthreads();   // every wave has read this stage: the slice S ahead may land in it
      issue(c_c, kt + C + S);
    });
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the trailing slices are zeros, but they do land in LDS)

  if (li < rows) {
    int32_t *at = work + ((size_t)split * rows + li) * wp;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int col = col0 + 32 * wave + 16 * u + 4 * g;
      if (col < out) *reinterpret_cast<i32x4 *>(at + col) = acc[u];   // (col + 3 < wp)
    }
  }
}

// gridDim = (ceil(out / 1024), rows); a thread owns four consecutive columns of one row.  splits == 0 (in == 0): acc = 0, `work`
// is not read.  `wide`: the output's base and pitch allow one 16-byte (fp32) or 4-byte (int8) store per thread where its four
// columns are inside `out`; otherwise element by element -- the same bits.
template <bool OUT8>
__global__ void __launch_bounds__(QD_FINISH_THREADS)
qdecode_finish_kernel(int rows, int out, int splits, const int32_t *__restrict__ work, int wp, const float *__restrict__ rx,
                      const float *__restrict__ rw, const float *__restrict__ bias, int relu, const float *__restrict__ so,
                      void *__restrict__ y, int ldo, int wide) {
#pragma clang fp contract(off)
  const int row = blockIdx.y, col = 4 * (blockIdx.x * QD_FINISH_THREADS + threadIdx.x);
  if (col >= out) return;
  i32x4 acc = {0, 0, 0, 0};
  for (int s = 0; s < splits; ++s) acc += *reinterpret_cast<const i32x4 *>(work + ((size_t)s * rows + row) * wp + col);
  const float r = rx[row];
  const float sc = OUT8 ? so[row] : 0.0f;
  const bool whole = col + 3 < out;
  float f[4];
  int q[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const bool in = whole || col + u < out;
    // plain operators under the pragma: each line rounds once (QlinearEpilogue's three roundings)
    float v = (float)acc[u] * r;
    v = v * (in ? rw[col + u] : 0.0f);
    if (bias) v = v + (in ? bias[col + u] : 0.0f);
    if (relu) v = !(v <= 0.0f) ? v : 0.0f;   // (NaN: not <= 0, stays)
    f[u] = v;
    if (OUT8) q[u] = quantize_one(v, sc);
  }
  if constexpr (OUT8) {
    int8_t *at = static_cast<int8_t *>(y) + (size_t)row * ldo + col;
    if (wide && whole) {
      *reinterpret_cast<uint32_t *>(at) = (unsigned)(q[0] & 255) | ((unsigned)(q[1] & 255) << 8) | ((unsigned)(q[2] & 255) << 16) |
                                          ((unsigned)(q[3] & 255) << 24);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (whole || col + u < out) at[u] = (int8_t)q[u];
    }
  } else {
    float *at = static_cast<float *>(y) + (size_t)row * ldo + col;
    if (wide && whole) {
      typedef float f32x4_t __attribute__((ext_vector_type(4)));
      *reinterpret_cast<f32x4_t *>(at) = f32x4_t{f[0], f[1], f[2], f[3]};
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (whole || col + u < out) at[u] = f[u];
    }
  }
}

}  // namespace mmh
