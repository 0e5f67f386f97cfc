// q4gdecode_s4.hpp -- the kernels of libmmult_hip_q4g.so (include/mmult_hip_q4g.h has the contract, tests/q4g_ref.py its numpy
// restatement, tests/test_gpu_q4gdecode.py holds them to it bit for bit):
//   q4gdecode_partial_kernel      csrc_q4d/q4decode_s4.hpp's q4decode_partial_kernel with ONE SCALE PER 128-k SLICE: the same grid
//                                 (column strips x K ranges), the same four waves of 32 columns, the same two-stage 8 KiB LDS-DMA
//                                 ring of the packed image, the same transposing LDS reads.  Per slice the int32 accumulators
//                                 start from zero; the slice's exact sum is converted, multiplied by the group's factor and added
//                                 into fp32 running sums, in ascending slice order.
//   q4gdecode_finish_kernel<OUT8> csrc_q8d/qdecode_s8.hpp's qdecode_finish_kernel on fp32 partials: added in range order, then the
//                                 two-rounding epilogue.
//   q4g_pack_weight_kernel        mmh_q4g_pack_weight: preparation, not the hot path.
// Every fp32 operation of the contract is a plain operator under `fp contract(off)`: a multiply, then an add, never an fma.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// qdecode_s8.hpp defines the int8 partial kernel as a plain __global__ function, and a plain kernel lands in every library
// whose translation unit sees it.  This library launches none: csrc_q4d/q4decode_s4.hpp's way round it (which itself is not
// included -- its three kernels are plain too; the two one-line nibble helpers are restated below).
#define qdecode_partial_kernel                                                                 \
  q4g_never_defined_kernel();                                                                  \
  template <class Q4gNeverInstantiated> __global__ void __launch_bounds__(QD_WAVES * 64, 2) qdecode_partial_kernel_in_q8d_only
#include "qdecode_s8.hpp"       // QD_*, qd_swz, QdecodeLoader's rows; igemm_s8.hpp's IK, LdsDma, i32x4; quantize_one
#undef qdecode_partial_kernel
#include "quant_rules_s4.hpp"   // scale4_of_amax, quantize4_one

#pragma clang fp contract(off)   // (file scope: every kernel below, their lambdas included)

namespace mmh {

constexpr int Q4G_STAGES = 2;           // slices of the ring (8 KiB each)
constexpr int Q4G_SLICE_ROWS = IK / 2;  // packed rows of a 128-k slice = of a group

typedef unsigned q4g_u32x4 __attribute__((ext_vector_type(4)));
typedef float q4g_f32x4 __attribute__((ext_vector_type(4)));
// q4decode_s4.hpp's q4_lo16 / q4_hi16: the int8 vectors 16 * W_lo and 16 * W_hi of a dword of packed bytes
__device__ __forceinline__ i32x4 q4g_lo16(q4g_u32x4 v) { return __builtin_bit_cast(i32x4, (v << 4) & 0xF0F0F0F0u); }
__device__ __forceinline__ i32x4 q4g_hi16(q4g_u32x4 v) { return __builtin_bit_cast(i32x4, v & 0xF0F0F0F0u); }

// rows in 1..16, out, in > 0; k_len: the K range's length, a multiple of IK; gridDim = (strips, splits); gs: the groups' factors
// r[g][j], rows of pitch_s floats (pitch_s % 4 == 0, gs 16-byte aligned); work: [split][rows][wp] FP32 with wp = out rounded up
// to 4.  Per wave and slice SIX vector-memory operations, issued in this order: 2 LDS-DMA chunks of the packed image, 2 register
// loads of the activations' fragments, 2 register loads of the slice's factors -- the lane's columns 4 g .. 4 g + 3 of tile u are
// 16 consecutive bytes of the group's row.  Three descriptors:
//   weight   q4decode_partial_kernel's: packed rows at or beyond min(range end, image end) arrive as ZEROS;
//   x        its: rows >= rows arrive as zeros;
//   factors  base = the strip's first column in the range's first group row; extent = the range's LAST group row's last strip
//            float (rounded up to 4 floats).  The slice's row offset travels in the VECTOR offset, which the range check covers.
// Computing past a range's end.  The loop computes nk rounded up to the ring depth, and the ring requests up to three slices
// beyond nk.  Their weights are zeros (S = 0).  Their factors must not be read: in a range that is not the last, the group row
// behind its end is the NEXT range's first, a real one, and 0 * inf or 0 * NaN there would poison this range's partial.  The
// factors' extent ends with the range, so such a row arrives as +0: t = fl(0 * 0) = +0.  The running sum P starts at +0, and a
// round-to-nearest sum is -0 only when both terms are -0, so P is never -0 and fl(P + (+0)) = P bit for bit: the surplus terms
// are harmless, and the result is the contract's chain over the range's real groups only.
__global__ void __launch_bounds__(QD_WAVES * 64, 2)
q4gdecode_partial_kernel(int rows, int out, int in, int k_len, const int8_t *__restrict__ xq, int ldq, const uint8_t *__restrict__ wp4,
                         int pitch_n, const float *__restrict__ gs, int pitch_s, float *__restrict__ work, int wp) {
  constexpr int S = Q4G_STAGES, STAGE = Q4G_SLICE_ROWS * QD_STRIP;
  constexpr int VM = 6;   // vector-memory operations per wave and slice: 2 chunks + 2 fragment loads + 2 factor loads
  __shared__ __attribute__((aligned(16))) int8_t ring[S * STAGE];

  const int col0 = blockIdx.x * QD_STRIP, split = blockIdx.y;
  const int k_begin = split * k_len;
  const int kr = min(k_len, in - k_begin);   // valid k of this range (> 0: the plan leaves no range empty)
  const int nk = (kr + IK - 1) / IK;         // its slices = its groups
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, g = lane >> 4;
  const int cols4 = (min(QD_STRIP, out - col0) + 3) & ~3;

  const uint32_t ext_w = (uint32_t)((nk * Q4G_SLICE_ROWS - 1) * pitch_n + cols4);
  const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t *>(wp4 + (size_t)(k_begin / 2) * pitch_n + col0), 0, ext_w, 0x00020000);
  const uint32_t ext_x = (uint32_t)((rows - 1) * ldq + ((in + 3) & ~3));
  const __amdgpu_buffer_rsrc_t rsrc_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t *>(xq), 0, ext_x, 0x00020000);
  const uint32_t ext_s = (uint32_t)(((nk - 1) * pitch_s + cols4) * 4);   // (a multiple of 16: a lane's vector is inside or outside)
  const __amdgpu_buffer_rsrc_t rsrc_s = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(gs + (size_t)(k_begin / IK) * pitch_s + col0), 0, ext_s, 0x00020000);

  // wave w moves chunks 2 w, 2 w + 1 of a slice: packed rows 16 w .. 16 w + 15, eight lanes per row
  uint32_t voff_w[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int r = 8 * (2 * wave + j) + (lane >> 3);
    voff_w[j] = (uint32_t)(r * pitch_n + 16 * ((lane & 7) ^ qd_swz(r)));
  }
  const uint32_t voff_x = (uint32_t)(li * ldq + k_begin + 16 * g);
  const uint32_t voff_s = (uint32_t)((32 * wave + 4 * g) * 4);   // tile 0's four columns; tile 1's are 64 bytes further
  // this lane's piece of packed rows 16 g + (li >> 1) of tile u (+ 8 rows as an immediate): qdecode_partial_kernel's b_off
  uint32_t b_off[2];
  {
    const int r = 16 * g + (li >> 1);
#pragma unroll
    for (int u = 0; u < 2; ++u) b_off[u] = (uint32_t)(r * QD_STRIP + 16 * ((2 * wave + u) ^ qd_swz(r)) + 8 * (li & 1));
  }

  i32x4 xa[S][2];
  q4g_f32x4 sc[S][2], sum[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  // slice kt >= nk: every weight and factor offset lies beyond its extent -- zeros arrive, nothing is fetched
  auto issue = [&](auto c_c, int kt) {
    constexpr int C = decltype(c_c)::value;
    LdsDma<2>::chunks(rsrc_w, ring + C * STAGE + 2 * wave * 1024, voff_w, kt * Q4G_SLICE_ROWS * pitch_n);
    xa[C][0] = QdecodeLoader::rows(rsrc_x, voff_x, kt * IK);
    xa[C][1] = QdecodeLoader::rows(rsrc_x, voff_x, kt * IK + 64);
    const uint32_t row = voff_s + (uint32_t)(kt * pitch_s * 4);
    sc[C][0] = __builtin_bit_cast(q4g_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_s, row, 0, 0));
    sc[C][1] = __builtin_bit_cast(q4g_f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_s, row + 64, 0, 0));
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
      q4g_u32x4 v[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const i32x2 lo = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_v2)(stage + b_off[u]));
        const i32x2 hi = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_v2)(stage + b_off[u] + 8 * QD_STRIP));
        v[u] = q4g_u32x4{(unsigned)lo[0], (unsigned)lo[1], (unsigned)hi[0], (unsigned)hi[1]};
      }
      // operands swapped as in K3t (D = tile^T): the lane holds 16 x S_g[row li][tile u's columns 4 g .. 4 g + 3], from zero
      i32x4 acc[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) acc[u] = __builtin_amdgcn_mfma_i32_16x16x64_i8(q4g_lo16(v[u]), xa[C][0], i32x4{0, 0, 0, 0}, 0, 0, 0);
#pragma unroll
      for (int u = 0; u < 2; ++u) acc[u] = __builtin_amdgcn_mfma_i32_16x16x64_i8(q4g_hi16(v[u]), xa[C][1], acc[u], 0, 0, 0);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const q4g_f32x4 t = __builtin_convertvector(acc[u] >> 4, q4g_f32x4) * sc[C][u];   // (exact shift, exact conversion; one rounding)
        sum[u] = sum[u] + t;                                                                // (one rounding; never an fma)
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __syncthreads();   // every wave has read this stage: the slice S ahead may land in it
      issue(c_c, kt + C + S);
    });
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the trailing slices are zeros, but they do land in LDS)

  if (li < rows) {
    float *at = work + ((size_t)split * rows + li) * wp;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int col = col0 + 32 * wave + 16 * u + 4 * g;
      if (col < out) *reinterpret_cast<q4g_f32x4 *>(at + col) = sum[u];   // (col + 3 < wp)
    }
  }
}

// gridDim = (ceil(out / 1024), rows); a thread owns four consecutive columns of one row.  splits == 0 (in == 0): Z = 0, `work` is
// not read.  `wide`: qdecode_finish_kernel's -- one 16-byte (fp32) or 4-byte (int8) store per thread where its four columns are
// inside `out`; otherwise element by element, the same bits.
template <bool OUT8>
__global__ void __launch_bounds__(QD_FINISH_THREADS)
q4gdecode_finish_kernel(int rows, int out, int splits, const float *__restrict__ work, int wp, const float *__restrict__ rx,
                        const float *__restrict__ bias, int relu, const float *__restrict__ so, void *__restrict__ y, int ldo, int wide) {
  const int row = blockIdx.y, col = 4 * (blockIdx.x * QD_FINISH_THREADS + threadIdx.x);
  if (col >= out) return;
  q4g_f32x4 z = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < splits; ++s) z = z + *reinterpret_cast<const q4g_f32x4 *>(work + ((size_t)s * rows + row) * wp + col);   // range order
  const float r = rx[row];
  const float sc = OUT8 ? so[row] : 0.0f;
  const bool whole = col + 3 < out;
  float f[4];
  int q[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const bool in = whole || col + u < out;
    // plain operators under the pragma: each line rounds once (two roundings: the channel's factor is in the groups')
    float v = z[u] * r;
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
      *reinterpret_cast<q4g_f32x4 *>(at) = q4g_f32x4{f[0], f[1], f[2], f[3]};
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (whole || col + u < out) at[u] = f[u];
    }
  }
}

// ---- mmh_q4g_pack_weight ---------------------------------------------------------------------------------------------------
// csrc_q4d/q4decode_s4.hpp's q4_pack_weight_kernel with the abs-max inside: 64 channels x one 128-k slice (= one group) per
// workgroup.  The 16 threads that share a channel hold its group, eight elements each: the group's abs-max over its finite
// elements is a reduction over those 16 lanes; then s4, fl(1 / s4), both halves of the slice quantised with it and packed into
// one byte, turned in LDS, written as 64 packed rows of 64 bytes along the channels.  Image channels [out, pitch) and nibbles of
// k >= in are written as 0, scale columns [out, pitch_s) as 0.  grid (slices, max(pitch, pitch_s) / 64 rounded up), 256 threads;
// pitch % 16 == 0.
constexpr int Q4G_PW_TILE = 64, Q4G_PW_PITCH = Q4G_PW_TILE + 16;
__global__ void __launch_bounds__(256) q4g_pack_weight_kernel(const float *__restrict__ W, int out, int in, int ldw,
                                                              uint8_t *__restrict__ img, int pitch, float *__restrict__ gscale,
                                                              float *__restrict__ ginv, int pitch_s) {
  __shared__ __attribute__((aligned(16))) uint8_t turned[Q4G_PW_TILE][Q4G_PW_PITCH];   // [packed row][channel]
  const int j0 = blockIdx.y * Q4G_PW_TILE, k0 = blockIdx.x * IK;
  const int tid = threadIdx.x, tj = tid >> 4, tk = 4 * (tid & 15);
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int jj = tj + 16 * p, j = j0 + jj;
    float w[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    float best = 0.0f;
    if (j < out) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k = k0 + Q4G_SLICE_ROWS * h + tk + u;
          if (k < in) {
            w[h][u] = W[(size_t)j * ldw + k];
            best = fmaxf(best, finite_abs(w[h][u]));
          }
        }
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) best = fmaxf(best, __shfl_xor(best, off, 64));   // (the channel's 16 lanes)
    const float s = scale4_of_amax(best);
    if ((tid & 15) == 0 && j < pitch_s) {
      gscale[(size_t)blockIdx.x * pitch_s + j] = j < out ? s : 0.0f;
      ginv[(size_t)blockIdx.x * pitch_s + j] = j < out ? __fdiv_rn(1.0f, s) : 0.0f;
    }
    int q[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    if (j < out) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (k0 + Q4G_SLICE_ROWS * h + tk + u < in) q[h][u] = quantize4_one(w[h][u], s);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) turned[tk + u][jj] = (uint8_t)((q[0][u] & 15) | ((q[1][u] & 15) << 4));
  }
  __syncthreads();
  const int rr = tid >> 2, seg = 16 * (tid & 3);
  if (j0 + seg < pitch)   // (pitch is a multiple of 16: a segment lies inside it or outside it)
    *reinterpret_cast<i32x4 *>(img + ((size_t)blockIdx.x * Q4G_SLICE_ROWS + rr) * pitch + j0 + seg) =
        *reinterpret_cast<const i32x4 *>(&turned[rr][seg]);
}

}  // namespace mmh
