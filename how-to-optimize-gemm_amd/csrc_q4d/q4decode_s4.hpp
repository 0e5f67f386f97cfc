// q4decode_s4.hpp -- the kernels of libmmult_hip_q4d.so that are its own (include/mmult_hip_q4d.h has the contract,
// tests/q4_ref.py its numpy restatement, tests/test_gpu_q4decode.py holds them to it bit for bit):
//   q4decode_partial_kernel     csrc_q8d/qdecode_s8.hpp's qdecode_partial_kernel on the PACKED image: grid = column strips x K
//                               ranges, 4 waves of 32 columns, the LDS-DMA ring, counted vmcnt waits, descriptor extents instead
//                               of an EDGE twin.  A 128-k slice of a strip is [64 packed rows][128 bytes] = 8 KiB; the
//                               transposing LDS read over those 64 rows hands each lane bytes whose LOW nibbles are the B
//                               fragment of k 0 .. 63 and whose HIGH nibbles are the fragment of k 64 .. 127.  The activation
//                               fragments, their descriptor and their k order are qdecode_partial_kernel's.
//   q4_row_amax_kernel,
//   q4_pack_weight_kernel       mmh_q4d_pack_weight: preparation, not the hot path.
// The finish kernel is qdecode_finish_kernel<OUT8> of qdecode_s8.hpp, instantiated in this library as it stands.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// qdecode_s8.hpp defines the int8 partial kernel as a plain __global__ function, and a plain kernel lands in every library
// whose translation unit sees it.  This library launches none: for the length of the include its name stands for "a kernel
// that is declared and never defined; then a template nobody instantiates", so the header is read as it stands and nothing of
// that kernel is emitted (tests/test_q4d_kernel_census.py holds the library to its five kernels).
#define qdecode_partial_kernel                                                                 \
  q4d_never_defined_kernel();                                                                  \
  template <class Q4NeverInstantiated> __global__ void __launch_bounds__(QD_WAVES * 64, 2) qdecode_partial_kernel_in_q8d_only
#include "qdecode_s8.hpp"       // QD_*, qd_swz, QdecodeLoader's rows, qdecode_finish_kernel; igemm_s8.hpp's IK, LdsDma, i32x4
#undef qdecode_partial_kernel
#include "quant_rules_s4.hpp"   // scale4_of_amax, quantize4_one

namespace mmh {

constexpr int Q4_STAGES = 2;           // slices of the ring (8 KiB each)
constexpr int Q4_SLICE_ROWS = IK / 2;  // packed rows of a 128-k slice

// Nibbles to int8 without a per-byte sign extension: a two's-complement nibble in a byte's HIGH half is that byte's signed
// value divided by 16 (-8 -> 0x80 = -128 = 16 * -8).  Of a dword v of packed bytes
//   v & 0xF0F0F0F0          is the int8 vector 16 * W_hi,
//   (v << 4) & 0xF0F0F0F0   is the int8 vector 16 * W_lo (what the shift carries into a byte's low half from its neighbour is
//                           masked away),
// so the accumulator holds exactly 16 * sum x W and `acc >> 4` (arithmetic) is the sum.  tests/test_q4_ref.py holds the
// identity for all 256 byte values.
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ i32x4 q4_lo16(u32x4 v) { return __builtin_bit_cast(i32x4, (v << 4) & 0xF0F0F0F0u); }
__device__ __forceinline__ i32x4 q4_hi16(u32x4 v) { return __builtin_bit_cast(i32x4, v & 0xF0F0F0F0u); }

// rows in 1..16, out, in > 0; k_len: the K range's length, a multiple of IK and at most 65536 (the accumulator holds 16 x the
// sum: |16 x W| <= 2^14 per k); gridDim = (strips, splits); work: [split][rows][wp] int32 with wp = out rounded up to 4.
// Per wave and slice: 2 LDS-DMA chunks of the packed image (1 KiB = 8 packed rows each) and 2 register loads of the
// activations' fragments.  The weight's descriptor: base = the strip's first column in the range's first packed row; extent =
// the range's last packed row's last strip byte (the image holds whole slices: the nibbles of k >= in are zeros IN it), so
// packed rows at or beyond min(range end, image end) arrive as ZEROS and fetch nothing.
__global__ void __launch_bounds__(QD_WAVES * 64, 2)
q4decode_partial_kernel(int rows, int out, int in, int k_len, const int8_t *__restrict__ xq, int ldq, const uint8_t *__restrict__ wp4,
                        int pitch_n, int32_t *__restrict__ work, int wp) {
  constexpr int S = Q4_STAGES, STAGE = Q4_SLICE_ROWS * QD_STRIP;
  constexpr int VM = 4;   // vector-memory operations per wave and slice: 2 chunks + 2 fragment loads, issued in this order
  __shared__ __attribute__((aligned(16))) int8_t ring[S * STAGE];

  const int col0 = blockIdx.x * QD_STRIP, split = blockIdx.y;
  const int k_begin = split * k_len;
  const int kr = min(k_len, in - k_begin);   // valid k of this range (> 0: the plan leaves no range empty)
  const int nk = (kr + IK - 1) / IK;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, g = lane >> 4;

  const uint32_t ext_w = (uint32_t)((nk * Q4_SLICE_ROWS - 1) * pitch_n + ((min(QD_STRIP, out - col0) + 3) & ~3));
  const __amdgpu_buffer_rsrc_t rsrc_w = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<uint8_t *>(wp4 + (size_t)(k_begin / 2) * pitch_n + col0), 0, ext_w, 0x00020000);
  const uint32_t ext_x = (uint32_t)((rows - 1) * ldq + ((in + 3) & ~3));
  const __amdgpu_buffer_rsrc_t rsrc_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t *>(xq), 0, ext_x, 0x00020000);

  // wave w moves chunks 2 w, 2 w + 1 of a slice: packed rows 16 w .. 16 w + 15, eight lanes per row
  uint32_t voff_w[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int r = 8 * (2 * wave + j) + (lane >> 3);
    voff_w[j] = (uint32_t)(r * pitch_n + 16 * ((lane & 7) ^ qd_swz(r)));
  }
  const uint32_t voff_x = (uint32_t)(li * ldq + k_begin + 16 * g);
  // this lane's piece of packed rows 16 g + (li >> 1) of tile u (+ 8 rows as an immediate): qdecode_partial_kernel's b_off
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
    LdsDma<2>::chunks(rsrc_w, ring + C * STAGE + 2 * wave * 1024, voff_w, kt * Q4_SLICE_ROWS * pitch_n);
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
      u32x4 v[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const i32x2 lo = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_v2)(stage + b_off[u]));
        const i32x2 hi = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_v2)(stage + b_off[u] + 8 * QD_STRIP));
        v[u] = u32x4{(unsigned)lo[0], (unsigned)lo[1], (unsigned)hi[0], (unsigned)hi[1]};
      }
      // operands swapped as in K3t (D = tile^T): the lane holds 16 x partial[row li][tile u's columns 4 g .. 4 g + 3]
#pragma unroll
      for (int u = 0; u < 2; ++u) acc[u] = __builtin_amdgcn_mfma_i32_16x16x64_i8(q4_lo16(v[u]), xa[C][0], acc[u], 0, 0, 0);
#pragma unroll
      for (int u = 0; u < 2; ++u) acc[u] = __builtin_amdgcn_mfma_i32_16x16x64_i8(q4_hi16(v[u]), xa[C][1], acc[u], 0, 0, 0);
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
      if (col < out) *reinterpret_cast<i32x4 *>(at + col) = acc[u] >> 4;   // (exact: every term is a multiple of 16; col + 3 < wp)
    }
  }
}

// ---- mmh_q4d_pack_weight ---------------------------------------------------------------------------------------------------
// One workgroup per output channel: the abs-max of its `in` finite elements, then s4 and fl(1 / s4).  in == 0: 1 and 1.
__global__ void __launch_bounds__(256) q4_row_amax_kernel(const float *__restrict__ W, int in, int ldw, float *__restrict__ scale,
                                                          float *__restrict__ inv_scale) {
  __shared__ float part[4];
  const int j = blockIdx.x;
  float best = 0.0f;
  for (int k = threadIdx.x; k < in; k += 256) best = fmaxf(best, finite_abs(W[(size_t)j * ldw + k]));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) best = fmaxf(best, __shfl_xor(best, off, 64));
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float s = scale4_of_amax(fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3])));
    scale[j] = s;
    inv_scale[j] = __fdiv_rn(1.0f, s);
  }
}

// 64 channels x one 128-k slice per workgroup: fp32 rows read along k, both halves of the slice quantised with the channel's
// scale and packed into one byte, turned in LDS, written as 64 packed rows of 64 bytes along the channels.  Channels
// [out, pitch) and nibbles of k >= in are written as 0.  grid (slices, pitch / 64 rounded up), 256 threads; pitch % 16 == 0.
constexpr int Q4_PW_TILE = 64, Q4_PW_PITCH = Q4_PW_TILE + 16;
__global__ void __launch_bounds__(256) q4_pack_weight_kernel(const float *__restrict__ W, int out, int in, int ldw,
                                                             const float *__restrict__ sw, uint8_t *__restrict__ img, int pitch) {
  __shared__ __attribute__((aligned(16))) uint8_t turned[Q4_PW_TILE][Q4_PW_PITCH];   // [packed row][channel]
  const int j0 = blockIdx.y * Q4_PW_TILE, k0 = blockIdx.x * IK;
  const int tid = threadIdx.x, tj = tid >> 4, tk = 4 * (tid & 15);
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int jj = tj + 16 * p, j = j0 + jj;
    int q[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    if (j < out) {
      const float s = sw[j];
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int k = k0 + Q4_SLICE_ROWS * h + tk + u;
          if (k < in) q[h][u] = quantize4_one(W[(size_t)j * ldw + k], s);
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) turned[tk + u][jj] = (uint8_t)((q[0][u] & 15) | ((q[1][u] & 15) << 4));
  }
  __syncthreads();
  const int rr = tid >> 2, seg = 16 * (tid & 3);
  if (j0 + seg < pitch)   // (pitch is a multiple of 16: a segment lies inside it or outside it)
    *reinterpret_cast<i32x4 *>(img + ((size_t)blockIdx.x * Q4_SLICE_ROWS + rr) * pitch + j0 + seg) =
        *reinterpret_cast<const i32x4 *>(&turned[rr][seg]);
}

}  // namespace mmh
