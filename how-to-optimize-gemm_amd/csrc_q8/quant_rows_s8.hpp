// quant_rows_s8.hpp -- the memory-bound kernels of libmmult_hip_q8.so (include/mmult_hip_q8.h has the contract,
// tests/qlinear_ref.py restates it, tests/test_gpu_qlinear.py holds both to it bit for bit):
//   quantize_rows_s8_kernel<WIDE>   one scale PER ROW of an fp32 matrix: the int8 row, its scale and the scale's reciprocal in
//                                   one pass over HBM -- the row waits in LDS between the abs-max and the quantise
//   prepare_weight_s8_kernel        a torch-layout weight (out x in fp32) -> its int8 image TRANSPOSED (in x pitch), quantised per
//                                   output channel with the scales quantize_rows_s8_kernel found (run without an image: scales only)
// The rules per element are csrc/quant_rules_s8.hpp's, shared with the per-tensor passes.  Included by q8.hip only (the second
// kernel is no template).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "igemm_s8.hpp"          // i32x4
#include "quant_rules_s8.hpp"

namespace mmh {

// ---- the row quantiser -----------------------------------------------------------------------------------------------------
constexpr int QR_WAVE_COLS = 1024;     // rows of fewer columns take a wave each (four rows per workgroup), wider ones a workgroup
constexpr int QR_LDS_FLOATS = 16380;   // floats of a wide row that wait in LDS (with the partial maxima: 64 KiB, no opt-in); a longer row's rest is read again (L2)

struct RowQuantArgs {
  const float *x;   // rows x cols, leading dimension ldx
  int rows, cols, ldx;
  int8_t *q;        // the int8 image, leading dimension ldq; columns [cols, pad_to) are written as 0.  NULL: scales only
  int ldq, pad_to;
  float *s, *r;     // per row: the scale and fl(1 / scale)
  int vec;          // quant_vec_ok's test: x 16-byte aligned, ldx % 4 == 0, q dword aligned, ldq % 4 == 0 -> 16-byte loads
};
inline size_t row_quant_lds(bool wide, int cols) {
  const int keep = wide ? (cols < QR_LDS_FLOATS ? (cols + 3) & ~3 : QR_LDS_FLOATS) : 4 * QR_WAVE_COLS;
  return (size_t)keep * sizeof(float) + 16;   // + the waves' partial maxima
}

// G lanes walk one row twice: loads (each kept in LDS at its own index: a lane reads back what it wrote, so only the maximum
// needs a barrier) and the abs-max; then the scale, and the quantised row from the copy in LDS.  No atomics, no abs-max words.
template <bool WIDE>
__global__ void __launch_bounds__(256) quantize_rows_s8_kernel(RowQuantArgs a) {
  extern __shared__ __attribute__((aligned(16))) float qr_lds[];
  constexpr int G = WIDE ? 256 : 64;
  const int lane = WIDE ? threadIdx.x : (threadIdx.x & 63), sub = WIDE ? 0 : (threadIdx.x >> 6);
  const int row = WIDE ? blockIdx.x : 4 * blockIdx.x + sub;
  const int cap = WIDE ? QR_LDS_FLOATS : QR_WAVE_COLS;
  float *keep = qr_lds + (WIDE ? 0 : sub * QR_WAVE_COLS);
  if (row >= a.rows) return;   // (a whole wave of the narrow form; the wide form has a workgroup per row)
  const float *xr = a.x + (size_t)row * a.ldx;
  const int c4 = a.vec ? a.cols / 4 : 0;   // float4s of the row; the columns behind them (all, on the scalar path) go one by one
  float best = 0.0f;
#pragma unroll 4
  for (int i = lane; i < c4; i += G) {
    const qf32x4 v = *reinterpret_cast<const qf32x4 *>(xr + 4 * i);
    best = fmaxf(best, abs4(v));
    if (4 * i < cap) *reinterpret_cast<qf32x4 *>(keep + 4 * i) = v;
  }
#pragma unroll 4
  for (int c = 4 * c4 + lane; c < a.cols; c += G) {
    const float v = xr[c];
    best = fmaxf(best, finite_abs(v));
    if (c < cap) keep[c] = v;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) best = fmaxf(best, __shfl_xor(best, off, 64));
  if constexpr (WIDE) {
    float *part = qr_lds + (a.cols < QR_LDS_FLOATS ? (a.cols + 3) & ~3 : QR_LDS_FLOATS);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
    best = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
  }
  const float scale = scale_of_amax(best);
  if (lane == 0) {
    a.s[row] = scale;
    a.r[row] = __fdiv_rn(1.0f, scale);
  }
  if (!a.q) return;
  int8_t *qr = a.q + (size_t)row * a.ldq;
  for (int i = lane; i < c4; i += G) {
    const qf32x4 v = 4 * i < cap ? *reinterpret_cast<const qf32x4 *>(keep + 4 * i) : *reinterpret_cast<const qf32x4 *>(xr + 4 * i);
    *reinterpret_cast<unsigned *>(qr + 4 * i) = quantize4(v, scale);
  }
  for (int c = 4 * c4 + lane; c < a.cols; c += G) qr[c] = (int8_t)quantize_one(c < cap ? keep[c] : xr[c], scale);
  for (int c = a.cols + lane; c < a.pad_to; c += G) qr[c] = 0;
}

// ---- the weight image ------------------------------------------------------------------------------------------------------
// A 64 (channels) x 64 (k) tile of W per workgroup: fp32 rows read along k, quantised with the channel's scale, turned in LDS,
// written as 64 image rows of 64 bytes along the channels.  Channels [out, pitch) of the image are written as 0; `vec`: W
// 16-byte aligned and ldw % 4 == 0.  grid (pitch / 64 rounded up, in / 64 rounded up), 256 threads.
constexpr int PW_TILE = 64, PW_PITCH = PW_TILE + 16;
__global__ void __launch_bounds__(256) prepare_weight_s8_kernel(const float *__restrict__ W, int out, int in, int ldw,
                                                                const float *__restrict__ sw, int8_t *__restrict__ img, int pitch,
                                                                int vec) {
  __shared__ __attribute__((aligned(16))) int8_t turned[PW_TILE][PW_PITCH];   // [k][channel]
  const int j0 = blockIdx.x * PW_TILE, k0 = blockIdx.y * PW_TILE;
  const int tid = threadIdx.x, tj = tid >> 4, tk = 4 * (tid & 15);
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int jj = tj + 16 * p, j = j0 + jj;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float s = 1.0f;
    if (j < out) {
      const float *row = W + (size_t)j * ldw + k0 + tk;
      if (vec && k0 + tk + 3 < in) {
        const qf32x4 f = *reinterpret_cast<const qf32x4 *>(row);
        v[0] = f[0], v[1] = f[1], v[2] = f[2], v[3] = f[3];
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (k0 + tk + u < in) v[u] = row[u];
      }
      s = sw[j];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) turned[tk + u][jj] = (int8_t)quantize_one(v[u], s);
  }
  __syncthreads();
  const int kk = tid >> 2, seg = 16 * (tid & 3);
  if (k0 + kk < in && j0 + seg < pitch)   // (pitch is a multiple of 16: a segment lies inside it or outside it)
    *reinterpret_cast<i32x4 *>(img + (size_t)(k0 + kk) * pitch + j0 + seg) = *reinterpret_cast<const i32x4 *>(&turned[kk][seg]);
}

}  // namespace mmh
