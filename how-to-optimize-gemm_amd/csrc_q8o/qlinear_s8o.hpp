// qlinear_s8o.hpp -- the GEMM of libmmult_hip_q8o.so, the int8 linear layer with an int8 OUTPUT (include/mmult_hip_q8o.h has
// the contract, tests/qchain_ref.py restates it in numpy, tests/test_gpu_qchain.py holds every instantiation to it bit for bit):
//   qlinear_s8o_kernel<BM,BN,TM,EDGE>   igemm_s8_dma_tile (csrc/igemm_s8.hpp, K3t) with a requantising epilogue behind its C
//                                       transposer that stores its row vectors itself: one dword of four int8 per lane
// Both operands are what libmmult_hip_q8.so makes: rows of quantize_rows, the weight image of mmh_q8_weight_info.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "igemm_s8.hpp"
#include "quant_rules_s8.hpp"

namespace mmh {

// Behind the transposer a lane holds four consecutive columns of one row:
//   y  = act(fl(fl(fl((float)acc * rx[row]) * rw[col]) + bias[col]))      qlinear_s8.hpp's three roundings, nothing contracted
//   yq = quantize_one(y, so[row])                                          one more rounding, then rint and the clamp
// Bias and ReLU are arguments, wave-uniform branches: a quantised zero has no sign, so "no bias: no sum" and "add +0" give
// the same bytes and there is nothing for a template parameter to keep apart.  The four bytes leave as one dword where the
// plan says so (`dwords`: yq's base and pitch are multiples of 4) and the lane's columns are all inside n, else byte by byte:
// a quarter-wave writes 64 contiguous bytes of a row.  A guarded instantiation reads none of rx, rw, bias, so at or beyond
// m / n and writes nothing outside rows x out bytes.
template <bool EDGE>
struct QlinearS8oEpilogue {
  static constexpr bool kFused = true, kStoresRows = true;
  const float *rx, *rw, *bias, *so;
  int relu;
  int8_t *yq;
  int ldyq, dwords;
  float cw[4], cb[4];
  __device__ __forceinline__ void columns(int col, int n, bool whole) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool in = !EDGE || whole || col + u < n;
      cw[u] = in ? rw[col + u] : 0.0f;
      cb[u] = bias && in ? bias[col + u] : 0.0f;
    }
  }
  __device__ __forceinline__ void store(i32x4 v, int row, int col, int m, int n, bool whole) const {
#pragma clang fp contract(off)
    if (EDGE && !whole && row >= m) return;
    const float r = rx[row], s = so[row];
    int q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float y = (float)v[u] * r;
      y = y * cw[u];
      if (bias) y = y + cb[u];
      if (relu) y = !(y <= 0.0f) ? y : 0.0f;   // (NaN: not <= 0, stays -- and quantises to 0)
      q[u] = quantize_one(y, s);
    }
    int8_t *at = yq + (size_t)row * ldyq + col;
    if (!EDGE || (dwords && (whole || col + 3 < n))) {
      *reinterpret_cast<uint32_t *>(at) = (unsigned)(q[0] & 255) | ((unsigned)(q[1] & 255) << 8) | ((unsigned)(q[2] & 255) << 16) |
                                          ((unsigned)(q[3] & 255) << 24);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (whole || col + u < n) at[u] = (int8_t)q[u];
    }
  }
};

// m x n = rows x out, k = in; xq: the activations' int8 rows (pitch ldq), wq: the weight image (in x pitch_n), read in place as B
template <int BM, int BN, int TM, bool EDGE>
__global__ void __launch_bounds__(BM / (16 * TM) * (BN / 64) * 64, (BM == 128 && BN == 128) ? 2 : 1)
qlinear_s8o_kernel(int m, int n, int k, const int8_t *__restrict__ xq, int ldq, const int8_t *__restrict__ wq, int pitch_n,
                   const float *__restrict__ rx, const float *__restrict__ rw, const float *__restrict__ bias, int relu,
                   const float *__restrict__ so, int8_t *__restrict__ yq, int ldyq, int dwords, int nbm, int nbn) {
  QlinearS8oEpilogue<EDGE> ep{rx, rw, bias, so, relu, yq, ldyq, dwords};
  igemm_s8_dma_tile<BM, BN, TM, EDGE, 0, true>(m, n, k, xq, ldq, wq, pitch_n, n, nullptr, 0, 0, nbm, nbn, nullptr, ep);
}

// ---- the four instantiations, one per translation unit (build.py compiles them in parallel), each behind one function ----------
struct QlinearS8oArgs {
  int rows, out, in;
  const int8_t *xq;
  int ldq;
  const int8_t *wq;
  int pitch_n;
  const float *rx, *rw, *bias;   // bias NULL: no sum
  int relu;
  const float *so;
  int8_t *yq;
  int ldyq, dwords, nbm, nbn;
};

hipError_t launch_qlinear_s8o_128(const QlinearS8oArgs &a, hipStream_t s);
hipError_t launch_qlinear_s8o_128_edge(const QlinearS8oArgs &a, hipStream_t s);
hipError_t launch_qlinear_s8o_256(const QlinearS8oArgs &a, hipStream_t s);
hipError_t launch_qlinear_s8o_256_edge(const QlinearS8oArgs &a, hipStream_t s);

// the one of the four that the plan (qlinear_s8o_plan.hpp, Q8oPlan: tile, edge) names -- a template, so that the kernels' translation
// units, which include this header, do not depend on the plan's
template <class Plan>
hipError_t launch_qlinear_s8o(const Plan &p, const QlinearS8oArgs &a, hipStream_t s) {
  return p.tile == 256 ? (p.edge ? launch_qlinear_s8o_256_edge(a, s) : launch_qlinear_s8o_256(a, s))
                       : (p.edge ? launch_qlinear_s8o_128_edge(a, s) : launch_qlinear_s8o_128(a, s));
}

template <int TILE, bool EDGE>
hipError_t launch_qlinear_s8o_tile(const QlinearS8oArgs &a, hipStream_t s) {
  constexpr int TM = TILE / 32;
  constexpr unsigned threads = TILE / (16 * TM) * (TILE / 64) * 64;
  constexpr size_t lds = 4 * (size_t)TILE * IK;   // two stages of (A image | B image)
  auto kern = qlinear_s8o_kernel<TILE, TILE, TM, EDGE>;
  if (const hipError_t e = opt_in_big_lds(reinterpret_cast<const void *>(kern), lds); e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3((unsigned)(a.nbm * a.nbn)), dim3(threads), lds, s, a.rows, a.out, a.in, a.xq, a.ldq, a.wq, a.pitch_n,
                     a.rx, a.rw, a.bias, a.relu, a.so, a.yq, a.ldyq, a.dwords, a.nbm, a.nbn);
  return hipGetLastError();
}

}  // namespace mmh
