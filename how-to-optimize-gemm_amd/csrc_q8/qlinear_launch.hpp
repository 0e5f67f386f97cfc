// qlinear_launch.hpp -- the GEMM's sixteen instantiations, four per translation unit (tile x guarded: qlinear_128.hip,
// qlinear_128_edge.hip, qlinear_256.hip, qlinear_256_edge.hip -- build.py compiles them in parallel), each behind one function.
#pragma once
#include <type_traits>

#include "qlinear_s8.hpp"

namespace mmh {

struct QlinearArgs {
  int rows, out, in;
  const int8_t *xq;
  int pitch_k;
  const int8_t *wq;
  int pitch_n;
  const float *rx, *rw, *bias;   // bias NULL: the instantiations without the sum
  int relu;
  float *y;
  int ldy, nbm, nbn;
};

hipError_t launch_qlinear_128(const QlinearArgs &a, hipStream_t s);
hipError_t launch_qlinear_128_edge(const QlinearArgs &a, hipStream_t s);
hipError_t launch_qlinear_256(const QlinearArgs &a, hipStream_t s);
hipError_t launch_qlinear_256_edge(const QlinearArgs &a, hipStream_t s);

// the one of the four that the plan (qlinear_plan.hpp, Q8Plan: tile, edge) names -- a template, so that the kernels' translation
// units, which include this header, do not depend on the plan's
template <class Plan>
hipError_t launch_qlinear(const Plan &p, const QlinearArgs &a, hipStream_t s) {
  return p.tile == 256 ? (p.edge ? launch_qlinear_256_edge(a, s) : launch_qlinear_256(a, s))
                       : (p.edge ? launch_qlinear_128_edge(a, s) : launch_qlinear_128(a, s));
}

template <int TILE, bool EDGE>
hipError_t launch_qlinear_tile(const QlinearArgs &a, hipStream_t s) {
  constexpr int TM = TILE / 32;
  constexpr unsigned threads = TILE / (16 * TM) * (TILE / 64) * 64;
  constexpr size_t lds = 4 * (size_t)TILE * IK;   // two stages of (A image | B image)
  auto go = [&](auto kern) -> hipError_t {
    if (const hipError_t e = opt_in_big_lds(reinterpret_cast<const void *>(kern), lds); e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)(a.nbm * a.nbn)), dim3(threads), lds, s, a.rows, a.out, a.in, a.xq, a.pitch_k, a.wq,
                       a.pitch_n, a.rx, a.rw, a.bias, a.y, a.ldy, a.nbm, a.nbn);
    return hipGetLastError();
  };
  if (a.bias) return a.relu ? go(qlinear_s8_kernel<TILE, TILE, TM, EDGE, true, true>) : go(qlinear_s8_kernel<TILE, TILE, TM, EDGE, true, false>);
  return a.relu ? go(qlinear_s8_kernel<TILE, TILE, TM, EDGE, false, true>) : go(qlinear_s8_kernel<TILE, TILE, TM, EDGE, false, false>);
}

}  // namespace mmh
