// q4gdecode_plan.hpp -- what an mmh_q4g_linear call will do, decided once: csrc_q8d/qdecode_plan.hpp's rule (its constants, its
// geometry, its workspace and finish-kernel forms) with ONE change, csrc_q4d/q4decode_plan.hpp's first: the weight is
// in * out / 2 bytes, so the partials' traffic (2 * splits * rows * out * 4 bytes) stays at or below a quarter of THAT:
//   cap = in * kQdTrafficNum / (16 * rows * kQdTrafficDen).
// That plan's second change, the 65536-k ceiling of a range, has no counterpart: the kernel's int32 accumulator restarts every
// slice (include/mmult_hip_q4g.h derives it).  The partials are fp32 here, 4 bytes as there: the same work_bytes.
// The partition (splits, k_len) is part of the NUMERIC contract -- the fp32 partial sums are added in its order -- so this file
// is too.  Host arithmetic only: mmh_q4g_linear launches what the plan says, mmh_q4g_linear_plan prints it, and
// tests/test_q4g_abi.py holds it to a Python restatement (tests/q4g_ref.py).
#pragma once
#include <stddef.h>
#include <stdio.h>

#include "q4decode_plan.hpp"   // q4_packed_rows, q4_window; qdecode_plan.hpp's QdPlan and constants; igemm_plan.hpp's i8_dword, kI8Window

namespace mmh {

constexpr int kQ4gGroup = kQdSlice;   // input features per scale: one slice

constexpr int q4g_groups(int in) { return (in + kQ4gGroup - 1) / kQ4gGroup; }
// x and the packed image as q4_window holds them; the scale rows and the (up to three) rows the ring requests behind a range's end
constexpr bool q4g_window(int ldq, int pitch_n, int in, int pitch_s) {
  return q4_window(ldq, pitch_n, in) && ((size_t)q4g_groups(in) + 4) * pitch_s * 4 + 1024 < kI8Window;
}

// rows in 1..16, out > 0, in >= 0; o16: the output's base modulo 16; forced: 0 or the caller's split count (> 0)
inline QdPlan plan_q4gdecode(int rows, int out, int in, bool out8, int ldo, int o16, int forced, int cus) {
  QdPlan p{};
  p.ok = true;
  p.out8 = out8;
  p.strips = (out + kQdStrip - 1) / kQdStrip;
  p.wp = (out + 3) & ~3;
  p.wide = out8 ? i8_dword(ldo, o16 % 4) : (ldo % 4 == 0 && o16 == 0);
  p.finish_x = (out + kQdFinishCols - 1) / kQdFinishCols;
  const int slices = q4g_groups(in);
  if (in > 0) {
    if (forced > 0) {
      p.splits = forced;
      if (forced > slices) p.ok = false;
    } else {
      const long want = ((long)kQdWgNum * cus + (long)kQdWgDen * p.strips - 1) / ((long)kQdWgDen * p.strips);
      const long cap = (long)in * kQdTrafficNum / (16L * rows * kQdTrafficDen);
      long s = want < cap ? want : cap;
      if (s > slices) s = slices;
      p.splits = s < 1 ? 1 : (int)s;
    }
    if (p.ok) {
      const int per = (slices + p.splits - 1) / p.splits;
      p.k_len = per * kQdSlice;
      if (forced > 0) p.ok = (long)(forced - 1) * p.k_len < in;
      else p.splits = (slices + per - 1) / per;
    }
  }
  if (!p.ok) return p;
  p.work_bytes = ((size_t)p.splits * rows * p.wp * 4 + 15) & ~(size_t)15;
  const char *o = out8 ? "true" : "false", *w = p.wide ? "wide" : "single";
  if (in > 0)
    snprintf(p.text, sizeof p.text, "q4gdecode_partial_kernel, %d strips x %d splits of %d k; q4gdecode_finish_kernel<%s>, %d workgroups, %s stores",
             p.strips, p.splits, p.k_len, o, p.finish_x * rows, w);
  else
    snprintf(p.text, sizeof p.text, "q4gdecode_finish_kernel<%s> alone, %d workgroups, %s stores", o, p.finish_x * rows, w);
  return p;
}

}  // namespace mmh
