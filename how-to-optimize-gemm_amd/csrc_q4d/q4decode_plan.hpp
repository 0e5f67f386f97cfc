// q4decode_plan.hpp -- what an mmh_q4d_linear call will do, decided once: csrc_q8d/qdecode_plan.hpp's rule (its constants, its
// geometry, its workspace and finish-kernel forms) with two changes.  Host arithmetic only: mmh_q4d_linear launches what the plan
// says, mmh_q4d_linear_plan prints it, and tests/test_q4d_abi.py holds it to a Python restatement (tests/q4_ref.py).
//
//   1. The weight is in * out / 2 bytes, so the partials' traffic (2 * splits * rows * out * 4 bytes) stays at or below a
//      quarter of THAT:  cap = in * kQdTrafficNum / (16 * rows * kQdTrafficDen).
//   2. No K range is longer than kQ4MaxRangeK = 65536 k (include/mmult_hip_q4d.h derives the bound: the accumulator holds 16 x
//      the sum):  splits >= ceil(slices / 512), whatever want and cap say.  A forced split count keeps its count and is
//      refused where its k_len exceeds the ceiling (`long_range`) or (splits - 1) * k_len >= in (an empty range).
// The 2 GiB window of the packed image: q4_window.
#pragma once
#include <stddef.h>
#include <stdio.h>

#include "qdecode_plan.hpp"   // QdPlan, the constants; igemm_plan.hpp's i8_dword, kI8Window

namespace mmh {

constexpr int kQ4MaxRangeK = 65536;
constexpr int kQ4SliceRows = kQdSlice / 2;   // packed rows of a 128-k slice

struct Q4Plan : QdPlan {
  bool long_range;   // !ok because a forced range would exceed kQ4MaxRangeK
};

constexpr int q4_packed_rows(int in) { return kQ4SliceRows * ((in + kQdSlice - 1) / kQdSlice); }
// the x rows as i8_window holds them; the packed image and the slices the ring requests behind its end
constexpr bool q4_window(int ldq, int pitch_n, int in) {
  return (size_t)256 * ldq + in < kI8Window && (size_t)(q4_packed_rows(in) + 128) * pitch_n + 256 < kI8Window;
}

// rows in 1..16, out > 0, in >= 0; o16: the output's base modulo 16; forced: 0 or the caller's split count (> 0)
inline Q4Plan plan_q4decode(int rows, int out, int in, bool out8, int ldo, int o16, int forced, int cus) {
  Q4Plan p{};
  p.ok = true;
  p.out8 = out8;
  p.strips = (out + kQdStrip - 1) / kQdStrip;
  p.wp = (out + 3) & ~3;
  p.wide = out8 ? i8_dword(ldo, o16 % 4) : (ldo % 4 == 0 && o16 == 0);
  p.finish_x = (out + kQdFinishCols - 1) / kQdFinishCols;
  const int slices = (in + kQdSlice - 1) / kQdSlice;
  if (in > 0) {
    if (forced > 0) {
      p.splits = forced;
      if (forced > slices) p.ok = false;
    } else {
      const long want = ((long)kQdWgNum * cus + (long)kQdWgDen * p.strips - 1) / ((long)kQdWgDen * p.strips);
      const long cap = (long)in * kQdTrafficNum / (16L * rows * kQdTrafficDen);
      const long least = (slices + kQ4MaxRangeK / kQdSlice - 1) / (kQ4MaxRangeK / kQdSlice);
      long s = want < cap ? want : cap;
      if (s > slices) s = slices;
      if (s < least) s = least;
      p.splits = s < 1 ? 1 : (int)s;
    }
    if (p.ok) {
      const int per = (slices + p.splits - 1) / p.splits;
      p.k_len = per * kQdSlice;
      if (forced > 0) {
        p.ok = (long)(forced - 1) * p.k_len < in;
        if (p.ok && p.k_len > kQ4MaxRangeK) p.ok = false, p.long_range = true;
      } else {
        p.splits = (slices + per - 1) / per;
      }
    }
  }
  if (!p.ok) return p;
  p.work_bytes = ((size_t)p.splits * rows * p.wp * 4 + 15) & ~(size_t)15;
  const char *o = out8 ? "true" : "false", *w = p.wide ? "wide" : "single";
  if (in > 0)
    snprintf(p.text, sizeof p.text, "q4decode_partial_kernel, %d strips x %d splits of %d k; qdecode_finish_kernel<%s>, %d workgroups, %s stores",
             p.strips, p.splits, p.k_len, o, p.finish_x * rows, w);
  else
    snprintf(p.text, sizeof p.text, "qdecode_finish_kernel<%s> alone, %d workgroups, %s stores", o, p.finish_x * rows, w);
  return p;
}

}  // namespace mmh
