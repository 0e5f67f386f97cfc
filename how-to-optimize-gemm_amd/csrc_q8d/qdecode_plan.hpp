// qdecode_plan.hpp -- what an mmh_q8d_linear call will do, decided once: the column strips, the K ranges, the bytes of the caller's
// workspace, the finish kernel's form and the text of mmh_q8d_last_launch.  Host arithmetic only: mmh_q8d_linear launches what the
// plan says, mmh_q8d_linear_plan prints it, and tests/test_q8d_abi.py holds it to a Python restatement (tests/qdecode_ref.py).
//
// The rule.  strips = ceil(out / 128), slices = ceil(in / 128).  The plan wants kQdWgNum workgroups on every kQdWgDen compute
// units (three on two):
//   want   = ceil(kQdWgNum * cus / (kQdWgDen * strips))
// but the partials cost traffic the tile path does not have -- each is written once and read once, 2 * splits * rows * out * 4
// bytes -- and that stays at or below kQdTrafficNum / kQdTrafficDen (a quarter) of the weight's in * out bytes:
//   cap    = in * kQdTrafficNum / (8 * rows * kQdTrafficDen)
//   splits = max(1, min(want, cap, slices))
// The range is then k_len = 128 * ceil(slices / splits) and splits = ceil(slices / (k_len / 128)): every range starts inside
// `in`, none is empty, the last one may be short or hold only a k tail.  A forced split count keeps its count, takes the same
// k_len and is refused where (splits - 1) * k_len >= in.  in == 0: no partial kernel, splits = 0, no workspace.
// profiles/qdecode_sweep.md has the measurements behind the two constants (its "fit" table: at 16 rows 4 - 8 ranges of a 4096-deep
// layer are the fastest, 16 cost a quarter more -- the finish kernel reads every partial).
#pragma once
#include <stddef.h>
#include <stdio.h>

#include "igemm_plan.hpp"   // i8_dword, i8_window

namespace mmh {

constexpr int kQdStrip = 128, kQdSlice = 128, kQdMaxRows = 16;
constexpr int kQdWgNum = 3, kQdWgDen = 2;              // the occupancy target: three workgroups on two CUs (five 32 KiB rings fit one)
constexpr int kQdTrafficNum = 1, kQdTrafficDen = 4;    // partial traffic <= 1/4 of the weight's bytes
constexpr int kQdFinishCols = 1024;                    // columns of a finish workgroup: 256 threads x 4

struct QdPlan {
  bool ok;       // false: a forced split count that leaves a range empty
  int strips, splits, k_len, wp;
  bool out8, wide;
  int finish_x;  // finish workgroups per row
  size_t work_bytes;
  char text[192];   // mmh_q8d_last_launch
};

// rows in 1..16, out > 0, in >= 0; o16: the output's base modulo 16; forced: 0 or the caller's split count (> 0)
inline QdPlan plan_qdecode(int rows, int out, int in, bool out8, int ldo, int o16, int forced, int cus) {
  QdPlan p{};
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
      const long cap = (long)in * kQdTrafficNum / (8L * rows * kQdTrafficDen);
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
    snprintf(p.text, sizeof p.text, "qdecode_partial_kernel, %d strips x %d splits of %d k; qdecode_finish_kernel<%s>, %d workgroups, %s stores",
             p.strips, p.splits, p.k_len, o, p.finish_x * rows, w);
  else
    snprintf(p.text, sizeof p.text, "qdecode_finish_kernel<%s> alone, %d workgroups, %s stores", o, p.finish_x * rows, w);
  return p;
}

}  // namespace mmh
