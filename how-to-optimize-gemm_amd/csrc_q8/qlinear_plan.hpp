// qlinear_plan.hpp -- what an mmh_q8_linear call will do, decided once: plan_qlinear turns (shape, leading dimensions, base
// residues, CU count, epilogue) into the row quantiser's form and path, the GEMM's instantiation and grid, the layout of the
// weight object's scratch and the text of mmh_q8_last_launch.  Host arithmetic only: mmh_q8_linear launches what the plan
// says, mmh_q8_linear_plan prints it, and tests/test_q8_abi.py holds it to a Python restatement.
#pragma once
#include <stddef.h>
#include <stdio.h>

#include "igemm_plan.hpp"   // i8_big_tile, i8_window

namespace mmh {

constexpr int kQrWaveCols = 1024;   // qlinear_s8.hpp's QR_WAVE_COLS

constexpr int q8_pitch(int n) { return (n + 15) & ~15; }
constexpr size_t q8_align16(size_t b) { return (b + 15) & ~(size_t)15; }

// The row quantiser's launch for rows x cols: a workgroup per row from kQrWaveCols columns on, else a wave per row, four to a workgroup
struct RowQuantPlan {
  bool wide, vec;
  unsigned grid;
};
inline RowQuantPlan plan_row_quant(int rows, int cols, bool vec) {
  const bool wide = cols >= kQrWaveCols;
  return {wide, vec, (unsigned)(wide ? rows : (rows + 3) / 4)};
}

struct Q8Plan {
  RowQuantPlan quant;
  int tile;          // BM = BN; TM = tile / 32
  bool edge;         // guarded tiles
  int nbm, nbn, grid;
  int pitch_k;       // of the activations' int8 image
  // the scratch: [int8 image rows x pitch_k | rows scales | rows reciprocals], each part 16-byte aligned
  size_t off_scale, off_inv, scratch;
  char text[256];    // mmh_q8_last_launch
};

// rows, out > 0, in >= 0, valid leading dimensions; x16 / y16: the bases of x and y modulo 16
inline Q8Plan plan_qlinear(int rows, int out, int in, int ldx, int ldy, int x16, int y16, int cus, bool bias, bool relu) {
  Q8Plan p{};
  p.pitch_k = q8_pitch(in);
  // (the image and the scale arrays are the object's own allocations: only x decides the quantiser's path)
  p.quant = plan_row_quant(rows, in, x16 == 0 && ldx % 4 == 0);
  p.tile = i8_big_tile(rows, out, cus) ? 256 : 128;
  p.edge = !(rows % p.tile == 0 && out % p.tile == 0 && ldy % 4 == 0 && y16 == 0);
  p.nbm = (rows + p.tile - 1) / p.tile, p.nbn = (out + p.tile - 1) / p.tile;
  p.grid = p.nbm * p.nbn;
  p.off_scale = q8_align16((size_t)rows * p.pitch_k);
  p.off_inv = p.off_scale + q8_align16((size_t)rows * sizeof(float));
  p.scratch = p.off_inv + q8_align16((size_t)rows * sizeof(float));
  snprintf(p.text, sizeof p.text, "quantize_rows_s8_kernel<%s> (%s path), %u workgroups, then qlinear_s8_kernel<%d,%d,%d,%s,%s,%s>, %d workgroups",
           p.quant.wide ? "true" : "false", p.quant.vec ? "vector" : "scalar", p.quant.grid, p.tile, p.tile, p.tile / 32,
           p.edge ? "true" : "false", bias ? "true" : "false", relu ? "true" : "false", p.grid);
  return p;
}

// The in-place tiles read the activations' image and the weight image through buffer descriptors: inside their 2 GiB window
inline bool q8_window(int out, int in) { return i8_window(q8_pitch(in), q8_pitch(out), in); }

}  // namespace mmh
