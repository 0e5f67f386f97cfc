// qlinear_s8o_plan.hpp -- what an mmh_q8o_linear call will do, decided once: the tile (csrc/igemm_plan.hpp, i8_big_tile, as
// plan_qlinear chooses it), whether its tiles are guarded, whether the epilogue may store dwords, the grid and the text of
// mmh_q8o_last_launch.  Host arithmetic only: mmh_q8o_linear launches what the plan says, mmh_q8o_linear_plan prints it, and
// tests/test_q8o_abi.py holds it to a Python restatement (tests/qchain_ref.py, plan_text_s8o).
#pragma once
#include <stdio.h>

#include "igemm_plan.hpp"   // i8_big_tile, i8_dword, i8_window

namespace mmh {

struct Q8oPlan {
  int tile;      // BM = BN; TM = tile / 32
  bool dwords;   // yq's base and pitch are multiples of 4: a lane's four bytes leave as one dword
  bool edge;     // guarded tiles: a ragged shape, or a yq that only takes bytes
  int nbm, nbn, grid;
  char text[128];   // mmh_q8o_last_launch
};

// rows, out > 0, ldyq >= out; yq4: yq's base modulo 4.  The fp32 family's guard rule with 4 bytes where it has 16.
inline Q8oPlan plan_qlinear_s8o(int rows, int out, int ldyq, int yq4, int cus) {
  Q8oPlan p{};
  p.tile = i8_big_tile(rows, out, cus) ? 256 : 128;
  p.dwords = i8_dword(ldyq, yq4);
  p.edge = !(rows % p.tile == 0 && out % p.tile == 0 && p.dwords);
  p.nbm = (rows + p.tile - 1) / p.tile, p.nbn = (out + p.tile - 1) / p.tile;
  p.grid = p.nbm * p.nbn;
  snprintf(p.text, sizeof p.text, "qlinear_s8o_kernel<%d,%d,%d,%s>, %d workgroups", p.tile, p.tile, p.tile / 32, p.edge ? "true" : "false",
           p.grid);
  return p;
}

}  // namespace mmh
