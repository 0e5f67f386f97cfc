// igemm_plan.hpp -- what an int8 call will do, decided once: the table of MMH_OPT_IGEMM_MODE values (kI8Modes) and the pure
// function plan_igemm_s8 that turns (entry point, mode, shape, leading dimensions, base residues, CU count, grid cap) into an
// I8Plan -- the kernel instantiation, its grid, which operands are first copied to dense images, fused or two-pass, the bytes of
// every scratch buffer and the text of mmh_last_launch.  Host arithmetic only: no HIP call, no pointer.  mmh_set_option reads
// the table, mmh_igemm_s8 / mmh_qgemm_f32 (igemm.hip) reserve and launch what the plan says, mmh_igemm_plan prints it, and the
// CPU tests hold it to their own restatement (tests/int8_ops.py).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "ab_build.hpp"

namespace mmh {

// The kernel families (igemm_s8.hpp, igemm_s8_pp.hpp; K3 and K3d: tools/ab/igemm_s8_k3.hpp)
enum class I8Family { Auto, Simple, K3t, K3p, K3, K3d };
enum class I8Form { Auto, Persistent, PerTile };   // K3p's launch form
constexpr int kI8Igemm = 0, kI8Qgemm = 1;          // the entry points (MMH_I8_IGEMM, MMH_I8_QGEMM)

// One row per MMH_OPT_IGEMM_MODE value: its name, whether the product has it (or only the tools build), and what it forces on
// operands that family can take (others: the simple kernel; in mode 0, dense copies first).  `ablate`: K3d's timing-only
// ablations, WRONG results (igemm_s8.hpp, ABLATE).
struct I8Mode {
  int value;
  const char *name;
  bool product;
  I8Family family;
  int tile;        // 128 / 256; 0: by the rounds of tiles (mode 0) or the family's only one
  int mfma_k;      // K3p: 64, or 32 for the instruction BASELINE.json configs[4] names
  I8Form form;
  bool packed_b;   // needs B packed into bt first
  int ablate;
};
constexpr I8Mode kI8Modes[] = {
    {0, "auto", true, I8Family::Auto, 0, 64, I8Form::Auto, false, 0},
    {1, "k3", false, I8Family::K3, 128, 64, I8Form::Auto, false, 0},
    {2, "simple", true, I8Family::Simple, 128, 64, I8Form::Auto, false, 0},
    {3, "k3d_128", false, I8Family::K3d, 128, 64, I8Form::Auto, true, 0},
    {4, "k3d_256", false, I8Family::K3d, 256, 64, I8Form::Auto, true, 0},
    {5, "k3t_128", true, I8Family::K3t, 128, 64, I8Form::Auto, false, 0},
    {6, "k3t_256", true, I8Family::K3t, 256, 64, I8Form::Auto, false, 0},
    {7, "k3p_mfma32", true, I8Family::K3p, 256, 32, I8Form::Auto, false, 0},
    {8, "k3p_persistent", true, I8Family::K3p, 256, 64, I8Form::Persistent, false, 0},
    {9, "k3p_per_tile", true, I8Family::K3p, 256, 64, I8Form::PerTile, false, 0},
    {10, "k3d_no_dma", false, I8Family::K3d, 256, 64, I8Form::Auto, true, 1},
    {11, "k3d_no_reads", false, I8Family::K3d, 256, 64, I8Form::Auto, true, 2},
    {12, "k3d_no_dma_no_reads", false, I8Family::K3d, 256, 64, I8Form::Auto, true, 3},
    {13, "k3d_no_store", false, I8Family::K3d, 256, 64, I8Form::Auto, true, 4},
};
// the row of a mode this build accepts, else nullptr
constexpr const I8Mode *i8_mode_row(int mode) {
  for (const I8Mode &r : kI8Modes)
    if (r.value == mode && (r.product || kAbBuild)) return &r;
  return nullptr;
}

// qs: [0, 2 AMAX_WORDS) abs-max words of a quantised GEMM's A and B, then its two scales, then the abs-max words of
// stand-alone mmh_quantize_sym_s8 calls, then 2 AMAX_WORDS words that are zero for as long as the buffer lives
constexpr int kI8AmaxWords = 64;   // quant_s8.hpp's AMAX_WORDS
constexpr size_t kQsWords = 4 * kI8AmaxWords + 16;
constexpr size_t kAmaxBytes = 2 * kI8AmaxWords * sizeof(unsigned);
constexpr size_t kQsBytes = kQsWords * sizeof(unsigned) + kAmaxBytes;
constexpr int kI8Xcds = 8;         // sgemm_tile.hpp's NXCD
constexpr int kI8SimpleK = 64;     // igemm_s8.hpp's IBK: the simple kernel's k bytes per slice

struct I8Plan {
  // the GEMM's instantiation ...
  I8Family family;
  int tile;        // BM = BN; TM = tile / 32
  bool edge, deq;  // guarded tiles; the dequantising epilogue
  int mfma_k, ablate;
  // ... its arguments: the shape, the leading dimensions it reads A, B (in place or their images) and writes C with ...
  int m, n, k, lda, ldb, ldc;
  // ... and its grid: `grid` workgroups over nbm x nbn tiles (fewer than tiles: persistent)
  int nbm, nbn, grid;
  bool copy_a, copy_b;   // mmh_igemm_s8: the operand is first copied to a dense image in qa / qb, with pitch_a / pitch_b
  int pitch_a, pitch_b;
  bool images;           // ... and the GEMM reads the images (else they too lie beyond the window: it reads the operands)
  bool fused;            // mmh_qgemm_f32: dequantised in the GEMM's epilogue; else int32 into qc, then dequantize_kernel
  bool vec_a, vec_b;     // mmh_qgemm_f32: the quantiser reads A / B on its vector path
  size_t qa, qb, qc, qs, bt;   // bytes the call needs of each scratch buffer
  char text[256];        // mmh_last_launch
};

// The arithmetic of plan_igemm_s8, one rule each.
// K3t / K3p read both operands in place through buffer descriptors: dword-aligned, byte offsets inside their 2 GiB window
constexpr bool i8_dword(int ld, int base16) { return ld % 4 == 0 && base16 % 4 == 0; }
constexpr size_t kI8Window = (1ull << 31) - 4096;
constexpr bool i8_window(int lda, int ldb, int k) {
  return (size_t)256 * lda + k < kI8Window && (size_t)(k + 256) * ldb + 256 < kI8Window;
}
// Tile choice of the in-place kernels: 256x256 tiles (K3p) run one per CU, 128x128 tiles (K3t) two per CU, and a full
// round of 128x128 tiles takes 0.58 of a 256x256 round's time for half its work (4096^3: 68.5 us in two rounds against
// 58.7 in one).  Rounds 3 - 5 never chose the big tile below one tile per CU; with the C stores coalesced (round 6) a
// part-filled chip of big tiles beats two rounds of small ones: 3072^3 31.8 against 43.1 us, 3584^3 42.9 / 53.0, 6144^3
// 205 / 217 -- and a single round of small tiles wins where there is one: 2048^3 14.1 / 22.5, 1024^3 9.8 / 13.1
// (profiles/r06_i8_persist_ab.txt).
inline bool i8_big_tile(int m, int n, int cus) {
  const long tiles256 = (long)((m + 255) / 256) * ((n + 255) / 256);
  const long tiles128 = (long)((m + 127) / 128) * ((n + 127) / 128);
  const long r256 = (tiles256 + cus - 1) / cus, r128 = (tiles128 + 2L * cus - 1) / (2L * cus);
  return (double)r256 <= 0.6 * (double)r128 + 1e-9;
}
// K3p's launch form.  Persistent (one workgroup per CU walking the tiles) saves a tile's launch and prologue: +1.3 / +4.5 /
// +1.7 % at 8192 x 8192 x 1024 / x 2048 and 5120^3; one workgroup per tile lets the dispatcher hand the next tile to whichever
// CU is free first -- tiles of a long K finish up to 20 us apart (tools/i8_timeline.py) -- and is 1.5 % ahead at 8192^3;
// level in between (profiles/r06_i8_persist_ab.txt).  `grid_cap` > 0 (the handle's MMH_I8_GRID_CAP test hook) overrides the
// count: a few persistent workgroups walk a small shape's tiles.  0: one workgroup per tile.
constexpr int i8_pp_cap(I8Form form, int k, int cus, int grid_cap) {
  if (form == I8Form::PerTile) return 0;
  if (grid_cap > 0) return grid_cap;
  if (form == I8Form::Persistent) return cus;
  return k <= 5120 ? cus : 0;
}
// tools build: bytes of B packed (transposed, zero padded) for K3d
constexpr size_t i8_pack_k(int k) { return ((size_t)k + 255) & ~(size_t)255; }
constexpr size_t i8_pack_bytes(int n, int k) { return (((size_t)n + 127) & ~(size_t)127) * i8_pack_k(k); }

// `mode` must be one this build accepts (i8_mode_row), m, n, k > 0 and the leading dimensions valid (check_gemm_args);
// a16 / b16 / c16: the operands' base addresses modulo 16 (mmh_qgemm_f32: of its float operands).
inline I8Plan plan_igemm_s8(int entry, int mode, int m, int n, int k, int lda, int ldb, int ldc, int a16, int b16, int c16,
                            int cus, int grid_cap) {
  const I8Mode &row = *i8_mode_row(mode);
  const bool automatic = row.family == I8Family::Auto;   // mode 0: everything is the plan's to choose
  I8Plan p{};
  p.m = m, p.n = n, p.k = k, p.lda = lda, p.ldb = ldb, p.ldc = ldc;
  char pre[96] = "";
  const char *post = "";
  if (entry == kI8Qgemm) {
    // dense, 16-byte-friendly workspace images: int8 A (m x lda), int8 B (k x ldb); hipMalloc'ed, so their alignment never decides.
    // vec_a / vec_b are quant_s8.hpp's quant_vec_ok of the float operands: its test of the int8 side (a dword base, a dword
    // pitch) always holds for these images, so the abs-max and the quantise pass take the same path
    p.vec_a = a16 == 0 && lda % 4 == 0, p.vec_b = b16 == 0 && ldb % 4 == 0;
    snprintf(pre, sizeof pre, "qgemm: absmax_kernel + quantize_kernel (A on the %s path, B on the %s path), then ",
             p.vec_a ? "vector" : "row", p.vec_b ? "vector" : "row");
    p.lda = (k + 15) & ~15, p.ldb = (n + 3) & ~3, a16 = b16 = 0;
    p.qa = (size_t)m * p.lda, p.qb = (size_t)k * p.ldb, p.qs = kQsBytes;
    // the fused form dequantises in the int8 GEMM's epilogue; the two-pass form (forced modes, images beyond the
    // descriptors' window) writes the int32 image m x ldb into qc first
    p.fused = p.deq = automatic && i8_window(p.lda, p.ldb, k);
    if (!p.fused) p.ldc = p.ldb, c16 = 0, p.qc = (size_t)m * p.ldb * sizeof(int32_t);
    post = p.fused ? ", dequantised in the epilogue" : " into int32 workspace, then dequantize_kernel (two-pass)";
  }
  bool in_place = i8_dword(p.lda, a16) && i8_dword(p.ldb, b16) && i8_window(p.lda, p.ldb, k);
  if (entry == kI8Igemm && automatic && !in_place) {
    // Default mode: operands the in-place kernels cannot take as they are (an odd leading dimension, a base that is not
    // dword-aligned) are first copied into dense dword-aligned workspace images -- one pass over m*k / k*n bytes, against
    // m*n*k MACs -- instead of falling back to the slow kernel.  (Where the images then lie beyond the descriptors' window
    // the copies are still made, as they always were, and the correctness-first kernel reads the operands themselves.)
    p.copy_a = !i8_dword(lda, a16), p.copy_b = !i8_dword(ldb, b16);
    p.pitch_a = p.copy_a ? (k + 15) & ~15 : lda, p.pitch_b = p.copy_b ? (n + 15) & ~15 : ldb;
    if (p.copy_a) p.qa = (size_t)m * p.pitch_a;
    if (p.copy_b) p.qb = (size_t)k * p.pitch_b;
    if ((p.images = in_place = i8_window(p.pitch_a, p.pitch_b, k))) {
      p.lda = p.pitch_a, p.ldb = p.pitch_b;
      if (p.copy_a) a16 = 0;
      if (p.copy_b) b16 = 0;
      post = p.copy_a && p.copy_b ? ", A copied to workspace, B copied to workspace"
                                  : p.copy_a ? ", A copied to workspace" : ", B copied to workspace";
    }
  }
  // The family and the tile: what the mode forces where the operands allow it, else the correctness-first kernel.  Left to
  // the plan (mode 0): the big tile by the rounds of tiles -- on K3p, which takes operands as the caller passed them
  // (mmh_igemm_s8 in place, the fused mmh_qgemm_f32) -- else K3t's small one.
  const bool big = row.tile ? row.tile == 256 : i8_big_tile(m, n, cus);
  p.family = row.family;
  if (automatic) p.family = big && !p.images ? I8Family::K3p : I8Family::K3t;
  if (p.family == I8Family::K3p && entry == kI8Qgemm && !p.fused) p.family = I8Family::Simple;
  if ((p.family == I8Family::K3t || p.family == I8Family::K3p) && !in_place) p.family = I8Family::Simple;
  if (p.family == I8Family::K3 &&
      !(i8_dword(p.lda, a16) && i8_dword(p.ldb, b16) && (size_t)128 * p.lda + k < kI8Window && (size_t)k * p.ldb + 128 < kI8Window))
    p.family = I8Family::Simple;
  if (p.family == I8Family::K3d && !(i8_dword(p.lda, a16) && (size_t)256 * p.lda + k < kI8Window && 256 * i8_pack_k(k) < kI8Window))
    p.family = I8Family::Simple;
  p.tile = p.family == I8Family::Simple || !big ? 128 : 256;
  p.mfma_k = p.family == I8Family::K3p ? row.mfma_k : 64;
  p.ablate = p.family == I8Family::K3d ? row.ablate : 0;
  if (row.packed_b) p.bt = i8_pack_bytes(n, k);   // (reserved whether or not the operands then allow K3d)
  // whole tiles and 16-byte C rows take the unguarded instantiation; the simple kernel's also reads whole 16-byte pieces of A
  // rows and dwords of B rows, unguarded
  const bool whole = m % p.tile == 0 && n % p.tile == 0 && p.ldc % 4 == 0 && c16 == 0;
  p.edge = !(whole && (p.family != I8Family::Simple ||
                       (k % kI8SimpleK == 0 && p.lda % 16 == 0 && a16 == 0 && i8_dword(p.ldb, b16))));
  p.nbm = (m + p.tile - 1) / p.tile, p.nbn = (n + p.tile - 1) / p.tile;
  const int tiles = p.nbm * p.nbn;
  p.grid = tiles;
  if (p.family == I8Family::K3p) {
    // the XCD map of block_to_tile reads the XCD off the (virtual) block index: a persistent grid is a multiple of the XCDs
    const int cap = i8_pp_cap(row.form, k, cus, grid_cap);
    if (cap > 0 && tiles > cap) p.grid = cap >= kI8Xcds ? cap / kI8Xcds * kI8Xcds : cap;
  }
  // mmh_last_launch: the instantiation, spelled as tools/kernel_resources.py demangles it, and its launch form -- written
  // straight into the plan: one snprintf for a call that neither quantises nor copies
  const char *e = p.edge ? "true" : "false", *d = p.deq ? "true" : "false";
  char *at = p.text, *const end = p.text + sizeof p.text;
  if (pre[0]) at += snprintf(at, end - at, "%s", pre);
  if (p.family == I8Family::Simple) at += snprintf(at, end - at, "igemm_s8_simple_kernel<%s>, %d workgroups", e, tiles);
  else if (p.family == I8Family::K3t)
    at += snprintf(at, end - at, "igemm_s8_dma_kernel<%d,%d,%d,%s,0,true>, B in place, %d workgroups", p.tile, p.tile, p.tile / 32, e, tiles);
  else if (p.family == I8Family::K3p && p.grid < tiles)
    at += snprintf(at, end - at, "igemm_s8_pp_kernel<%s,%s,%d>, persistent: %d workgroups walk %d tiles", e, d, p.mfma_k, p.grid, tiles);
  else if (p.family == I8Family::K3p)
    at += snprintf(at, end - at, "igemm_s8_pp_kernel<%s,%s,%d>, %d workgroups, one per tile", e, d, p.mfma_k, p.grid);
  // (the tools build's K3 / K3d leave no marker of their own)
  if (post[0]) snprintf(at, end - at, "%s", post);
  return p;
}

}  // namespace mmh

