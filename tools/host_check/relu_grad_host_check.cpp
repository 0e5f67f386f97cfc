// relu_grad_host_check.cpp -- csrc/relu_grad.hpp's kernels run as HOST functions, thread by thread, on exactly sized heap
// buffers, against a plain scalar loop: built with -fsanitize=address,undefined it shows on the CPU every access outside a
// window's last row, every misaligned vector access and every use of an index the grid does not cover, for shapes x layouts
// x modes (gate on / off, dz written / not / in place, column sum on / off / accumulated; 16-byte and scalar paths; the strided
// column loop; the finish kernel's batches), and -- the inputs' sums round, the scalar loop is the contract's order, and
// -ffp-contract=off keeps its adds adds -- every column sum's order.  No GPU, no HIP runtime: hip/hip_runtime.h next to this file stands in for the few constructs the header uses.
//
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//           -Itools/host_check tools/host_check/relu_grad_host_check.cpp -o /tmp/relu_grad_host_check && /tmp/relu_grad_host_check
// (tests/test_relu_grad_host_check.py does exactly that.)
#define MMH_RG_PER_LANE(offset, stride) ((void)0)   // the device build's register-class hint (an empty asm on vector registers)
#include "../../how-to-optimize-gemm_amd/csrc/relu_grad.hpp"
#include "../../include/mmult_hip.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>
thread_local dim3 blockIdx, threadIdx, gridDim, blockDim;
using namespace mmh;

template <int W, bool G, bool Z, bool S>
static void run_pass(dim3 grid, const ReluGradArgs &a) {
  gridDim = grid;
  for (unsigned by = 0; by < grid.y; ++by)
    for (unsigned bx = 0; bx < grid.x; ++bx)
      for (unsigned t = 0; t < RG_THREADS; ++t) {
        blockIdx.x = bx; blockIdx.y = by; threadIdx.x = t;
        relu_grad_colsum_kernel<W, G, Z, S>(a);
      }
}
template <int W>
static void pass(bool g, bool z, bool s, dim3 grid, const ReluGradArgs &a) {
  if (g) { if (z && s) run_pass<W, true, true, true>(grid, a); else if (z) run_pass<W, true, true, false>(grid, a); else run_pass<W, true, false, true>(grid, a); }
  else { if (z && s) run_pass<W, false, true, true>(grid, a); else if (z) run_pass<W, false, true, false>(grid, a); else run_pass<W, false, false, true>(grid, a); }
}
static unsigned bits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static bool same(float a, float b) { return (std::isnan(a) && std::isnan(b)) || bits(a) == bits(b); }

int main() {
  setvbuf(stdout, nullptr, _IONBF, 0);   // a mismatch returns with its buffers still allocated: the message must be out before the leak report ends the process
  const int R = MMH_COLSUM_BLOCK_ROWS;
  const int rowsv[] = {1, 7, 8, 9, R - 1, R, R + 1, 2 * R + 44}, colsv[] = {1, 3, 4, 5, 255, 256, 257, 1023, 1028};
  // the finish kernel's batches of RG_FU partial rows behind p_0: one full batch (the last block one row), a batch plus one
  // block, two batches, two batches plus one block -- at two column counts only (thread by thread, the full list would take minutes)
  const int manyv[] = {RG_FU * R + 1, (RG_FU + 1) * R + 77, 2 * RG_FU * R + 1, (2 * RG_FU + 1) * R + 77}, manycolsv[] = {5, 260};
  std::vector<std::pair<int, int>> shapes;
  for (int rows : rowsv) for (int cols : colsv) shapes.push_back({rows, cols});
  for (int rows : manyv) for (int cols : manycolsv) shapes.push_back({rows, cols});
  long checked = 0;
  for (auto [rows, cols] : shapes) for (int layout = 0; layout < 3; ++layout)
  for (int mode = 0; mode < 7; ++mode) {
    const bool gate = mode == 0 || mode == 2 || mode == 3 || mode == 4, dz = mode != 2 && mode != 5, sum = mode != 3 && mode != 6;
    const bool inplace = mode == 4 || mode == 6, acc = mode == 1 || mode == 4;
    const int ld = layout == 0 ? cols : layout == 1 ? (cols + 3) / 4 * 4 + 4 : (cols + 4) | 1;
    const bool vec = ld % 4 == 0;
    // exact-size buffers
    const size_t n = (size_t)(rows - 1) * ld + cols;
    // (16-byte aligned, the size rounded up to 16 bytes: at most 3 floats of slack behind the last row)
    float *g = (float *)aligned_alloc(16, (n * 4 + 15) / 16 * 16), *y = (float *)aligned_alloc(16, (n * 4 + 15) / 16 * 16);
    float *z = inplace ? g : (float *)aligned_alloc(16, (n * 4 + 15) / 16 * 16);
    std::vector<float> hg(n), hy(n);
    // (sevenths: the sums ROUND, so the order of the additions shows in the bits, not only the addressing)
    for (size_t i = 0; i < n; ++i) { hg[i] = (float)(rand() % 2001 - 1000) / 7.0f; hy[i] = (float)(rand() % 7 - 3); if (rand() % 17 == 0) hg[i] = -0.0f; }
    memcpy(g, hg.data(), n * 4); memcpy(y, hy.data(), n * 4);
    if (!inplace) for (size_t i = 0; i < n; ++i) z[i] = -777.25f;
    const int nblocks = (rows + R - 1) / R;
    const long long ldo = ((long long)cols + 3) & ~3ll;
    float *parts = (float *)malloc((size_t)nblocks * ldo * 4), *out = (float *)malloc((size_t)cols * 4);
    std::vector<float> old(cols);
    for (int j = 0; j < cols; ++j) out[j] = old[j] = (float)(rand() % 100) / 7.0f;
    ReluGradArgs a{g, gate ? y : nullptr, dz ? z : nullptr, nblocks > 1 ? parts : out, ld, ld, ld, nblocks > 1 ? ldo : 0, rows, cols, R, nblocks > 1 ? 0 : (acc ? 2 : 1)};
    const int W = vec ? 4 : 1;
    const long long items = cols / W + cols % W, chunks = (items + RG_THREADS - 1) / RG_THREADS;
    dim3 grid; grid.x = nblocks; grid.y = (unsigned)chunks;
    if (layout == 2 && cols > 300) grid.y = 1;   // the strided column loop
    if (vec) pass<4>(gate, dz, sum, grid, a); else pass<1>(gate, dz, sum, grid, a);
    if (sum && nblocks > 1) {
      gridDim.x = (cols + RG_FIN_THREADS - 1) / RG_FIN_THREADS; gridDim.y = 1;
      for (unsigned bx = 0; bx < gridDim.x; ++bx) for (unsigned t = 0; t < RG_FIN_THREADS; ++t) { blockIdx.x = bx; blockIdx.y = 0; threadIdx.x = t; colsum_finish_kernel(parts, nblocks, ldo, cols, out, acc ? 1 : 0); }
    }
    // reference
    for (int j = 0; j < cols; ++j) {
      volatile float s = 0;
      for (int b = 0; b < nblocks; ++b) {
        volatile float p = 0;
        for (int r = b * R; r < rows && r < b * R + R; ++r) {
          const float gv = hg[(size_t)r * ld + j], yv = hy[(size_t)r * ld + j];
          const float zv = gate ? (yv <= 0.0f ? 0.0f : gv) : gv;
          if (dz && !same(z[(size_t)r * ld + j], zv)) { printf("dz mismatch rows %d cols %d layout %d mode %d at (%d,%d)\n", rows, cols, layout, mode, r, j); return 1; }
          if (r == b * R) p = zv; else p = p + zv;
        }
        if (b == 0) s = p; else s = s + p;
      }
      const float want = acc ? old[j] + s : s;
      if (sum && !same(out[j], want)) { printf("colsum mismatch rows %d cols %d layout %d mode %d col %d: %g vs %g\n", rows, cols, layout, mode, j, out[j], want); return 1; }
      if (!sum && !same(out[j], old[j])) { printf("colsum touched\n"); return 1; }
    }
    // gaps between rows are never written
    if (dz && !inplace)
      for (int r = 0; r + 1 < rows; ++r) for (int j = cols; j < ld; ++j) if (z[(size_t)r * ld + j] != -777.25f) { printf("gap written rows %d cols %d layout %d mode %d\n", rows, cols, layout, mode); return 1; }
    ++checked;
    free(g); free(y); if (!inplace) free(z); free(parts); free(out);
  }
  printf("emulated %ld cases: all equal\n", checked);
  return 0;
}
