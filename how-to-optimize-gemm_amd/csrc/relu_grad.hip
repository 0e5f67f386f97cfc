// relu_grad.hip -- mmh_relu_grad_colsum: the linear layer's backward beside its two GEMMs -- the ReLU gate on the incoming
// gradient and the bias gradient (column sums), one pass over rows x cols floats (relu_grad.hpp) and, from two row blocks up,
// the finish kernel that sums the blocks' partial rows in block order.  Part of libmmult_hip.so (see internal.hpp).
#include "internal.hpp"
#include "relu_grad.hpp"

namespace mmh {

static bool rows16(const void *p, int ld) { return aligned16(p) && ld % 4 == 0; }

static int relu_grad_check_args(int rows, int cols, const float *dG, int ldg, const float *dY, int ldy, const float *dZ, int ldz,
                                const float *dColsum) {
  if (rows < 0 || cols < 0 || !dG || (!dZ && !dColsum)) return MMH_ERR_INVALID_ARG;
  if (ldg < cols || (dY && ldy < cols) || (dZ && ldz < cols)) return MMH_ERR_INVALID_ARG;
  return MMH_OK;
}

template <int W>
static void launch_pass(bool gate, bool dz, bool sum, dim3 grid, hipStream_t s, const ReluGradArgs &a) {
#define MMH_RG_LAUNCH(G, Z, S) hipLaunchKernelGGL((relu_grad_colsum_kernel<W, G, Z, S>), grid, dim3(RG_THREADS), 0, s, a)
  if (gate) {
    if (dz && sum) MMH_RG_LAUNCH(true, true, true);
    else if (dz) MMH_RG_LAUNCH(true, true, false);
    else MMH_RG_LAUNCH(true, false, true);
  } else {
    if (dz && sum) MMH_RG_LAUNCH(false, true, true);
    else if (dz) MMH_RG_LAUNCH(false, true, false);
    else MMH_RG_LAUNCH(false, false, true);
  }
#undef MMH_RG_LAUNCH
}

int relu_grad_colsum_on(mmh_context *h, int rows, int cols, const float *dG, int ldg, const float *dY, int ldy, float *dZ, int ldz,
                        float *dColsum, int accumulate, hipStream_t s) {
  if (int rc = relu_grad_check_args(rows, cols, dG, ldg, dY, ldy, dZ, ldz, dColsum); rc != MMH_OK) return rc;
  if (cols == 0) return MMH_OK;
  if (rows == 0) {
    if (dColsum && !accumulate) HIP_TRY(hipMemsetAsync(dColsum, 0, (size_t)cols * sizeof(float), s));   // the empty sum: +0
    set_last_launch("relu_grad_colsum: no rows");
    return MMH_OK;
  }
  constexpr int R = MMH_COLSUM_BLOCK_ROWS;
  const bool gate = dY != nullptr, dz = dZ != nullptr, sum = dColsum != nullptr;
  const int nblocks = (rows + R - 1) / R;
  const bool vec = rows16(dG, ldg) && (!gate || rows16(dY, ldy)) && (!dz || rows16(dZ, ldz));
  ReluGradArgs a{dG, dY, dZ, dColsum, ldg, ldy, ldz, 0, rows, cols, R, accumulate ? 2 : 1};
  if (sum && nblocks > 1) {
    // the partial rows: nblocks x ldo floats of handle-owned workspace (16-byte rows), grown on demand as the quantiser's
    // buffers are.  Nothing can be allocated while the stream is capturing: such a call is refused (mmult_hip.h).
    a.ldo = ((long long)cols + 3) & ~3ll;
    const size_t need = (size_t)nblocks * (size_t)a.ldo * sizeof(float);
    // A captured launch bakes the workspace's address into its graph: from the first such call on, a buffer that has to grow
    // is RETIRED (freed with the handle), never freed under the graph -- the rule of the stream-K sets (state.hip).
    if (int rc = reserve_scratch(h, s, "mmh_relu_grad_colsum", {{&h->colsum_parts, need}}); rc != MMH_OK) return rc;
    a.out = static_cast<float *>(h->colsum_parts.p);
    a.direct = 0;
  }
  const int W = vec ? 4 : 1;
  const long long items = cols / W + cols % W;   // whole column groups, then the columns past them one by one (relu_grad.hpp)
  const long long chunks = (items + RG_THREADS - 1) / RG_THREADS;
  const dim3 grid((unsigned)nblocks, (unsigned)(chunks < 65535 ? chunks : 65535));
  if (vec) launch_pass<4>(gate, dz, sum, grid, s, a);
  else launch_pass<1>(gate, dz, sum, grid, s, a);
  if (sum && nblocks > 1)
    hipLaunchKernelGGL(colsum_finish_kernel, dim3((unsigned)((cols + RG_FIN_THREADS - 1) / RG_FIN_THREADS)), dim3(RG_FIN_THREADS), 0, s,
                       a.out, nblocks, a.ldo, cols, dColsum, accumulate ? 1 : 0);
  HIP_TRY(hipGetLastError());
  char tail[96] = "no colsum";
  if (sum)
    snprintf(tail, sizeof tail, "colsum %d block%s of %d rows%s%s", nblocks, nblocks == 1 ? "" : "s", R,
             nblocks == 1 ? ", written by the pass" : " + finish", accumulate ? ", accumulated" : "");
  char buf[192];
  snprintf(buf, sizeof buf, "relu_grad_colsum_kernel (%s path), gate %s, dz %s, %s", vec ? "vector" : "scalar", gate ? "on" : "off",
           dz ? "written" : "not written", tail);
  set_last_launch(buf);
  return MMH_OK;
}

}  // namespace mmh

using namespace mmh;

extern "C" int mmh_relu_grad_colsum(mmh_handle_t h, int rows, int cols, const float *dG, int ldg, const float *dY, int ldy, float *dZ,
                                    int ldz, float *dColsum, int accumulate, void *stream) {
  if (!h) return MMH_ERR_INVALID_ARG;
  if (int rc = relu_grad_check_args(rows, cols, dG, ldg, dY, ldy, dZ, ldz, dColsum); rc != MMH_OK) return rc;   // (before the device is touched)
  ENTER(h);
  return relu_grad_colsum_on(h, rows, cols, dG, ldg, dY, ldy, dZ, ldz, dColsum, accumulate, static_cast<hipStream_t>(stream));
}
