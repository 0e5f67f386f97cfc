// q8d.hip -- libmmult_hip_q8d.so: the extern "C" entry points of include/mmult_hip_q8d.h and the two kernels' launches.
// Stateless: no object, no allocation; the split-K partials live in the caller's workspace.  Every argument is checked before the
// first device call; every entry point that touches the device restores the caller's.
#include <string>

#include "../../include/mmult_hip_q8d.h"
#include "q8_host.hpp"
#include "qdecode_plan.hpp"
#include "qdecode_s8.hpp"

using namespace mmh;

static_assert(kQdStrip == QD_STRIP && kQdSlice == IK && kQdMaxRows == QD_ROWS && kQdMaxRows == MMH_Q8D_MAX_ROWS &&
                  kQdFinishCols == QD_FINISH_COLS,
              "the plan's geometry is the kernels'");

namespace {

constexpr ShapeRules kShape{"kernel", "kernel", kQdMaxRows};   // mmh_q8o_linear's rules, and at most 16 rows

struct Call {
  int device, rows, out, in;
  const int8_t *xq;
  int ldq;
  const float *rx;
  const int8_t *wq;
  int pitch_n;
  const float *rw, *bias;
  int activation;
  const float *so;
  float *y;
  int ldy;
  int8_t *yq;
  int ldyq;
  void *work;
  size_t work_bytes;
  int splits;
  bool out8() const { return so != nullptr; }
  int ldo() const { return out8() ? ldyq : ldy; }
  const void *o() const { return out8() ? static_cast<const void *>(yq) : y; }
};

// Everything that needs no device.  (The workspace's SIZE is held to the plan of the device's CU count: linear_on, before its
// first launch.)
int call_status(const char *who, const Call &c) {
  if (c.device < 0 || !act_ok(c.activation) || c.splits < 0 || c.rows < 0 || c.out < 0 || c.in < 0) return MMH_ERR_INVALID_ARG;
  if (c.rows == 0) return MMH_OK;   // (nothing is read, nothing launched)
  if ((c.y != nullptr) == (c.yq != nullptr) || c.out8() != (c.yq != nullptr)) return MMH_ERR_INVALID_ARG;   // exactly one, and the scale's
  if (const int rc = shape_status(who, kShape, c.rows, c.out, c.in, c.ldq, c.pitch_n, c.ldo(), mod4(c.xq), mod4(c.wq)); rc != MMH_OK || c.rows == 0)
    return rc;
  if ((c.in > 0 && (!c.xq || !c.wq)) || !c.rx || !c.rw) return MMH_ERR_INVALID_ARG;
  if (c.in > 0) {
    if (!c.work || mod16(c.work)) return MMH_ERR_INVALID_ARG;
    // a forced count that leaves a range empty is refused whatever the device (the CU count does not enter a forced plan)
    if (c.splits > 0 && !plan_qdecode(c.rows, c.out, c.in, c.out8(), c.ldo(), mod16(c.o()), c.splits, 256).ok)
      return fail(MMH_ERR_INVALID_ARG, std::string(who) + ": the forced split count leaves a K range empty");
  }
  return MMH_OK;
}

// mmh_q8d_linear behind its argument checks, on the call's device
int linear_on(const char *who, const Call &c, hipStream_t s) {
  const QdPlan p = plan_qdecode(c.rows, c.out, c.in, c.out8(), c.ldo(), mod16(c.o()), c.splits, cu_count(c.device));
  if (c.in > 0 && c.work_bytes < p.work_bytes)
    return fail(MMH_ERR_INVALID_ARG, std::string(who) + ": the workspace is smaller than the plan's work_bytes");
  int32_t *work = static_cast<int32_t *>(c.work);
  if (c.in > 0) {
    hipLaunchKernelGGL(qdecode_partial_kernel, dim3((unsigned)p.strips, (unsigned)p.splits), dim3(QD_WAVES * 64), 0, s, c.rows, c.out,
                       c.in, p.k_len, c.xq, c.ldq, c.wq, c.pitch_n, work, p.wp);
    Q8_TRY(hipGetLastError());
  }
  const dim3 grid((unsigned)p.finish_x, (unsigned)c.rows);
  const int relu = c.activation == MMH_ACT_RELU ? 1 : 0;
  if (p.out8)
    hipLaunchKernelGGL(qdecode_finish_kernel<true>, grid, dim3(QD_FINISH_THREADS), 0, s, c.rows, c.out, p.splits, work, p.wp, c.rx, c.rw,
                       c.bias, relu, c.so, static_cast<void *>(c.yq), c.ldyq, p.wide ? 1 : 0);
  else
    hipLaunchKernelGGL(qdecode_finish_kernel<false>, grid, dim3(QD_FINISH_THREADS), 0, s, c.rows, c.out, p.splits, work, p.wp, c.rx, c.rw,
                       c.bias, relu, c.so, static_cast<void *>(c.y), c.ldy, p.wide ? 1 : 0);
  Q8_TRY(hipGetLastError());
  g_launch = p.text;
  return MMH_OK;
}

}  // namespace

extern "C" {

const char *mmh_q8d_last_error(void) { return g_error.c_str(); }
const char *mmh_q8d_last_launch(void) { return g_launch.c_str(); }

int mmh_q8d_linear(int device, int rows, int out, int in, const int8_t *dXq, int ldq, const float *d_inv_scale, const int8_t *dWq,
                   int pitch_n, const float *d_w_inv_scale, const float *dBias, int activation, const float *d_out_scale,
                   float *dY, int ldy, int8_t *dYq, int ldyq, void *d_work, size_t work_bytes, int splits, void *stream) {
  const Call c{device, rows, out,   in,  dXq,  ldq,  d_inv_scale, dWq,        pitch_n, d_w_inv_scale, dBias, activation, d_out_scale,
               dY,     ldy,  dYq,   ldyq, d_work, work_bytes, splits};
  if (const int rc = call_status("mmh_q8d_linear", c); rc != MMH_OK || rows == 0) return rc;
  DeviceGuard guard;
  Q8_TRY(guard.enter(device));
  return linear_on("mmh_q8d_linear", c, static_cast<hipStream_t>(stream));
}

int mmh_q8d_linear_plan(int rows, int out, int in, int ldq, int pitch_n, int out8, int ldo, int xq_mod4, int wq_mod4, int o_mod16,
                        int splits, int cu_count, char *text, int text_bytes, size_t *work_bytes) {
  if (rows <= 0 || out <= 0 || ((xq_mod4 | wq_mod4) & ~3) || (o_mod16 & ~15) || (out8 & ~1) || splits < 0 || !text || text_bytes <= 0 ||
      !work_bytes)
    return MMH_ERR_INVALID_ARG;
  if (const int rc = shape_status("mmh_q8d_linear_plan", kShape, rows, out, in, ldq, pitch_n, ldo, xq_mod4, wq_mod4); rc != MMH_OK) return rc;
  const QdPlan p = plan_qdecode(rows, out, in, out8 != 0, ldo, o_mod16, splits, cu_count > 0 ? cu_count : 256);
  if (!p.ok) return fail(MMH_ERR_INVALID_ARG, "mmh_q8d_linear_plan: the forced split count leaves a K range empty");
  snprintf(text, (size_t)text_bytes, "%s", p.text);
  *work_bytes = p.work_bytes;
  return MMH_OK;
}

int mmh_time_q8d_linear(int device, int rows, int out, int in, const int8_t *dXq, int ldq, const float *d_inv_scale,
                        const int8_t *dWq, int pitch_n, const float *d_w_inv_scale, const float *dBias, int activation,
                        const float *d_out_scale, float *dY, int ldy, int8_t *dYq, int ldyq, void *d_work, size_t work_bytes,
                        int splits, int warmup, int reps, void *stream, float *ms_per_call) {
  if (reps <= 0 || warmup < 0 || !ms_per_call) return MMH_ERR_INVALID_ARG;
  const Call c{device, rows, out,   in,  dXq,  ldq,  d_inv_scale, dWq,        pitch_n, d_w_inv_scale, dBias, activation, d_out_scale,
               dY,     ldy,  dYq,   ldyq, d_work, work_bytes, splits};
  if (const int rc = call_status("mmh_time_q8d_linear", c); rc != MMH_OK) return rc;
  if (rows == 0) return MMH_ERR_INVALID_ARG;   // (nothing to time)
  DeviceGuard guard;
  Q8_TRY(guard.enter(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  return timed("mmh_time_q8d_linear", warmup, reps, s, ms_per_call, [&] { return linear_on("mmh_time_q8d_linear", c, s); });
}

}  // extern "C"
