// q4g.hip -- libmmult_hip_q4g.so: the extern "C" entry points of include/mmult_hip_q4g.h and the kernels' launches.
// Stateless: no object, no allocation; the image, the groups' scales and the split-K partials live in the caller's memory.  Every
// argument is checked before the first device call; every entry point that touches the device restores the caller's.
#include <string>

#include "../../include/mmult_hip_q4g.h"
#include "q8_host.hpp"
#include "q4gdecode_plan.hpp"
#include "q4gdecode_s4.hpp"

using namespace mmh;

static_assert(kQdStrip == QD_STRIP && kQdSlice == IK && kQdMaxRows == QD_ROWS && kQdMaxRows == MMH_Q4G_MAX_ROWS &&
                  kQdFinishCols == QD_FINISH_COLS && kQ4SliceRows == Q4G_SLICE_ROWS && kQ4gGroup == MMH_Q4G_GROUP && kQ4gGroup == IK,
              "the plan's geometry is the kernels'");
// the accumulator restarts every slice and holds 16 x the group's sum: 128 * 128 per k over 128 k; the sum itself converts exactly
static_assert(128ll * 128 * MMH_Q4G_GROUP <= (1ll << 21) && ((128ll * 128 * MMH_Q4G_GROUP) >> 4) < (1ll << 24), "a group cannot overflow");

namespace {

struct Call {
  int device, rows, out, in;
  const int8_t *xq;
  int ldq;
  const float *rx;
  const uint8_t *wp4;
  int pitch_n;
  const float *gs;
  int pitch_s;
  const float *bias;
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

// csrc_q4d/q4d.hip's shape_status4 with the groups' factors: the same rules in the same order, then theirs (gs16: the base
// modulo 16)
int shape_status4g(const char *who, int rows, int out, int in, int ldq, int pitch_n, int pitch_s, int ldo, int xq4, int wp4, int gs16) {
  if (rows < 0 || out < 0 || in < 0) return MMH_ERR_INVALID_ARG;
  if (rows == 0) return MMH_OK;
  if (rows > MMH_Q4G_MAX_ROWS)
    return fail(MMH_ERR_UNSUPPORTED, std::string(who) + ": at most " + std::to_string(MMH_Q4G_MAX_ROWS) +
                " rows (MMH_Q4G_MAX_ROWS) -- there are no 4-bit tiles for larger batches");
  if (out == 0 || ldq < in || pitch_n < out || ldo < out || (in > 0 && pitch_s < out)) return MMH_ERR_INVALID_ARG;
  if (in > 0 && !(i8_dword(ldq, xq4) && i8_dword(pitch_n, wp4)))
    return fail(MMH_ERR_UNSUPPORTED, std::string(who) + ": the kernel reads the int8 rows and the packed image in dwords -- their "
                "pitches and base addresses must be multiples of 4");
  if (in > 0 && (pitch_s % 4 || gs16))
    return fail(MMH_ERR_UNSUPPORTED, std::string(who) + ": the kernel reads four group scales as one 16-byte vector -- pitch_s must be a "
                "multiple of 4 floats and the scales' base 16-byte aligned");
  if (!q4g_window(ldq, pitch_n, in, in > 0 ? pitch_s : 0))
    return fail(MMH_ERR_UNSUPPORTED, std::string(who) + ": the operands lie beyond the kernel's 2 GiB descriptor window");
  return MMH_OK;
}

int plan_refusal(const char *who) { return fail(MMH_ERR_INVALID_ARG, std::string(who) + ": the forced split count leaves a K range empty"); }

// Everything that needs no device.  (The workspace's SIZE is held to the plan of the device's CU count in linear_on, before
// its first launch; what no device's plan could do with is refused here.)
int call_status(const char *who, const Call &c) {
  if (c.device < 0 || !act_ok(c.activation) || c.splits < 0 || c.rows < 0 || c.out < 0 || c.in < 0) return MMH_ERR_INVALID_ARG;
  if (c.rows == 0) return MMH_OK;   // (nothing is read, nothing launched)
  if ((c.y != nullptr) == (c.yq != nullptr) || c.out8() != (c.yq != nullptr)) return MMH_ERR_INVALID_ARG;   // exactly one, and the scale's
  if (const int rc = shape_status4g(who, c.rows, c.out, c.in, c.ldq, c.pitch_n, c.pitch_s, c.ldo(), mod4(c.xq), mod4(c.wp4), mod16(c.gs));
      rc != MMH_OK)
    return rc;
  if ((c.in > 0 && (!c.xq || !c.wp4 || !c.gs)) || !c.rx) return MMH_ERR_INVALID_ARG;
  if (c.in > 0) {
    if (!c.work || mod16(c.work)) return MMH_ERR_INVALID_ARG;
    // a forced count is refused whatever the device (the CU count does not enter a forced plan); so is a workspace below what
    // the forced plan, or the smallest plan there is (one range), needs
    const QdPlan p = plan_q4gdecode(c.rows, c.out, c.in, c.out8(), c.ldo(), mod16(c.o()), c.splits, 256);
    if (!p.ok) return plan_refusal(who);
    if (c.work_bytes < (c.splits > 0 ? p.work_bytes : (((size_t)c.rows * p.wp * 4 + 15) & ~(size_t)15)))
      return fail(MMH_ERR_INVALID_ARG, std::string(who) + ": the workspace is smaller than the plan's work_bytes");
  }
  return MMH_OK;
}

// mmh_q4g_linear behind its argument checks, on the call's device
int linear_on(const char *who, const Call &c, hipStream_t s) {
  const QdPlan p = plan_q4gdecode(c.rows, c.out, c.in, c.out8(), c.ldo(), mod16(c.o()), c.splits, cu_count(c.device));
  if (c.in > 0 && c.work_bytes < p.work_bytes)
    return fail(MMH_ERR_INVALID_ARG, std::string(who) + ": the workspace is smaller than the plan's work_bytes");
  float *work = static_cast<float *>(c.work);
  if (c.in > 0) {
    hipLaunchKernelGGL(q4gdecode_partial_kernel, dim3((unsigned)p.strips, (unsigned)p.splits), dim3(QD_WAVES * 64), 0, s, c.rows, c.out,
                       c.in, p.k_len, c.xq, c.ldq, c.wp4, c.pitch_n, c.gs, c.pitch_s, work, p.wp);
    Q8_TRY(hipGetLastError());
  }
  const dim3 grid((unsigned)p.finish_x, (unsigned)c.rows);
  const int relu = c.activation == MMH_ACT_RELU ? 1 : 0;
  if (p.out8)
    hipLaunchKernelGGL(q4gdecode_finish_kernel<true>, grid, dim3(QD_FINISH_THREADS), 0, s, c.rows, c.out, p.splits, work, p.wp, c.rx,
                       c.bias, relu, c.so, static_cast<void *>(c.yq), c.ldyq, p.wide ? 1 : 0);
  else
    hipLaunchKernelGGL(q4gdecode_finish_kernel<false>, grid, dim3(QD_FINISH_THREADS), 0, s, c.rows, c.out, p.splits, work, p.wp, c.rx,
                       c.bias, relu, c.so, static_cast<void *>(c.y), c.ldy, p.wide ? 1 : 0);
  Q8_TRY(hipGetLastError());
  g_launch = p.text;
  return MMH_OK;
}

}  // namespace

extern "C" {

const char *mmh_q4g_last_error(void) { return g_error.c_str(); }
const char *mmh_q4g_last_launch(void) { return g_launch.c_str(); }

int mmh_q4g_weight_layout(int out, int in, int *pitch_n, int *packed_rows, int *groups, int *pitch_s, size_t *image_bytes,
                          size_t *scale_bytes) {
  if (out < 0 || in < 0 || !pitch_n || !packed_rows || !groups || !pitch_s || !image_bytes || !scale_bytes) return MMH_ERR_INVALID_ARG;
  *pitch_n = *pitch_s = (int)(((long)out + 15) & ~15L);
  *packed_rows = q4_packed_rows(in);
  *groups = q4g_groups(in);
  *image_bytes = (size_t)*packed_rows * (size_t)*pitch_n;
  *scale_bytes = (size_t)*groups * (size_t)*pitch_s * 4;
  return MMH_OK;
}

int mmh_q4g_pack_weight(int device, int out, int in, const float *dW, int ldw, void *dP, int pitch_n, float *d_group_scale,
                        float *d_group_inv_scale, int pitch_s, void *stream) {
  if (device < 0 || out < 0 || in < 0) return MMH_ERR_INVALID_ARG;
  if (out == 0 || in == 0) return MMH_OK;   // (no group, no packed row)
  if (!dW || !dP || !d_group_scale || !d_group_inv_scale || ldw < in || pitch_n < out || pitch_n % 16 || mod16(dP) || pitch_s < out)
    return MMH_ERR_INVALID_ARG;
  DeviceGuard guard;
  Q8_TRY(guard.enter(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int widest = pitch_n > pitch_s ? pitch_n : pitch_s;
  const dim3 grid((unsigned)q4g_groups(in), (unsigned)((widest + Q4G_PW_TILE - 1) / Q4G_PW_TILE));
  hipLaunchKernelGGL(q4g_pack_weight_kernel, grid, dim3(256), 0, s, dW, out, in, ldw, static_cast<uint8_t *>(dP), pitch_n, d_group_scale,
                     d_group_inv_scale, pitch_s);
  Q8_TRY(hipGetLastError());
  return MMH_OK;
}

int mmh_q4g_linear(int device, int rows, int out, int in, const int8_t *dXq, int ldq, const float *d_inv_scale, const void *dWp,
                   int pitch_n, const float *d_group_inv_scale, int pitch_s, const float *dBias, int activation,
                   const float *d_out_scale, float *dY, int ldy, int8_t *dYq, int ldyq, void *d_work, size_t work_bytes, int splits,
                   void *stream) {
  const Call c{device, rows, out,  in,  dXq,  ldq,    d_inv_scale, static_cast<const uint8_t *>(dWp), pitch_n, d_group_inv_scale, pitch_s, dBias,
               activation, d_out_scale, dY, ldy, dYq, ldyq, d_work, work_bytes, splits};
  if (const int rc = call_status("mmh_q4g_linear", c); rc != MMH_OK || rows == 0) return rc;
  DeviceGuard guard;
  Q8_TRY(guard.enter(device));
  return linear_on("mmh_q4g_linear", c, static_cast<hipStream_t>(stream));
}

int mmh_q4g_linear_plan(int rows, int out, int in, int ldq, int pitch_n, int pitch_s, int out8, int ldo, int xq_mod4, int wp_mod4,
                        int gs_mod16, int o_mod16, int splits, int cu_count, char *text, int text_bytes, size_t *work_bytes) {
  if (rows <= 0 || out <= 0 || ((xq_mod4 | wp_mod4) & ~3) || ((o_mod16 | gs_mod16) & ~15) || (out8 & ~1) || splits < 0 || !text ||
      text_bytes <= 0 || !work_bytes)
    return MMH_ERR_INVALID_ARG;
  if (const int rc = shape_status4g("mmh_q4g_linear_plan", rows, out, in, ldq, pitch_n, pitch_s, ldo, xq_mod4, wp_mod4, gs_mod16); rc != MMH_OK)
    return rc;
  const QdPlan p = plan_q4gdecode(rows, out, in, out8 != 0, ldo, o_mod16, splits, cu_count > 0 ? cu_count : 256);
  if (!p.ok) return plan_refusal("mmh_q4g_linear_plan");
  snprintf(text, (size_t)text_bytes, "%s", p.text);
  *work_bytes = p.work_bytes;
  return MMH_OK;
}

int mmh_time_q4g_linear(int device, int rows, int out, int in, const int8_t *dXq, int ldq, const float *d_inv_scale,
                        const void *dWp, int pitch_n, const float *d_group_inv_scale, int pitch_s, const float *dBias, int activation,
                        const float *d_out_scale, float *dY, int ldy, int8_t *dYq, int ldyq, void *d_work, size_t work_bytes,
                        int splits, int warmup, int reps, void *stream, float *ms_per_call) {
  if (reps <= 0 || warmup < 0 || !ms_per_call) return MMH_ERR_INVALID_ARG;
  const Call c{device, rows, out,  in,  dXq,  ldq,    d_inv_scale, static_cast<const uint8_t *>(dWp), pitch_n, d_group_inv_scale, pitch_s, dBias,
               activation, d_out_scale, dY, ldy, dYq, ldyq, d_work, work_bytes, splits};
  if (const int rc = call_status("mmh_time_q4g_linear", c); rc != MMH_OK) return rc;
  if (rows == 0) return MMH_ERR_INVALID_ARG;   // (nothing to time)
  DeviceGuard guard;
  Q8_TRY(guard.enter(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  return timed("mmh_time_q4g_linear", warmup, reps, s, ms_per_call, [&] { return linear_on("mmh_time_q4g_linear", c, s); });
}

}  // extern "C"
