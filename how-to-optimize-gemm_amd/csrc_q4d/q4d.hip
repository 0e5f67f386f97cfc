// q4d.hip -- libmmult_hip_q4d.so: the extern "C" entry points of include/mmult_hip_q4d.h and the kernels' launches.
// Stateless: no object, no allocation; the images, the scales and the split-K partials live in the caller's memory.  Every
// argument is checked before the first device call; every entry point that touches the device restores the caller's.
#include <string>

#include "../../include/mmult_hip_q4d.h"
#include "q8_host.hpp"
#include "q4decode_plan.hpp"
#include "q4decode_s4.hpp"

using namespace mmh;

static_assert(kQdStrip == QD_STRIP && kQdSlice == IK && kQdMaxRows == QD_ROWS && kQdMaxRows == MMH_Q4D_MAX_ROWS &&
                  kQdFinishCols == QD_FINISH_COLS && kQ4SliceRows == Q4_SLICE_ROWS && kQ4MaxRangeK == MMH_Q4D_MAX_RANGE_K,
              "the plan's geometry is the kernels'");
// the accumulator holds 16 x the sum: 128 * 128 per k, below 2^31 over the longest range
static_assert((long long)128 * 128 * MMH_Q4D_MAX_RANGE_K < (1ll << 31), "a range of MMH_Q4D_MAX_RANGE_K k cannot overflow");

namespace {

struct Call {
  int device, rows, out, in;
  const int8_t *xq;
  int ldq;
  const float *rx;
  const uint8_t *wp4;
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

// q8_host.hpp's shape_status for int8 rows and a PACKED image: the same rules in the same order, the image's own window
int shape_status4(const char *who, int rows, int out, int in, int ldq, int pitch_n, int ldo, int xq4, int wp4) {
  if (rows < 0 || out < 0 || in < 0) return MMH_ERR_INVALID_ARG;
  if (rows == 0) return MMH_OK;
  if (rows > MMH_Q4D_MAX_ROWS)
    return fail(MMH_ERR_UNSUPPORTED, std::string(who) + ": at most " + std::to_string(MMH_Q4D_MAX_ROWS) +
                " rows (MMH_Q4D_MAX_ROWS) -- there are no 4-bit tiles for larger batches");
  if (out == 0 || ldq < in || pitch_n < out || ldo < out) return MMH_ERR_INVALID_ARG;
  if (in > 0 && !(i8_dword(ldq, xq4) && i8_dword(pitch_n, wp4)))
    return fail(MMH_ERR_UNSUPPORTED, std::string(who) + ": the kernel reads the int8 rows and the packed image in dwords -- their "
                "pitches and base addresses must be multiples of 4");
  if (!q4_window(ldq, pitch_n, in))
    return fail(MMH_ERR_UNSUPPORTED, std::string(who) + ": the operands lie beyond the kernel's 2 GiB descriptor window");
  return MMH_OK;
}

int plan_refusal(const char *who, const Q4Plan &p) {
  return fail(MMH_ERR_INVALID_ARG, std::string(who) + (p.long_range ? ": the forced split count leaves a K range longer than 65536 k "
                                                                       "(MMH_Q4D_MAX_RANGE_K)"
                                                                     : ": the forced split count leaves a K range empty"));
}

// Everything that needs no device.  (The workspace's SIZE is held to the plan of the device's CU count in linear_on, before
// its first launch; what no device's plan could do with is refused here.)
int call_status(const char *who, const Call &c) {
  if (c.device < 0 || !act_ok(c.activation) || c.splits < 0 || c.rows < 0 || c.out < 0 || c.in < 0) return MMH_ERR_INVALID_ARG;
  if (c.rows == 0) return MMH_OK;   // (nothing is read, nothing launched)
  if ((c.y != nullptr) == (c.yq != nullptr) || c.out8() != (c.yq != nullptr)) return MMH_ERR_INVALID_ARG;   // exactly one, and the scale's
  if (const int rc = shape_status4(who, c.rows, c.out, c.in, c.ldq, c.pitch_n, c.ldo(), mod4(c.xq), mod4(c.wp4)); rc != MMH_OK) return rc;
  if ((c.in > 0 && (!c.xq || !c.wp4)) || !c.rx || !c.rw) return MMH_ERR_INVALID_ARG;
  if (c.in > 0) {
    if (!c.work || mod16(c.work)) return MMH_ERR_INVALID_ARG;
    // a forced count is refused whatever the device (the CU count does not enter a forced plan); so is a workspace below what
    // the forced plan, or the smallest plan there is (one range), needs
    const Q4Plan p = plan_q4decode(c.rows, c.out, c.in, c.out8(), c.ldo(), mod16(c.o()), c.splits, 256);
    if (!p.ok) return plan_refusal(who, p);
    if (c.work_bytes < (c.splits > 0 ? p.work_bytes : (((size_t)c.rows * p.wp * 4 + 15) & ~(size_t)15)))
      return fail(MMH_ERR_INVALID_ARG, std::string(who) + ": the workspace is smaller than the plan's work_bytes");
  }
  return MMH_OK;
}

// mmh_q4d_linear behind its argument checks, on the call's device
int linear_on(const char *who, const Call &c, hipStream_t s) {
  const Q4Plan p = plan_q4decode(c.rows, c.out, c.in, c.out8(), c.ldo(), mod16(c.o()), c.splits, cu_count(c.device));
  if (c.in > 0 && c.work_bytes < p.work_bytes)
    return fail(MMH_ERR_INVALID_ARG, std::string(who) + ": the workspace is smaller than the plan's work_bytes");
  int32_t *work = static_cast<int32_t *>(c.work);
  if (c.in > 0) {
    hipLaunchKernelGGL(q4decode_partial_kernel, dim3((unsigned)p.strips, (unsigned)p.splits), dim3(QD_WAVES * 64), 0, s, c.rows, c.out,
                       c.in, p.k_len, c.xq, c.ldq, c.wp4, c.pitch_n, work, p.wp);
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

const char *mmh_q4d_last_error(void) { return g_error.c_str(); }
const char *mmh_q4d_last_launch(void) { return g_launch.c_str(); }

int mmh_q4d_weight_layout(int out, int in, int *pitch_n, int *packed_rows, size_t *bytes) {
  if (out < 0 || in < 0 || !pitch_n || !packed_rows || !bytes) return MMH_ERR_INVALID_ARG;
  *pitch_n = (int)(((long)out + 15) & ~15L);
  *packed_rows = q4_packed_rows(in);
  *bytes = (size_t)*packed_rows * (size_t)*pitch_n;
  return MMH_OK;
}

int mmh_q4d_pack_weight(int device, int out, int in, const float *dW, int ldw, void *dP, int pitch_n, float *d_scale,
                        float *d_inv_scale, void *stream) {
  if (device < 0 || out < 0 || in < 0) return MMH_ERR_INVALID_ARG;
  if (out == 0) return MMH_OK;
  if (!d_scale || !d_inv_scale || ldw < in) return MMH_ERR_INVALID_ARG;
  if (in > 0 && (!dW || !dP || pitch_n < out || pitch_n % 16 || mod16(dP))) return MMH_ERR_INVALID_ARG;
  DeviceGuard guard;
  Q8_TRY(guard.enter(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(q4_row_amax_kernel, dim3((unsigned)out), dim3(256), 0, s, dW, in, ldw, d_scale, d_inv_scale);
  Q8_TRY(hipGetLastError());
  if (in > 0) {
    const dim3 grid((unsigned)((in + IK - 1) / IK), (unsigned)((pitch_n + Q4_PW_TILE - 1) / Q4_PW_TILE));
    hipLaunchKernelGGL(q4_pack_weight_kernel, grid, dim3(256), 0, s, dW, out, in, ldw, d_scale, static_cast<uint8_t *>(dP), pitch_n);
    Q8_TRY(hipGetLastError());
  }
  return MMH_OK;
}

int mmh_q4d_linear(int device, int rows, int out, int in, const int8_t *dXq, int ldq, const float *d_inv_scale, const void *dWp,
                   int pitch_n, const float *d_w_inv_scale, const float *dBias, int activation, const float *d_out_scale,
                   float *dY, int ldy, int8_t *dYq, int ldyq, void *d_work, size_t work_bytes, int splits, void *stream) {
  const Call c{device, rows, out,  in,  dXq,  ldq,    d_inv_scale, static_cast<const uint8_t *>(dWp), pitch_n, d_w_inv_scale, dBias, activation,
               d_out_scale, dY, ldy, dYq, ldyq, d_work, work_bytes,  splits};
  if (const int rc = call_status("mmh_q4d_linear", c); rc != MMH_OK || rows == 0) return rc;
  DeviceGuard guard;
  Q8_TRY(guard.enter(device));
  return linear_on("mmh_q4d_linear", c, static_cast<hipStream_t>(stream));
}

int mmh_q4d_linear_plan(int rows, int out, int in, int ldq, int pitch_n, int out8, int ldo, int xq_mod4, int wp_mod4, int o_mod16,
                        int splits, int cu_count, char *text, int text_bytes, size_t *work_bytes) {
  if (rows <= 0 || out <= 0 || ((xq_mod4 | wp_mod4) & ~3) || (o_mod16 & ~15) || (out8 & ~1) || splits < 0 || !text || text_bytes <= 0 ||
      !work_bytes)
    return MMH_ERR_INVALID_ARG;
  if (const int rc = shape_status4("mmh_q4d_linear_plan", rows, out, in, ldq, pitch_n, ldo, xq_mod4, wp_mod4); rc != MMH_OK) return rc;
  const Q4Plan p = plan_q4decode(rows, out, in, out8 != 0, ldo, o_mod16, splits, cu_count > 0 ? cu_count : 256);
  if (!p.ok) return plan_refusal("mmh_q4d_linear_plan", p);
  snprintf(text, (size_t)text_bytes, "%s", p.text);
  *work_bytes = p.work_bytes;
  return MMH_OK;
}

int mmh_time_q4d_linear(int device, int rows, int out, int in, const int8_t *dXq, int ldq, const float *d_inv_scale,
                        const void *dWp, int pitch_n, const float *d_w_inv_scale, const float *dBias, int activation,
                        const float *d_out_scale, float *dY, int ldy, int8_t *dYq, int ldyq, void *d_work, size_t work_bytes,
                        int splits, int warmup, int reps, void *stream, float *ms_per_call) {
  if (reps <= 0 || warmup < 0 || !ms_per_call) return MMH_ERR_INVALID_ARG;
  const Call c{device, rows, out,  in,  dXq,  ldq,    d_inv_scale, static_cast<const uint8_t *>(dWp), pitch_n, d_w_inv_scale, dBias, activation,
               d_out_scale, dY, ldy, dYq, ldyq, d_work, work_bytes,  splits};
  if (const int rc = call_status("mmh_time_q4d_linear", c); rc != MMH_OK) return rc;
  if (rows == 0) return MMH_ERR_INVALID_ARG;   // (nothing to time)
  DeviceGuard guard;
  Q8_TRY(guard.enter(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  return timed("mmh_time_q4d_linear", warmup, reps, s, ms_per_call, [&] { return linear_on("mmh_time_q4d_linear", c, s); });
}

}  // extern "C"
