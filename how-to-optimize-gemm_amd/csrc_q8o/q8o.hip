// q8o.hip -- the host side of libmmult_hip_q8o.so: the extern "C" entry points of include/mmult_hip_q8o.h.  Stateless: no
// object, no scratch, no allocation.  The GEMM's instantiations live in qlinear_s8o_*.hip.  Every argument is checked before
// the first device call; every entry point that touches the device restores the caller's.
#include <string>

#include "../../include/mmult_hip_q8o.h"
#include "q8_host.hpp"
#include "qlinear_s8o.hpp"
#include "qlinear_s8o_plan.hpp"

using namespace mmh;

namespace {

constexpr ShapeRules kShape{"tile", "GEMM", 0};

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
  int8_t *yq;
  int ldyq;
};

int call_status(const char *who, const Call &c) {
  if (c.device < 0 || !act_ok(c.activation)) return MMH_ERR_INVALID_ARG;
  if (const int rc = shape_status(who, kShape, c.rows, c.out, c.in, c.ldq, c.pitch_n, c.ldyq, mod4(c.xq), mod4(c.wq)); rc != MMH_OK || c.rows == 0)
    return rc;
  if ((c.in > 0 && (!c.xq || !c.wq)) || !c.rx || !c.rw || !c.so || !c.yq) return MMH_ERR_INVALID_ARG;
  return MMH_OK;
}

// mmh_q8o_linear behind its argument checks, on the call's device
int linear_on(const Call &c, hipStream_t s) {
  const Q8oPlan p = plan_qlinear_s8o(c.rows, c.out, c.ldyq, mod4(c.yq), cu_count(c.device));
  const QlinearS8oArgs g{c.rows, c.out, c.in, c.xq, c.ldq, c.wq, c.pitch_n, c.rx, c.rw, c.bias, c.activation == MMH_ACT_RELU ? 1 : 0,
                         c.so, c.yq, c.ldyq, p.dwords ? 1 : 0, p.nbm, p.nbn};
  Q8_TRY(launch_qlinear_s8o(p, g, s));
  g_launch = p.text;
  return MMH_OK;
}

}  // namespace

extern "C" {

const char *mmh_q8o_last_error(void) { return g_error.c_str(); }
const char *mmh_q8o_last_launch(void) { return g_launch.c_str(); }

int mmh_q8o_linear(int device, int rows, int out, int in, const int8_t *dXq, int ldq, const float *d_inv_scale, const int8_t *dWq,
                   int pitch_n, const float *d_w_inv_scale, const float *dBias, int activation, const float *d_out_scale,
                   int8_t *dYq, int ldyq, void *stream) {
  const Call c{device, rows, out, in, dXq, ldq, d_inv_scale, dWq, pitch_n, d_w_inv_scale, dBias, activation, d_out_scale, dYq, ldyq};
  if (const int rc = call_status("mmh_q8o_linear", c); rc != MMH_OK || rows == 0) return rc;
  DeviceGuard guard;
  Q8_TRY(guard.enter(device));
  return linear_on(c, static_cast<hipStream_t>(stream));
}

int mmh_q8o_linear_plan(int rows, int out, int in, int ldq, int pitch_n, int ldyq, int xq_mod4, int wq_mod4, int yq_mod4,
                        int cu_count, char *text, int text_bytes) {
  if (rows <= 0 || out <= 0 || ((xq_mod4 | wq_mod4 | yq_mod4) & ~3) || !text || text_bytes <= 0) return MMH_ERR_INVALID_ARG;
  if (const int rc = shape_status("mmh_q8o_linear_plan", kShape, rows, out, in, ldq, pitch_n, ldyq, xq_mod4, wq_mod4); rc != MMH_OK) return rc;
  const Q8oPlan p = plan_qlinear_s8o(rows, out, ldyq, yq_mod4, cu_count > 0 ? cu_count : 256);
  snprintf(text, (size_t)text_bytes, "%s", p.text);
  return MMH_OK;
}

int mmh_time_q8o_linear(int device, int rows, int out, int in, const int8_t *dXq, int ldq, const float *d_inv_scale,
                        const int8_t *dWq, int pitch_n, const float *d_w_inv_scale, const float *dBias, int activation,
                        const float *d_out_scale, int8_t *dYq, int ldyq, int warmup, int reps, void *stream, float *ms_per_call) {
  if (reps <= 0 || warmup < 0 || !ms_per_call) return MMH_ERR_INVALID_ARG;
  const Call c{device, rows, out, in, dXq, ldq, d_inv_scale, dWq, pitch_n, d_w_inv_scale, dBias, activation, d_out_scale, dYq, ldyq};
  if (const int rc = call_status("mmh_time_q8o_linear", c); rc != MMH_OK) return rc;
  if (rows == 0) return MMH_ERR_INVALID_ARG;   // (nothing to time)
  DeviceGuard guard;
  Q8_TRY(guard.enter(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  return timed("mmh_time_q8o_linear", warmup, reps, s, ms_per_call, [&] { return linear_on(c, s); });
}

}  // extern "C"
