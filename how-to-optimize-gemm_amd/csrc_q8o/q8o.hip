// q8o.hip -- the host side of libmmult_hip_q8o.so: the extern "C" entry points of include/mmult_hip_q8o.h.  Stateless: no
// object, no scratch, no allocation.  The GEMM's instantiations live in qlinear_s8o_*.hip.  Every argument is checked before
// the first device call; every entry point that touches the device restores the caller's.
#include <atomic>
#include <string>

#include "../../include/mmult_hip_q8o.h"
#include "qlinear_s8o.hpp"
#include "qlinear_s8o_plan.hpp"

using namespace mmh;

namespace {

thread_local std::string g_error, g_launch;

int fail(int status, const std::string &text) {
  g_error = text;
  return status;
}
int hip_fail(hipError_t e, const char *what) { return fail(MMH_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
#define Q8O_TRY(expr)                                 \
  do {                                                \
    hipError_t e_ = (expr);                           \
    if (e_ != hipSuccess) return hip_fail(e_, #expr); \
  } while (0)

struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  hipError_t enter(int device) {
    hipError_t e = hipGetDevice(&prev);
    if (e != hipSuccess || prev == device) return e;
    e = hipSetDevice(device);
    switched = e == hipSuccess;
    return e;
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};

int mod4(const void *p) { return (int)(reinterpret_cast<uintptr_t>(p) & 3); }
bool act_ok(int activation) { return activation == MMH_ACT_NONE || activation == MMH_ACT_RELU; }

// The shape's and the layout's rules, shared by the call and its plan (mods: the bases modulo 4)
int shape_status(const char *who, int rows, int out, int in, int ldq, int pitch_n, int ldyq, int xq4, int wq4) {
  if (rows < 0 || out < 0 || in < 0) return MMH_ERR_INVALID_ARG;
  if (rows == 0) return MMH_OK;
  if (out == 0 || ldq < in || pitch_n < out || ldyq < out) return MMH_ERR_INVALID_ARG;
  if (in > 0 && !(i8_dword(ldq, xq4) && i8_dword(pitch_n, wq4)))
    return fail(MMH_ERR_UNSUPPORTED, std::string(who) + ": the tile reads the int8 rows and the weight image in dwords -- their pitches "
                "and base addresses must be multiples of 4");
  if (!i8_window(ldq, pitch_n, in))
    return fail(MMH_ERR_UNSUPPORTED, std::string(who) + ": the operands lie beyond the GEMM's 2 GiB descriptor window");
  return MMH_OK;
}

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
  if (const int rc = shape_status(who, c.rows, c.out, c.in, c.ldq, c.pitch_n, c.ldyq, mod4(c.xq), mod4(c.wq)); rc != MMH_OK || c.rows == 0)
    return rc;
  if ((c.in > 0 && (!c.xq || !c.wq)) || !c.rx || !c.rw || !c.so || !c.yq) return MMH_ERR_INVALID_ARG;
  return MMH_OK;
}

// the device's CU count, asked once per device (the plan's only input that is not an argument)
int cu_count(int device) {
  static std::atomic<int> known[64];
  if (device < 64 && known[device].load(std::memory_order_relaxed) > 0) return known[device].load(std::memory_order_relaxed);
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
  if (device < 64) known[device].store(cus, std::memory_order_relaxed);
  return cus;
}

// mmh_q8o_linear behind its argument checks, on the call's device
int linear_on(const Call &c, hipStream_t s) {
  const Q8oPlan p = plan_qlinear_s8o(c.rows, c.out, c.ldyq, mod4(c.yq), cu_count(c.device));
  const QlinearS8oArgs g{c.rows, c.out, c.in, c.xq, c.ldq, c.wq, c.pitch_n, c.rx, c.rw, c.bias, c.activation == MMH_ACT_RELU ? 1 : 0,
                         c.so, c.yq, c.ldyq, p.dwords ? 1 : 0, p.nbm, p.nbn};
  Q8O_TRY(p.tile == 256 ? (p.edge ? launch_qlinear_s8o_256_edge(g, s) : launch_qlinear_s8o_256(g, s))
                        : (p.edge ? launch_qlinear_s8o_128_edge(g, s) : launch_qlinear_s8o_128(g, s)));
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
  Q8O_TRY(guard.enter(device));
  return linear_on(c, static_cast<hipStream_t>(stream));
}

int mmh_q8o_linear_plan(int rows, int out, int in, int ldq, int pitch_n, int ldyq, int xq_mod4, int wq_mod4, int yq_mod4,
                        int cu_count, char *text, int text_bytes) {
  if (rows <= 0 || out <= 0 || ((xq_mod4 | wq_mod4 | yq_mod4) & ~3) || !text || text_bytes <= 0) return MMH_ERR_INVALID_ARG;
  if (const int rc = shape_status("mmh_q8o_linear_plan", rows, out, in, ldq, pitch_n, ldyq, xq_mod4, wq_mod4); rc != MMH_OK) return rc;
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
  Q8O_TRY(guard.enter(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc = MMH_OK;
  for (int i = 0; i < warmup && rc == MMH_OK; ++i) rc = linear_on(c, s);
  if (rc != MMH_OK) return rc;
  hipEvent_t t0 = nullptr, t1 = nullptr;
  hipError_t e = hipEventCreate(&t0);
  if (e == hipSuccess) e = hipEventCreate(&t1);
  if (e == hipSuccess) e = hipEventRecord(t0, s);
  for (int i = 0; i < reps && rc == MMH_OK && e == hipSuccess; ++i) rc = linear_on(c, s);
  float ms = 0.f;
  if (rc == MMH_OK && e == hipSuccess) e = hipEventRecord(t1, s);
  if (rc == MMH_OK && e == hipSuccess) e = hipEventSynchronize(t1);
  if (rc == MMH_OK && e == hipSuccess) e = hipEventElapsedTime(&ms, t0, t1);
  if (t0) (void)hipEventDestroy(t0);
  if (t1) (void)hipEventDestroy(t1);
  if (rc != MMH_OK) return rc;
  if (e != hipSuccess) return hip_fail(e, "mmh_time_q8o_linear");
  *ms_per_call = ms / reps;
  return MMH_OK;
}

}  // extern "C"
