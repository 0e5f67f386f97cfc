// q8_host.hpp -- what the host sides of the int8 layer libraries share: q8.hip, q8o.hip and q8d.hip each include it once, after
// their C header.  The per-thread error and launch texts, the argument rules that need no device, the cached CU count and the
// timing loop; csrc/device_memory.hpp's device guard and owners come with it.  Everything here has internal linkage: each .so
// keeps its own state, and an error in one library never shows in another's mmh_*_last_error.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <string>

#include "../../include/mmult_hip.h"   // the statuses, MMH_ACT_*
#include "device_memory.hpp"           // mmh::capturing, DeviceGuard, DevBuf / GraphBuf / Retired
#include "igemm_plan.hpp"              // i8_dword, i8_window

namespace {

thread_local std::string g_error, g_launch;   // mmh_*_last_error, mmh_*_last_launch

int fail(int status, const std::string &text) {
  g_error = text;
  return status;
}
int hip_fail(hipError_t e, const char *what) { return fail(MMH_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
#define Q8_TRY(expr)                                  \
  do {                                                \
    hipError_t e_ = (expr);                           \
    if (e_ != hipSuccess) return hip_fail(e_, #expr); \
  } while (0)

[[maybe_unused]] int mod4(const void *p) { return (int)(reinterpret_cast<uintptr_t>(p) & 3); }
[[maybe_unused]] int mod16(const void *p) { return (int)(reinterpret_cast<uintptr_t>(p) & 15); }
bool act_ok(int activation) { return activation == MMH_ACT_NONE || activation == MMH_ACT_RELU; }

// The device's CU count, asked once per device (a stateless library's plan has no other input that is not an argument)
[[maybe_unused]] int cu_count(int device) {
  static std::atomic<int> known[64];
  if (device < 64 && known[device].load(std::memory_order_relaxed) > 0) return known[device].load(std::memory_order_relaxed);
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
  if (device < 64) known[device].store(cus, std::memory_order_relaxed);
  return cus;
}

// The shape's and the layout's rules of a call on int8 rows and a weight image, shared by the call and its plan (xq4, wq4: the
// bases modulo 4).  ShapeRules: what reads the operands and whose descriptor window they lie in, as the messages name them, and
// the most rows a call takes (0: no cap; the small-batch library's MMH_Q8D_MAX_ROWS is the one cap there is).
struct ShapeRules {
  const char *reader, *owner;
  int max_rows;
};
[[maybe_unused]] int shape_status(const char *who, const ShapeRules &r, int rows, int out, int in, int ldq, int pitch_n, int ldo, int xq4,
                                  int wq4) {
  if (rows < 0 || out < 0 || in < 0) return MMH_ERR_INVALID_ARG;
  if (rows == 0) return MMH_OK;
  if (r.max_rows && rows > r.max_rows)
    return fail(MMH_ERR_UNSUPPORTED, std::string(who) + ": at most " + std::to_string(r.max_rows) +
                " rows (MMH_Q8D_MAX_ROWS) -- larger batches are the tile path's");
  if (out == 0 || ldq < in || pitch_n < out || ldo < out) return MMH_ERR_INVALID_ARG;
  if (in > 0 && !(mmh::i8_dword(ldq, xq4) && mmh::i8_dword(pitch_n, wq4)))
    return fail(MMH_ERR_UNSUPPORTED, std::string(who) + ": the " + r.reader + " reads the int8 rows and the weight image in dwords -- their "
                "pitches and base addresses must be multiples of 4");
  if (!mmh::i8_window(ldq, pitch_n, in))
    return fail(MMH_ERR_UNSUPPORTED, std::string(who) + ": the operands lie beyond the " + r.owner + "'s 2 GiB descriptor window");
  return MMH_OK;
}

// Mean milliseconds of `reps` calls behind `warmup` untimed ones, one event pair around them; call() is a linear_on on the
// guarded device.  The first call that fails ends it with that call's status and message, and the events are destroyed.
template <class Call>
int timed(const char *who, int warmup, int reps, hipStream_t s, float *ms_per_call, Call call) {
  int rc = MMH_OK;
  for (int i = 0; i < warmup && rc == MMH_OK; ++i) rc = call();
  if (rc != MMH_OK) return rc;
  hipEvent_t t0 = nullptr, t1 = nullptr;
  hipError_t e = hipEventCreate(&t0);
  if (e == hipSuccess) e = hipEventCreate(&t1);
  if (e == hipSuccess) e = hipEventRecord(t0, s);
  for (int i = 0; i < reps && rc == MMH_OK && e == hipSuccess; ++i) rc = call();
  float ms = 0.f;
  if (rc == MMH_OK && e == hipSuccess) e = hipEventRecord(t1, s);
  if (rc == MMH_OK && e == hipSuccess) e = hipEventSynchronize(t1);
  if (rc == MMH_OK && e == hipSuccess) e = hipEventElapsedTime(&ms, t0, t1);
  if (t0) (void)hipEventDestroy(t0);
  if (t1) (void)hipEventDestroy(t1);
  if (rc != MMH_OK) return rc;
  if (e != hipSuccess) return hip_fail(e, who);
  *ms_per_call = ms / reps;
  return MMH_OK;
}

}  // namespace
