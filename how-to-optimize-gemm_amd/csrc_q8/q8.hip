// q8.hip -- the host side of libmmult_hip_q8.so: the extern "C" entry points of include/mmult_hip_q8.h, the weight object and
// its scratch, the row quantiser's and the weight image's launches.  The GEMM's instantiations live in qlinear_*.hip.
// Every argument is checked before the first device call; every entry point that touches the device restores the caller's.
#include <string.h>

#include <new>
#include <string>

#include "../../include/mmult_hip_q8.h"
#include "q8_host.hpp"
#include "qlinear_launch.hpp"
#include "qlinear_plan.hpp"
#include "quant_rows_s8.hpp"

using namespace mmh;

static_assert(kQrWaveCols == QR_WAVE_COLS, "qlinear_plan.hpp restates the kernels' constants");

struct mmh_q8_weight {
  int device = 0, out = 0, in = 0, pitch = 0, cus = 256;
  DevBuf q;                  // int8, in x pitch
  DevBuf scale, inv_scale;   // out floats each
  GraphBuf scratch;          // the activations' image and row scales of the call in flight: grown on demand, under the capture rule
  Retired retired;
};

namespace {

// quant_vec_ok's convention for the row quantiser's operands (q NULL: scales only)
bool rows_vec_ok(const float *x, int ldx, const int8_t *q, int ldq) {
  return mod16(x) == 0 && ldx % 4 == 0 && (!q || (mod4(q) == 0 && ldq % 4 == 0));
}

hipError_t launch_row_quant(const RowQuantArgs &a, const RowQuantPlan &p, hipStream_t s) {
  const size_t lds = row_quant_lds(p.wide, a.cols);
  if (p.wide) hipLaunchKernelGGL(quantize_rows_s8_kernel<true>, dim3(p.grid), dim3(256), lds, s, a);
  else hipLaunchKernelGGL(quantize_rows_s8_kernel<false>, dim3(p.grid), dim3(256), lds, s, a);
  return hipGetLastError();
}

// The object's scratch holds `need` bytes when this returns MMH_OK; refused, with the object as it was, where that takes an
// allocation on a capturing stream
int reserve(mmh_q8_weight *w, size_t need, hipStream_t s, const char *who) {
  hipError_t e;
  if (w->scratch.reserve(need, capturing(s), w->retired, &e) == Growth::Refused)
    return fail(MMH_ERR_UNSUPPORTED, std::string(who) + ": the weight object's scratch would have to be allocated or grown while the "
                "stream is capturing -- make one uncaptured call at the largest size, or mmh_q8_linear_reserve, first");
  if (e != hipSuccess) return fail(MMH_ERR_ALLOC, std::string("hipMalloc: ") + hipGetErrorString(e));
  return MMH_OK;
}

int linear_args(const mmh_q8_weight *w, int rows, const float *dX, int ldx, int activation, const float *dY, int ldy) {
  if (!w || rows < 0 || !act_ok(activation)) return MMH_ERR_INVALID_ARG;
  if (rows == 0) return MMH_OK;
  if ((w->in > 0 && !dX) || !dY || ldx < w->in || ldx < 1 || ldy < w->out) return MMH_ERR_INVALID_ARG;   // (in == 0: x is not read)
  return MMH_OK;
}

// mmh_q8_linear behind its argument checks, on the object's device
int linear_on(mmh_q8_weight *w, int rows, const float *dX, int ldx, const float *dBias, int activation, float *dY, int ldy, hipStream_t s) {
  const Q8Plan p = plan_qlinear(rows, w->out, w->in, ldx, ldy, mod16(dX), mod16(dY), w->cus, dBias != nullptr, activation == MMH_ACT_RELU);
  if (const int rc = reserve(w, p.scratch, s, "mmh_q8_linear"); rc != MMH_OK) return rc;
  char *base = w->scratch.as<char>();
  int8_t *xq = reinterpret_cast<int8_t *>(base);
  float *sx = reinterpret_cast<float *>(base + p.off_scale), *rx = reinterpret_cast<float *>(base + p.off_inv);
  const RowQuantArgs qa{dX, rows, w->in, ldx, xq, p.pitch_k, p.pitch_k, sx, rx, p.quant.vec ? 1 : 0};
  Q8_TRY(launch_row_quant(qa, p.quant, s));
  const QlinearArgs g{rows, w->out, w->in, xq, p.pitch_k, w->q.as<int8_t>(), w->pitch, rx, w->inv_scale.as<float>(), dBias, activation == MMH_ACT_RELU ? 1 : 0,
                      dY, ldy, p.nbm, p.nbn};
  Q8_TRY(launch_qlinear(p, g, s));
  g_launch = p.text;
  return MMH_OK;
}

}  // namespace

extern "C" {

const char *mmh_q8_last_error(void) { return g_error.c_str(); }
const char *mmh_q8_last_launch(void) { return g_launch.c_str(); }

int mmh_q8_weight_create(mmh_q8_weight_t *weight, int device, int out, int in, const float *dW, int ldw, void *stream) {
  if (!weight || device < 0 || out <= 0 || in < 0 || ldw < in || ldw < 1 || (in > 0 && !dW)) return MMH_ERR_INVALID_ARG;
  *weight = nullptr;
  int devices = 0;
  if (hipGetDeviceCount(&devices) != hipSuccess || device >= devices) return fail(MMH_ERR_NO_DEVICE, "mmh_q8_weight_create: no such device");
  if (!q8_window(out, in)) return fail(MMH_ERR_UNSUPPORTED, "mmh_q8_weight_create: the image lies beyond the GEMM's 2 GiB descriptor window");
  DeviceGuard guard;
  Q8_TRY(guard.enter(device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (capturing(s)) return fail(MMH_ERR_UNSUPPORTED, "mmh_q8_weight_create allocates: not on a capturing stream");
  mmh_q8_weight *w = new (std::nothrow) mmh_q8_weight;
  if (!w) return MMH_ERR_ALLOC;
  w->device = device, w->out = out, w->in = in, w->pitch = q8_pitch(out);
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) w->cus = cus;
  const size_t image = (size_t)in * w->pitch, floats = (size_t)w->pitch * sizeof(float);
  hipError_t e = w->q.reserve(image ? image : 16);
  if (e == hipSuccess) e = w->scale.reserve(floats);
  if (e == hipSuccess) e = w->inv_scale.reserve(floats);
  if (e != hipSuccess) {
    delete w;
    return fail(MMH_ERR_ALLOC, std::string("hipMalloc: ") + hipGetErrorString(e));
  }
  // the channel scales: the row quantiser without an image; then the image, tile by tile
  const bool vec = rows_vec_ok(dW, ldw, nullptr, 0);
  const RowQuantArgs qa{dW, out, in, ldw, nullptr, 0, 0, w->scale.as<float>(), w->inv_scale.as<float>(), vec ? 1 : 0};
  e = launch_row_quant(qa, plan_row_quant(out, in, vec), s);
  if (e == hipSuccess && in > 0) {
    const dim3 grid((unsigned)((w->pitch + PW_TILE - 1) / PW_TILE), (unsigned)((in + PW_TILE - 1) / PW_TILE));
    if (grid.y > 65535u) e = hipErrorInvalidValue;
    else {
      hipLaunchKernelGGL(prepare_weight_s8_kernel, grid, dim3(256), 0, s, dW, out, in, ldw, w->scale.as<float>(), w->q.as<int8_t>(), w->pitch, vec ? 1 : 0);
      e = hipGetLastError();
    }
  }
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(s);
    delete w;
    return hip_fail(e, "mmh_q8_weight_create");
  }
  *weight = w;
  return MMH_OK;
}

int mmh_q8_weight_destroy(mmh_q8_weight_t w) {
  if (!w) return MMH_OK;
  DeviceGuard guard;
  Q8_TRY(guard.enter(w->device));
  delete w;   // (its buffers' hipFree waits for the device: no launch still reads what goes)
  return MMH_OK;
}

int mmh_q8_weight_info(mmh_q8_weight_t w, int *out, int *in, int *pitch, const int8_t **dQ, const float **d_scale,
                       const float **d_inv_scale) {
  if (!w) return MMH_ERR_INVALID_ARG;
  if (out) *out = w->out;
  if (in) *in = w->in;
  if (pitch) *pitch = w->pitch;
  if (dQ) *dQ = w->q.as<int8_t>();
  if (d_scale) *d_scale = w->scale.as<float>();
  if (d_inv_scale) *d_inv_scale = w->inv_scale.as<float>();
  return MMH_OK;
}

int mmh_q8_quantize_rows(int device, int rows, int cols, const float *dX, int ldx, int8_t *dQ, int ldq, float *d_scale,
                         float *d_inv_scale, void *stream) {
  if (device < 0 || rows < 0 || cols < 0) return MMH_ERR_INVALID_ARG;
  if (rows == 0) return MMH_OK;
  // (cols == 0: neither x nor q has a byte to read or write -- an empty tensor's address is NULL --, the scales are 1)
  if ((cols > 0 && !dQ) || !d_scale || !d_inv_scale || (cols > 0 && !dX) || ldx < cols || ldx < 1 || ldq < cols) return MMH_ERR_INVALID_ARG;
  DeviceGuard guard;
  Q8_TRY(guard.enter(device));
  const bool vec = rows_vec_ok(dX, ldx, dQ, ldq);
  const RowQuantPlan p = plan_row_quant(rows, cols, vec);
  const int pad_to = ldq < q8_pitch(cols) ? ldq : q8_pitch(cols);
  const RowQuantArgs a{dX, rows, cols, ldx, dQ, ldq, pad_to, d_scale, d_inv_scale, vec ? 1 : 0};
  Q8_TRY(launch_row_quant(a, p, static_cast<hipStream_t>(stream)));
  char text[128];
  snprintf(text, sizeof text, "quantize_rows_s8_kernel<%s> (%s path), %u workgroups", p.wide ? "true" : "false", vec ? "vector" : "scalar", p.grid);
  g_launch = text;
  return MMH_OK;
}

int mmh_q8_linear(mmh_q8_weight_t w, int rows, const float *dX, int ldx, const float *dBias, int activation, float *dY, int ldy,
                  void *stream) {
  if (const int rc = linear_args(w, rows, dX, ldx, activation, dY, ldy); rc != MMH_OK || rows == 0) return rc;
  DeviceGuard guard;
  Q8_TRY(guard.enter(w->device));
  return linear_on(w, rows, dX, ldx, dBias, activation, dY, ldy, static_cast<hipStream_t>(stream));
}

int mmh_q8_linear_s8(mmh_q8_weight_t w, int rows, const int8_t *dXq, int ldq, const float *d_inv_scale, const float *dBias,
                     int activation, float *dY, int ldy, void *stream) {
  if (!w || rows < 0 || !act_ok(activation)) return MMH_ERR_INVALID_ARG;
  if (rows == 0) return MMH_OK;
  if ((w->in > 0 && !dXq) || !d_inv_scale || !dY || ldq < w->in || ldy < w->out) return MMH_ERR_INVALID_ARG;   // (in == 0: xq is not read)
  if (w->in > 0 && !i8_dword(ldq, mod16(dXq)))
    return fail(MMH_ERR_UNSUPPORTED, "mmh_q8_linear_s8: the tile reads the int8 rows in dwords -- ldq and dXq's address must be multiples of 4");
  if (!i8_window(ldq, w->pitch, w->in))
    return fail(MMH_ERR_UNSUPPORTED, "mmh_q8_linear_s8: the int8 rows lie beyond the GEMM's 2 GiB descriptor window");
  DeviceGuard guard;
  Q8_TRY(guard.enter(w->device));
  // the plan of the fp32 call on these rows, without its quantiser: the same tile, guard and grid, launched straight on dXq
  const Q8Plan p = plan_qlinear(rows, w->out, w->in, w->in > 0 ? w->in : 1, ldy, 0, mod16(dY), w->cus, dBias != nullptr, activation == MMH_ACT_RELU);
  const QlinearArgs g{rows, w->out, w->in, dXq, ldq, w->q.as<int8_t>(), w->pitch, d_inv_scale, w->inv_scale.as<float>(), dBias, activation == MMH_ACT_RELU ? 1 : 0,
                      dY, ldy, p.nbm, p.nbn};
  Q8_TRY(launch_qlinear(p, g, static_cast<hipStream_t>(stream)));
  const char *then = strstr(p.text, "then ");
  g_launch = then ? then + 5 : p.text;
  return MMH_OK;
}

int mmh_q8_linear_reserve(mmh_q8_weight_t w, int max_rows, void *stream) {
  if (!w || max_rows < 0) return MMH_ERR_INVALID_ARG;
  if (max_rows == 0) return MMH_OK;
  DeviceGuard guard;
  Q8_TRY(guard.enter(w->device));
  const Q8Plan p = plan_qlinear(max_rows, w->out, w->in, w->in > 0 ? w->in : 1, w->out, 0, 0, w->cus, false, false);
  return reserve(w, p.scratch, static_cast<hipStream_t>(stream), "mmh_q8_linear_reserve");
}

int mmh_q8_linear_plan(int rows, int out, int in, int ldx, int ldy, int x_mod16, int y_mod16, int has_bias, int activation, int cu_count,
                       char *text, int text_bytes, size_t *scratch_bytes) {
  if (rows <= 0 || out <= 0 || in < 0 || ldx < in || ldx < 1 || ldy < out || ((x_mod16 | y_mod16) & ~15) || !act_ok(activation) || !text ||
      text_bytes <= 0 || !scratch_bytes)
    return MMH_ERR_INVALID_ARG;
  if (!q8_window(out, in)) return MMH_ERR_UNSUPPORTED;
  const Q8Plan p = plan_qlinear(rows, out, in, ldx, ldy, x_mod16, y_mod16, cu_count > 0 ? cu_count : 256, has_bias != 0, activation == MMH_ACT_RELU);
  snprintf(text, (size_t)text_bytes, "%s", p.text);
  *scratch_bytes = p.scratch;
  return MMH_OK;
}

int mmh_time_q8_linear(mmh_q8_weight_t w, int rows, const float *dX, int ldx, const float *dBias, int activation, float *dY, int ldy,
                       int warmup, int reps, void *stream, float *ms_per_call) {
  if (reps <= 0 || warmup < 0 || !ms_per_call) return MMH_ERR_INVALID_ARG;
  if (const int rc = linear_args(w, rows, dX, ldx, activation, dY, ldy); rc != MMH_OK) return rc;
  if (rows == 0) return MMH_ERR_INVALID_ARG;   // (nothing to time)
  DeviceGuard guard;
  Q8_TRY(guard.enter(w->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  return timed("mmh_time_q8_linear", warmup, reps, s, ms_per_call, [&] { return linear_on(w, rows, dX, ldx, dBias, activation, dY, ldy, s); });
}

}  // extern "C"
