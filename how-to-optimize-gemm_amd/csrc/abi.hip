// abi.hip -- the extern "C" entry points of include/mmult_hip.h that are not tied to one kernel family: library
// and handle queries, options, the device-pointer MY_MMult (mmh_sgemm), the measurement helpers -- and the catalogue
// of kernel ids (kKernels) behind mmh_kernel_name, mmh_kernel_id and kernel_row().
// Part of libmmult_hip.so (see internal.hpp).
#include <algorithm>

#include "internal.hpp"
#include "igemm_plan.hpp"
#ifdef MMH_AB_BUILD
#include "ab_kernels.hpp"   // tools/ab/: the MMH_KERNEL_* numbers of the tools build's tile families
#endif

using namespace mmh;

namespace {
// mmh_time_sgemm_*: warmup + reps calls of `call(stream)` between one event pair on the stream: ms per call (every exit
// destroys what was created: a sticky error or a failed launch inside the loop must not leak events).  `what`: the entry point.
template <typename F>
int time_calls(mmh_context *h, void *stream, int warmup, int reps, float *ms_per_call, const char *what, F call) {
  if (!h || reps <= 0 || warmup < 0 || !ms_per_call) return MMH_ERR_INVALID_ARG;
  ENTER(h);
  hipStream_t s = static_cast<hipStream_t>(stream);
  int rc = MMH_OK;
  for (int i = 0; i < warmup && rc == MMH_OK; ++i) rc = call(s);
  if (rc != MMH_OK) return rc;
  hipEvent_t t0 = nullptr, t1 = nullptr;
  hipError_t e = hipEventCreate(&t0);
  if (e == hipSuccess) e = hipEventCreate(&t1);
  if (e == hipSuccess) e = hipEventRecord(t0, s);
  for (int i = 0; i < reps && rc == MMH_OK && e == hipSuccess; ++i) rc = call(s);
  float ms = 0.f;
  if (rc == MMH_OK && e == hipSuccess) e = hipEventRecord(t1, s);
  if (rc == MMH_OK && e == hipSuccess) e = hipEventSynchronize(t1);
  if (rc == MMH_OK && e == hipSuccess) e = hipEventElapsedTime(&ms, t0, t1);
  if (t0) (void)hipEventDestroy(t0);
  if (t1) (void)hipEventDestroy(t1);
  if (rc != MMH_OK) return rc;
  if (e != hipSuccess) return hip_fail(e, what);
  *ms_per_call = ms / reps;
  return check_sticky(h);
}

// The GEMM calls' C parameters as call_on takes them (policy.hip): the one place per call kind where a parameter meets its
// GemmArgs / BatchArgs field -- pack_X takes mmh_sgemm_X's parameters between the handle and the stream, in their order, and
// mmh_sgemm_X and mmh_time_sgemm_X (accumulate = 0) both go through it.  The stream is set where the call is made.
struct PackedCall {
  Call call;
  GemmArgs g;
  BatchArgs b = {};
};
PackedCall pack_op(int transa, int transb, int m, int n, int k, const float *dA, int lda, const float *dB, int ldb, float *dC, int ldc,
                   int accumulate) {
  return {Call::Op, op_args(transa, transb, m, n, k, dA, lda, dB, ldb, dC, ldc, accumulate, nullptr)};
}
PackedCall pack_ex(int transa, int transb, int m, int n, int k, float alpha, const float *dA, int lda, const float *dB, int ldb,
                   float beta, float *dC, int ldc, const float *dBias, int bias_mode, int activation) {
  return {Call::Ex, ex_args_of(pack_op(transa, transb, m, n, k, dA, lda, dB, ldb, dC, ldc, 0).g, alpha, beta, dBias, bias_mode, activation)};
}
PackedCall pack_batched(int transa, int transb, int m, int n, int k, const float *dA, int lda, long long strideA, const float *dB,
                        int ldb, long long strideB, float *dC, int ldc, long long strideC, int batch, int accumulate) {
  return {Call::Batched, pack_op(transa, transb, m, n, k, dA, lda, dB, ldb, dC, ldc, accumulate).g, {strideA, strideB, strideC, batch}};
}
PackedCall pack_batched_ex(int transa, int transb, int m, int n, int k, float alpha, const float *dA, int lda, long long strideA,
                           const float *dB, int ldb, long long strideB, float beta, float *dC, int ldc, long long strideC,
                           const float *dBias, long long strideBias, int bias_mode, int activation, int batch) {
  return {Call::BatchedEx, pack_ex(transa, transb, m, n, k, alpha, dA, lda, dB, ldb, beta, dC, ldc, dBias, bias_mode, activation).g,
          {strideA, strideB, strideC, batch, strideBias}};
}
int run_call(mmh_context *h, PackedCall c, void *stream) {
  if (!h) return MMH_ERR_INVALID_ARG;
  ENTER(h);
  c.g.s = static_cast<hipStream_t>(stream);
  return call_on(h, c.call, h->kernel, c.g, c.b);
}
int time_call(mmh_context *h, PackedCall c, int warmup, int reps, void *stream, float *ms_per_call, const char *what) {
  return time_calls(h, stream, warmup, reps, ms_per_call, what, [&](hipStream_t s) {
    c.g.s = s;
    return call_on(h, c.call, h->kernel, c.g, c.b);
  });
}

// The catalogue (internal.hpp, KernelRow): every id this build accepts.  A new kernel id is one row here -- name, the family
// whose launcher takes it, the register-staged tile that takes the shapes the family refuses -- plus its tile's row in
// internal.hpp's tile table and its number in mmult_hip.h.
constexpr KernelRow kKernels[] = {
    {MMH_KERNEL_AUTO, "MMult_hip_auto", Launcher::Auto, -1},
    {MMH_KERNEL_VALU, "MMult_hip_valu", Launcher::Valu, -1},
    {MMH_KERNEL_VALU_128X128, "MMult_hip_valu_128x128", Launcher::Valu, -1},
    {MMH_KERNEL_VALU_64X64, "MMult_hip_valu_64x64", Launcher::Valu, -1},
    {MMH_KERNEL_VALU_128X64, "MMult_hip_valu_128x64", Launcher::Valu, -1},
    {MMH_KERNEL_MFMA, "MMult_hip_mfma", Launcher::Reg, -1},
    {MMH_KERNEL_MFMA_256, "MMult_hip_mfma256", Launcher::Reg, -1},
    {MMH_KERNEL_NAIVE, "MMult_hip_naive", Launcher::Naive, -1},
    {MMH_KERNEL_MFMA_SIMPLE, "MMult_hip_mfma_simple", Launcher::Reg, -1},
    {MMH_KERNEL_MFMA_PIPE, "MMult_hip_mfma_pipe", Launcher::Reg, -1},
    {MMH_KERNEL_MFMA_TILES, "MMult_hip_mfma_tiles", Launcher::Reg, -1},
    {MMH_KERNEL_MFMA_128X64, "MMult_hip_mfma_128x64", Launcher::Reg, -1},
    {MMH_KERNEL_MFMA_64X64, "MMult_hip_mfma_64x64", Launcher::Reg, -1},
    {MMH_KERNEL_MFMA_256X256, "MMult_hip_mfma_256x256", Launcher::Reg, -1},
    {MMH_KERNEL_MFMA_64X64_DMA, "MMult_hip_mfma_64x64_dma", Launcher::K2L, MMH_KERNEL_MFMA_64X64},
    {MMH_KERNEL_MFMA_128X64_DMA, "MMult_hip_mfma_128x64_dma", Launcher::K2L, MMH_KERNEL_MFMA_128X64},
    {MMH_KERNEL_MFMA_128X128_DMA, "MMult_hip_mfma_128x128_dma", Launcher::K2L, MMH_KERNEL_MFMA},
    {MMH_KERNEL_MFMA_64X64_DMA5, "MMult_hip_mfma_64x64_dma5", Launcher::K2W, MMH_KERNEL_MFMA_64X64},
    {MMH_KERNEL_MFMA_128X64_DMA5, "MMult_hip_mfma_128x64_dma5", Launcher::K2W, MMH_KERNEL_MFMA_128X64},
    {MMH_KERNEL_MFMA_128X128_DMA5, "MMult_hip_mfma_128x128_dma5", Launcher::K2W, MMH_KERNEL_MFMA},
    {MMH_KERNEL_MFMA_96X96_DMA5, "MMult_hip_mfma_96x96_dma5", Launcher::K2W, MMH_KERNEL_MFMA},
    {MMH_KERNEL_MFMA_96X64_DMA5, "MMult_hip_mfma_96x64_dma5", Launcher::K2W, MMH_KERNEL_MFMA},
    {MMH_KERNEL_MFMA_160X160_DMA5, "MMult_hip_mfma_160x160_dma5", Launcher::K2W, MMH_KERNEL_MFMA},
    {MMH_KERNEL_MFMA_SPLITK, "MMult_hip_mfma_splitk", Launcher::SplitK, MMH_KERNEL_MFMA},
    {MMH_KERNEL_MFMA_SPLITK_128X64, "MMult_hip_mfma_splitk_128x64", Launcher::SplitK, MMH_KERNEL_MFMA_128X64},
#ifdef MMH_AB_BUILD
#include "ab_kernels.inc"   // tools/ab/: the A/B ids and the tile families that were measured and lost
#endif
};
// id -> row (ids are small numbers: MMH_KERNEL_* and the tools build's stay below 128), so that the launch path's
// look-ups cost an index; -1: no such id.  Building it checks the catalogue: no id twice, every fall-back a
// register-staged id.
constexpr int kMaxKernelId = 127;
struct KernelIndex {
  signed char row[kMaxKernelId + 1];
  bool ok;
};
constexpr KernelIndex kernel_index() {
  KernelIndex ix{};
  ix.ok = true;
  for (signed char &r : ix.row) r = -1;
  int n = 0;
  for (const KernelRow &r : kKernels) {
    if (r.id < 0 || r.id > kMaxKernelId || ix.row[r.id] >= 0) ix.ok = false;
    else ix.row[r.id] = (signed char)n;
    ++n;
  }
  for (const KernelRow &r : kKernels)
    if (r.fallback >= 0 && (ix.row[r.fallback] < 0 || kKernels[ix.row[r.fallback]].launcher != Launcher::Reg)) ix.ok = false;
  return ix;
}
constexpr KernelIndex kKernelIndex = kernel_index();
static_assert(kKernelIndex.ok, "kKernels: an id twice or out of range, or a fall-back that is no register-staged id");

// The handle options that are ONE int of the handle, read by mmh_set_option and mmh_get_option alike: the id, the field, and
// what set accepts -- lo .. hi, stored as it came, or (squash) any value, stored as 0 / 1.  get returns the field.  The options
// that are more than that -- a counter on the device or of the handle, a value in other units, a side effect, two fields -- are the explicit
// cases of the two functions.
struct OptionRow {
  int id;
  int mmh_context::*field;
  int lo, hi;
  bool squash;
};
constexpr OptionRow kOptions[] = {
    {MMH_OPT_STREAMK, &mmh_context::streamk, 0, 2, false},
    {MMH_OPT_SPLITK, &mmh_context::splitk, 0, 16, false},
    {MMH_OPT_HOST_PANELS, &mmh_context::host_panels, -1, kMaxHostPanels, false},
    {MMH_OPT_STREAMK_ORDER, &mmh_context::sk_order, 0, 1, true},
    {MMH_OPT_STREAMK_CHAIN, &mmh_context::sk_chain, 0, 1, true},
    {MMH_OPT_PERSIST, &mmh_context::persist, 0, 1, false},
    // the rim lives in the tools build (measured: it does not pay); the product accepts "off" only
    {MMH_OPT_RIM, &mmh_context::rim, 0, kAbBuild ? 16 : 0, false},
    {MMH_OPT_RIM5, &mmh_context::rim5, 0, 0, kAbBuild},   // (tools build: the fused rim, on / off)
#ifdef MMH_AB_BUILD
    // A/B: pin the residency of persistent launches by their LDS request (default on)
    {100, &mmh_context::pin, 0, 1, true},
    // A/B: raster group height of the plain K2W launch (0 = the product's GROUP_M)
    {101, &mmh_context::ab_group_m, 0, 1024, false},
    // A/B: chained stream-K heads publish on the spot instead of on the next part's first slice
    {102, &mmh_context::ab_nodefer, 0, 1, true},
    // A/B (prepared at the end of round 4, not yet measured): whole-tile stream-K launches of the K2W tiles bounded by their own
    // instantiation's residency (77 / 117 registers: three / two workgroups per CU) instead of the guarded one's
    {103, &mmh_context::ab_own_occ, 0, 1, true},
    // A/B: phase-ordered stream-K tables from this many tiles per workgroup, in tenths (product: 18)
    {104, &mmh_context::sk_order_min10, 10, 1000, false},
    // A/B: the vector-ALU rung as it was before round 5 (register-staged K1) instead of K1W
    {105, &mmh_context::ab_valu_old, 0, 1, true},
    // A/B (round 6): persistent launches of ragged counts with WHOLE-tile ranges -- no partial tiles, no hand-over, a
    // deterministic share per CU where a plain launch's last round is placed greedily (profiles/r06_notes.md section 6)
    {106, &mmh_context::ab_whole_ranges, 0, 1, true},
    // A/B (round 6): the tail split of plain K2W launches (launch_dma5.hpp) on (product) / off
    {107, &mmh_context::split_tail, 0, 1, true},
    // A/B: the batched K2W launch in plain batch-major order instead of XCD-contiguous runs (profiles/batched_sweep.md)
    {108, &mmh_context::ab_batch_major, 0, 1, true},
#endif
};
const OptionRow *option_row(int option) {
  for (const OptionRow &r : kOptions)
    if (r.id == option) return &r;
  return nullptr;
}
}  // namespace

const KernelRow *mmh::kernel_row(int kernel) {
  if (kernel < 0 || kernel > kMaxKernelId || kKernelIndex.row[kernel] < 0) return nullptr;
  return &kKernels[kKernelIndex.row[kernel]];
}

extern "C" {

const char *mmh_strerror(int status) {
  switch (status) {
    case MMH_OK: return "success";
    case MMH_ERR_INVALID_ARG: return "invalid argument";
    case MMH_ERR_HIP: return "HIP runtime error";
    case MMH_ERR_NO_DEVICE: return "no gfx950 device";
    case MMH_ERR_UNSUPPORTED: return "unsupported in this build";
    case MMH_ERR_ALLOC: return "allocation failed";
    case MMH_ERR_COMM: return "RCCL error";
    default: return "unknown status";
  }
}

const char *mmh_last_error(void) { return last_error_ref().c_str(); }

const char *mmh_last_launch(void) { return last_launch_ref().c_str(); }

int mmh_version(void) { return 303; }

int mmh_is_ab_build(void) {
#ifdef MMH_AB_BUILD
  return 1;
#else
  return 0;
#endif
}

int mmh_device_count(int *count) {
  if (!count) return MMH_ERR_INVALID_ARG;
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *count = 0;
    (void)hipGetLastError();
    return MMH_OK;  // "no devices" is an answer, not a failure
  }
  *count = c;
  return MMH_OK;
}

int mmh_device_info(int device, char *name, int *cu_count, int *clock_mhz) {
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (name) snprintf(name, 256, "%s (%s)", prop.name, prop.gcnArchName);
  if (cu_count) *cu_count = prop.multiProcessorCount;
  if (clock_mhz) *clock_mhz = prop.clockRate / 1000;
  return MMH_OK;
}

int mmh_create(mmh_handle_t *handle, int device) {
  if (!handle) return MMH_ERR_INVALID_ARG;
  return create_context(handle, device);
}

int mmh_destroy(mmh_handle_t h) {
  destroy_context(h);
  return MMH_OK;
}

int mmh_set_kernel(mmh_handle_t h, int kernel) {
  if (!h || !known_kernel(kernel)) return MMH_ERR_INVALID_ARG;
  h->kernel = kernel;
  return MMH_OK;
}

int mmh_set_option(mmh_handle_t h, int option, int value) {
  if (!h) return MMH_ERR_INVALID_ARG;
  if (const OptionRow *r = option_row(option)) {
    if (!r->squash && (value < r->lo || value > r->hi)) return MMH_ERR_INVALID_ARG;
    h->*(r->field) = r->squash ? (value ? 1 : 0) : value;
    return MMH_OK;
  }
  switch (option) {
    case MMH_OPT_STREAMK_TIMEOUTS:   // writing 0 clears the sticky error
      if (value != 0) return MMH_ERR_INVALID_ARG;
      {
        DeviceGuard guard;
        HIP_TRY(guard.enter(h->device));
        HIP_TRY(hipDeviceSynchronize());
      }
      if (h->sticky) *reinterpret_cast<volatile int *>(h->sticky) = 0;
      workspaces_suspect(h);   // a launch that timed out may have left hand-off counters behind
      return MMH_OK;
    case MMH_OPT_IGEMM_MODE:   // the rows of kI8Modes (igemm_plan.hpp) that this build has
      if (!i8_mode_row(value)) return MMH_ERR_INVALID_ARG;
      h->igemm_mode = value;
      return MMH_OK;
    case MMH_OPT_STREAMK_SPIN_LIMIT:   // in units of 1024 polls
      if (value < 1) return MMH_ERR_INVALID_ARG;
      h->spin_limit = (long long)value << 10;
      return MMH_OK;
    case MMH_OPT_FAULT_INJECT:
      h->fault = value ? 1 : 0;
      workspaces_suspect(h);
      return MMH_OK;
    case MMH_OPT_STREAMK_DELEGATIONS:   // writing 0 resets the counter
      if (value != 0) return MMH_ERR_INVALID_ARG;
      if (h->sk_stats) {
        DeviceGuard guard;
        HIP_TRY(guard.enter(h->device));
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemset(h->sk_stats, 0, 64));
      }
      return MMH_OK;
    case MMH_OPT_DMA_EDGE:   // 0: ragged / unaligned shapes on the register-staged tiles only; 1: guarded LDS-DMA tiles
      h->dma_edge = value ? 1 : 0;     //    for rows that are 16-byte aligned; 2 (default): for any 4-byte aligned rows
      h->dma_dword_rows = value >= 2 ? 1 : 0;
      return MMH_OK;
    case MMH_OPT_RETIRED_BUFFERS:   // read-only
    case MMH_OPT_WARMED:            // read-only
    default:
      return MMH_ERR_INVALID_ARG;
  }
}

int mmh_get_option(mmh_handle_t h, int option, int *value) {
  if (!h || !value) return MMH_ERR_INVALID_ARG;
  if (const OptionRow *r = option_row(option)) {
    *value = h->*(r->field);
    return MMH_OK;
  }
  switch (option) {
    case MMH_OPT_STREAMK_TIMEOUTS: {
      // synchronises, then reads the sticky word: how many hand-off waits have timed out on this
      // handle since it was last cleared
      *value = 0;
      DeviceGuard guard;
      HIP_TRY(guard.enter(h->device));
      HIP_TRY(hipDeviceSynchronize());
      if (h->sticky) *value = *reinterpret_cast<volatile int *>(h->sticky);
      return MMH_OK;
    }
    case MMH_OPT_IGEMM_MODE: *value = h->igemm_mode; return MMH_OK;
    case MMH_OPT_STREAMK_SPIN_LIMIT: *value = (int)(h->spin_limit >> 10); return MMH_OK;
    case MMH_OPT_FAULT_INJECT: *value = h->fault; return MMH_OK;
    case MMH_OPT_STREAMK_DELEGATIONS: {
      *value = 0;
      if (!h->sk_stats) return MMH_OK;
      DeviceGuard guard;
      HIP_TRY(guard.enter(h->device));
      HIP_TRY(hipDeviceSynchronize());
      HIP_TRY(hipMemcpy(value, h->sk_stats, sizeof(int), hipMemcpyDeviceToHost));
      return MMH_OK;
    }
    case MMH_OPT_DMA_EDGE: *value = h->dma_edge ? (h->dma_dword_rows ? 2 : 1) : 0; return MMH_OK;
    case MMH_OPT_RETIRED_BUFFERS: *value = (int)h->retired.size(); return MMH_OK;   // (host state: no synchronisation)
    case MMH_OPT_WARMED: *value = h->warmed ? 1 : 0; return MMH_OK;
    default:
      return MMH_ERR_INVALID_ARG;
  }
}

int mmh_get_kernel(mmh_handle_t h, int *kernel) {
  if (!h || !kernel) return MMH_ERR_INVALID_ARG;
  *kernel = h->kernel;
  return MMH_OK;
}

const char *mmh_kernel_name(int kernel) {
  const KernelRow *r = kernel_row(kernel);
  return r ? r->name : nullptr;
}

// the inverse of mmh_kernel_name, on the short names the harness, MMULT_KERNEL and the Python API use
int mmh_kernel_id(const char *name) {
  if (!name) return -1;
  const std::string want = std::string("MMult_hip_") + name;
  for (const KernelRow &r : kKernels)
    if (want == r.name || strcmp(name, r.name) == 0) return r.id;   // (the A/B ids of the tools build carry bare names)
  return -1;
}

int mmh_reserve_stream(mmh_handle_t h, void *stream, int m, int n, int k) {
  if (!h) return MMH_ERR_INVALID_ARG;
  ENTER(h);
  return reserve_stream(h, static_cast<hipStream_t>(stream), m, n, k);
}

int mmh_warm(mmh_handle_t h) {
  if (!h) return MMH_ERR_INVALID_ARG;
  ENTER(h);
  return warm_context(h);
}

int mmh_sgemm(mmh_handle_t h, int m, int n, int k, const float *dA, int lda, const float *dB,
              int ldb, float *dC, int ldc, int accumulate, void *stream) {
  if (!h) return MMH_ERR_INVALID_ARG;
  ENTER(h);
  return sgemm_on(h, h->kernel, m, n, k, dA, lda, dB, ldb, dC, ldc, accumulate,
                  static_cast<hipStream_t>(stream));
}
int mmh_sgemm_op(mmh_handle_t h, int transa, int transb, int m, int n, int k, const float *dA, int lda, const float *dB,
                 int ldb, float *dC, int ldc, int accumulate, void *stream) {
  return run_call(h, pack_op(transa, transb, m, n, k, dA, lda, dB, ldb, dC, ldc, accumulate), stream);
}
int mmh_sgemm_ex(mmh_handle_t h, int transa, int transb, int m, int n, int k, float alpha, const float *dA, int lda,
                 const float *dB, int ldb, float beta, float *dC, int ldc, const float *dBias, int bias_mode, int activation,
                 void *stream) {
  return run_call(h, pack_ex(transa, transb, m, n, k, alpha, dA, lda, dB, ldb, beta, dC, ldc, dBias, bias_mode, activation), stream);
}
int mmh_sgemm_batched(mmh_handle_t h, int transa, int transb, int m, int n, int k, const float *dA, int lda, long long strideA,
                      const float *dB, int ldb, long long strideB, float *dC, int ldc, long long strideC, int batch, int accumulate,
                      void *stream) {
  return run_call(h, pack_batched(transa, transb, m, n, k, dA, lda, strideA, dB, ldb, strideB, dC, ldc, strideC, batch, accumulate),
                  stream);
}
int mmh_sgemm_batched_ex(mmh_handle_t h, int transa, int transb, int m, int n, int k, float alpha, const float *dA, int lda,
                         long long strideA, const float *dB, int ldb, long long strideB, float beta, float *dC, int ldc,
                         long long strideC, const float *dBias, long long strideBias, int bias_mode, int activation, int batch,
                         void *stream) {
  return run_call(h, pack_batched_ex(transa, transb, m, n, k, alpha, dA, lda, strideA, dB, ldb, strideB, beta, dC, ldc, strideC, dBias,
                                     strideBias, bias_mode, activation, batch), stream);
}
int mmh_time_sgemm(mmh_handle_t h, int m, int n, int k, const float *dA, int lda, const float *dB,
                   int ldb, float *dC, int ldc, int warmup, int reps, void *stream,
                   float *ms_per_call) {
  return mmh_time_sgemm_op(h, MMH_OP_N, MMH_OP_N, m, n, k, dA, lda, dB, ldb, dC, ldc, warmup, reps, stream, ms_per_call);
}
int mmh_time_sgemm_op(mmh_handle_t h, int transa, int transb, int m, int n, int k, const float *dA, int lda, const float *dB,
                      int ldb, float *dC, int ldc, int warmup, int reps, void *stream, float *ms_per_call) {
  return time_call(h, pack_op(transa, transb, m, n, k, dA, lda, dB, ldb, dC, ldc, 0), warmup, reps, stream, ms_per_call,
                   "mmh_time_sgemm_op");
}
int mmh_time_sgemm_ex(mmh_handle_t h, int transa, int transb, int m, int n, int k, float alpha, const float *dA, int lda,
                      const float *dB, int ldb, float beta, float *dC, int ldc, const float *dBias, int bias_mode, int activation,
                      int warmup, int reps, void *stream, float *ms_per_call) {
  return time_call(h, pack_ex(transa, transb, m, n, k, alpha, dA, lda, dB, ldb, beta, dC, ldc, dBias, bias_mode, activation), warmup,
                   reps, stream, ms_per_call, "mmh_time_sgemm_ex");
}
int mmh_time_relu_grad_colsum(mmh_handle_t h, int rows, int cols, const float *dG, int ldg, const float *dY, int ldy, float *dZ, int ldz,
                              float *dColsum, int accumulate, int warmup, int reps, void *stream, float *ms_per_call) {
  return time_calls(h, stream, warmup, reps, ms_per_call, "mmh_time_relu_grad_colsum", [&](hipStream_t s) {
    return relu_grad_colsum_on(h, rows, cols, dG, ldg, dY, ldy, dZ, ldz, dColsum, accumulate, s);
  });
}
int mmh_time_sgemm_batched(mmh_handle_t h, int transa, int transb, int m, int n, int k, const float *dA, int lda,
                           long long strideA, const float *dB, int ldb, long long strideB, float *dC, int ldc, long long strideC,
                           int batch, int warmup, int reps, void *stream, float *ms_per_call) {
  return time_call(h, pack_batched(transa, transb, m, n, k, dA, lda, strideA, dB, ldb, strideB, dC, ldc, strideC, batch, 0), warmup,
                   reps, stream, ms_per_call, "mmh_time_sgemm_batched");
}
int mmh_time_sgemm_batched_ex(mmh_handle_t h, int transa, int transb, int m, int n, int k, float alpha, const float *dA, int lda,
                              long long strideA, const float *dB, int ldb, long long strideB, float beta, float *dC, int ldc,
                              long long strideC, const float *dBias, long long strideBias, int bias_mode, int activation,
                              int batch, int warmup, int reps, void *stream, float *ms_per_call) {
  return time_call(h, pack_batched_ex(transa, transb, m, n, k, alpha, dA, lda, strideA, dB, ldb, strideB, beta, dC, ldc, strideC,
                                      dBias, strideBias, bias_mode, activation, batch), warmup, reps, stream, ms_per_call,
                   "mmh_time_sgemm_batched_ex");
}

// per-launch durations of `count` back-to-back calls (one event pair each): the clock-ramp trace
int mmh_trace_sgemm(mmh_handle_t h, int m, int n, int k, const float *dA, int lda, const float *dB, int ldb,
                    float *dC, int ldc, int count, void *stream, float *ms_each) {
  if (!h || count <= 0 || count > 4096 || !ms_each) return MMH_ERR_INVALID_ARG;
  ENTER(h);
  hipStream_t s = static_cast<hipStream_t>(stream);
  std::vector<hipEvent_t> ev(count + 1, nullptr);
  int rc = MMH_OK;
  hipError_t e = hipSuccess;
  for (auto &x : ev)
    if (e == hipSuccess) e = hipEventCreate(&x);
  if (e == hipSuccess) e = hipEventRecord(ev[0], s);
  for (int i = 0; i < count && rc == MMH_OK && e == hipSuccess; ++i) {
    rc = sgemm_on(h, h->kernel, m, n, k, dA, lda, dB, ldb, dC, ldc, 0, s);
    if (rc == MMH_OK) e = hipEventRecord(ev[i + 1], s);
  }
  if (rc == MMH_OK && e == hipSuccess) e = hipEventSynchronize(ev[count]);
  for (int i = 0; i < count && rc == MMH_OK && e == hipSuccess; ++i) e = hipEventElapsedTime(&ms_each[i], ev[i], ev[i + 1]);
  for (auto &x : ev)   // every event that was created, whatever failed in between
    if (x) (void)hipEventDestroy(x);
  if (rc == MMH_OK && e != hipSuccess) rc = hip_fail(e, "mmh_trace_sgemm");
  return rc;
}

int mmh_streamk_plan(long tiles, int nk, int grid, int *order, int *place) {
  if (!order || !place) return MMH_ERR_INVALID_ARG;
  return build_sk_tables(tiles, nk, grid, order, place) ? MMH_OK : MMH_ERR_INVALID_ARG;
}

int mmh_auto_plan(int m, int n, int k, int lda, int ldb, int ldc, int base_align, int cu_count, int *kernel, long *tiles,
                  int *streamk_grid) {
  return mmh::auto_plan(m, n, k, lda, ldb, ldc, base_align, cu_count, kernel, tiles, streamk_grid);
}

int mmh_kernel_has_op_forms(int kernel) {
  if (!known_kernel(kernel)) return MMH_ERR_INVALID_ARG;
  return kernel == MMH_KERNEL_AUTO || kernel == MMH_KERNEL_NAIVE || k2w_tiles::with(kernel, [](auto t) { return (int)t.OPS; }, 0);
}
int mmh_auto_plan_op(int transa, int transb, int m, int n, int k, int lda, int ldb, int ldc, int base_align, int cu_count,
                     int *kernel, long *tiles, int *streamk_grid) {
  return mmh::auto_plan_op(transa, transb, m, n, k, lda, ldb, ldc, base_align, cu_count, kernel, tiles, streamk_grid);
}
int mmh_auto_plan_ex(int transa, int transb, int m, int n, int k, int lda, int ldb, int ldc, int base_align, int cu_count,
                     int *kernel, long *tiles, int *streamk_grid) {
  return mmh::auto_plan_op(transa, transb, m, n, k, lda, ldb, ldc, base_align, cu_count, kernel, tiles, streamk_grid, 1);
}
int mmh_auto_plan_batched(int transa, int transb, int m, int n, int k, int lda, int ldb, int ldc, long long strideA,
                          long long strideB, long long strideC, int batch, int base_align, int cu_count, int *kernel,
                          int *form, long *workgroups) {
  return plan_batched(transa, transb, m, n, k, lda, ldb, ldc, strideA, strideB, strideC, 0, MMH_BIAS_NONE, 0, batch, base_align,
                      cu_count, kernel, form, workgroups);
}
int mmh_auto_plan_batched_ex(int transa, int transb, int m, int n, int k, int lda, int ldb, int ldc, long long strideA,
                             long long strideB, long long strideC, long long strideBias, int bias_mode, int batch, int base_align,
                             int cu_count, int *kernel, int *form, long *workgroups) {
  return plan_batched(transa, transb, m, n, k, lda, ldb, ldc, strideA, strideB, strideC, strideBias, bias_mode, 1, batch, base_align,
                      cu_count, kernel, form, workgroups);
}

}  // extern "C"
