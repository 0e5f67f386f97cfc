// igemm.hip -- BASELINE.json config 5 and the callers either side of it: mmh_igemm_s8 (int8 x int8 -> int32 on
// v_mfma_i32_16x16x64_i8), mmh_quantize_sym_s8 and mmh_qgemm_f32 (symmetric per-tensor quantisation, dequantisation
// fused into the GEMM's epilogue).  The reference project holds no int8 code (its README.md:71-85 is prose): every
// instantiation is pinned to an exact integer reference by tests/test_gpu_int8_parity.py, and the handle-owned scratch under
// graph capture and growth by tests/test_gpu_int8_graph.py.
// The scratch (qa / qb / qc / qs, bt in the tools build) grows through reserve_scratch only: each entry point states ALL it needs
// before its first memset or launch, so a call on a capturing stream that would have to allocate is refused with nothing done.
// Part of libmmult_hip.so (see internal.hpp).
#include <algorithm>

#include "internal.hpp"
#include "igemm_plan.hpp"
#include "igemm_s8.hpp"
#include "igemm_s8_pp.hpp"
#ifdef MMH_AB_BUILD
#include "igemm_s8_k3.hpp"   // tools/ab/: K3 and the packed-B kernel K3d (modes 1, 3, 4, 10..13)
#endif
#include "quant_s8.hpp"

using namespace mmh;

static_assert(kI8AmaxWords == AMAX_WORDS && kI8Xcds == NXCD && kI8SimpleK == IBK && kI8Igemm == MMH_I8_IGEMM && kI8Qgemm == MMH_I8_QGEMM,
              "igemm_plan.hpp restates the kernels' and the header's constants");

// what the plans are made with: a base address modulo 16, the handle's CU count
static int base16(const void *p) { return (int)(reinterpret_cast<uintptr_t>(p) & 15); }
static int cus_of(const mmh_context *h) { return h->cu_count > 0 ? h->cu_count : 256; }

// mmh_last_launch of the quantiser passes: which path a tensor took (quant_vec_ok: 16-byte rows, float4 loads; else the row loop)
static const char *quant_path(bool vec) { return vec ? "vector" : "row"; }

// Zero a call's abs-max words on its stream.  A COPY of the zero block, not a memset: a captured hipMemsetAsync node was seen
// (ROCm 7.0, MI355X) to fill with a stale 8-byte pattern from the second replay of its graph on -- the first replay is right --
// which left words above every real maximum (tests/test_gpu_int8_graph.py replays every form three times on new data).  The
// zero block is written once per allocation, which reserve_scratch never makes on a capturing stream.
static int zero_amax(mmh_context *h, unsigned *amax, hipStream_t s) {
  unsigned *zeros = static_cast<unsigned *>(h->qs.p) + kQsWords;
  if (h->qs_zeros_of != h->qs.p) {
    HIP_TRY(hipMemsetAsync(zeros, 0, kAmaxBytes, s));
    HIP_TRY(hipStreamSynchronize(s));   // (once per handle: later calls may come on any stream)
    h->qs_zeros_of = h->qs.p;
  }
  HIP_TRY(hipMemcpyAsync(amax, zeros, kAmaxBytes, hipMemcpyDeviceToDevice, s));
  return MMH_OK;
}

// f(std::true_type{}) or f(std::false_type{}): a flag of the plan as a template argument
template <typename F>
static hipError_t with_flag(bool flag, F f) {
  return flag ? f(std::true_type{}) : f(std::false_type{});
}

// The plan's GEMM: its instantiation -> the kernel symbol, on the plan's grid.  A, B: the operands or their images, as the
// plan says; `bt`: the packed-B workspace (tools build, K3d).
static hipError_t launch_i8(const I8Plan &p, const int8_t *A, const int8_t *B, int32_t *C, int acc, const float *deq, int8_t *bt,
                            hipStream_t s) {
#ifdef MMH_AB_BUILD
  if (p.family == I8Family::K3 || p.family == I8Family::K3d) return launch_igemm_s8_ab(p, A, B, C, acc, bt, s);
#endif
  (void)bt;
  auto go = [&](auto kern, unsigned threads, size_t lds, auto... args) -> hipError_t {
    if (lds > 64 * 1024)   // > 64 KiB of dynamic LDS must be opted into (remembered per device)
      if (const hipError_t e = opt_in_big_lds(reinterpret_cast<const void *>(kern), lds); e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)p.grid), dim3(threads), lds, s, p.m, p.n, p.k, A, p.lda, B, p.ldb, args...);
    return hipGetLastError();
  };
  constexpr size_t kPpLds = 4 * 256 * IK + 8 * 4096;   // K3p: the ring and the eight waves' C transposers, 160 KiB
  return with_flag(p.edge, [&](auto edge) -> hipError_t {
    constexpr bool E = decltype(edge)::value;
    if (p.family == I8Family::Simple) return go(igemm_s8_simple_kernel<E>, 256, 0, C, p.ldc, acc, p.nbm, p.nbn);
    if (p.family == I8Family::K3t)   // (B in place: the kernel's Bt / kp / n_pad are B, ldb, n)
      return p.tile == 256 ? go(igemm_s8_dma_kernel<256, 256, 8, E, 0, true>, 512, 4 * 256 * IK, p.n, C, p.ldc, acc, p.nbm, p.nbn, deq)
                           : go(igemm_s8_dma_kernel<128, 128, 4, E, 0, true>, 256, 4 * 128 * IK, p.n, C, p.ldc, acc, p.nbm, p.nbn, deq);
    if (p.mfma_k == 32) return go(igemm_s8_pp_kernel<E, false, 32>, 512, kPpLds, C, p.ldc, acc, p.nbm, p.nbn, deq);
    return with_flag(p.deq, [&](auto d) -> hipError_t {
      return go(igemm_s8_pp_kernel<E, decltype(d)::value, 64>, 512, kPpLds, C, p.ldc, acc, p.nbm, p.nbn, deq);
    });
  });
}

extern "C" {

#ifdef MMH_DMA_TIMELINE
// timeline build only: where K3p's waves 0 and 4 write their per-tile stamps (2 x 16 x 8 uint64 per workgroup; NULL = off)
int mmh_ab_set_stamps_i8(mmh_handle_t h, void *stamps) {
  if (!h) return MMH_ERR_INVALID_ARG;
  ENTER(h);
  HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_i8_stamps), &stamps, sizeof(void *)));
  return MMH_OK;
}
#endif

int mmh_igemm_plan(int entry, int mode, int m, int n, int k, int lda, int ldb, int ldc, int a_mod16, int b_mod16, int c_mod16,
                   int cu_count, int grid_cap, char *text, int text_bytes, size_t *scratch_bytes) {
  if ((entry != MMH_I8_IGEMM && entry != MMH_I8_QGEMM) || !i8_mode_row(mode) || m <= 0 || n <= 0 || k <= 0 || lda < k || ldb < n ||
      ldc < n || ((a_mod16 | b_mod16 | c_mod16) & ~15) || grid_cap < 0 || !text || text_bytes <= 0 || !scratch_bytes)
    return MMH_ERR_INVALID_ARG;
  const I8Plan p = plan_igemm_s8(entry, mode, m, n, k, lda, ldb, ldc, a_mod16, b_mod16, c_mod16, cu_count > 0 ? cu_count : 256, grid_cap);
  snprintf(text, (size_t)text_bytes, "%s", p.text);
  const size_t sizes[5] = {p.qa, p.qb, p.qc, p.qs, p.bt};
  std::copy(sizes, sizes + 5, scratch_bytes);
  return MMH_OK;
}

int mmh_igemm_s8(mmh_handle_t h, int m, int n, int k, const int8_t *dA, int lda, const int8_t *dB,
                 int ldb, int32_t *dC, int ldc, int accumulate, void *stream) {
  if (!h) return MMH_ERR_INVALID_ARG;
  int rc = check_gemm_args(m, n, k, dA, lda, dB, ldb, dC, ldc);
  if (rc != MMH_OK) return rc;
  if (m == 0 || n == 0) return MMH_OK;
  ENTER(h);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (k == 0) {
    if (!accumulate)
      HIP_TRY(hipMemset2DAsync(dC, (size_t)ldc * 4, 0, (size_t)n * 4, (size_t)m, s));
    return MMH_OK;
  }
  const I8Plan p = plan_igemm_s8(kI8Igemm, h->igemm_mode, m, n, k, lda, ldb, ldc, base16(dA), base16(dB), base16(dC), cus_of(h),
                                 h->i8_grid_cap);
  if ((rc = reserve_scratch(h, s, "mmh_igemm_s8", {{&h->qa, p.qa}, {&h->qb, p.qb}, {&h->bt, p.bt}})) != MMH_OK) return rc;
  if (p.copy_a) HIP_TRY(hipMemcpy2DAsync(h->qa.p, (size_t)p.pitch_a, dA, (size_t)lda, (size_t)k, (size_t)m, hipMemcpyDeviceToDevice, s));
  if (p.copy_b) HIP_TRY(hipMemcpy2DAsync(h->qb.p, (size_t)p.pitch_b, dB, (size_t)ldb, (size_t)n, (size_t)k, hipMemcpyDeviceToDevice, s));
  HIP_TRY(launch_i8(p, p.copy_a && p.images ? static_cast<const int8_t *>(h->qa.p) : dA,
                    p.copy_b && p.images ? static_cast<const int8_t *>(h->qb.p) : dB, dC, accumulate ? 1 : 0, nullptr,
                    static_cast<int8_t *>(h->bt.p), s));
  if (p.text[0]) set_last_launch(p.text);   // (none: the tools build's K3 / K3d)
  return MMH_OK;
}

int mmh_quantize_sym_s8(mmh_handle_t h, int rows, int cols, const float *dX, int ldx, int8_t *dQ,
                        int ldq, float *d_scale, void *stream) {
  if (!h || rows < 0 || cols < 0) return MMH_ERR_INVALID_ARG;
  if (rows == 0 || cols == 0) return MMH_OK;
  if (!dX || !dQ || !d_scale || ldx < cols || ldq < cols) return MMH_ERR_INVALID_ARG;
  ENTER(h);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = reserve_scratch(h, s, "mmh_quantize_sym_s8", {{&h->qs, kQsBytes}}); rc != MMH_OK) return rc;
  unsigned *amax = static_cast<unsigned *>(h->qs.p) + 2 * AMAX_WORDS + 16;
  if (int rc = zero_amax(h, amax, s); rc != MMH_OK) return rc;
  const QuantTensor t{dX, rows, cols, ldx, dQ, ldq}, none{nullptr, 0, 0, 0, nullptr, 0};
  const bool v_in = quant_vec_ok(t, false), v_out = quant_vec_ok(t, true);
  hipLaunchKernelGGL(absmax_kernel, dim3(quant_grid(t, v_in), 1), dim3(256), 0, s, t, none, v_in ? 1 : 0, 0, amax);
  hipLaunchKernelGGL(quantize_kernel, dim3(quant_grid(t, v_out), 1), dim3(256), 0, s, t, none, v_out ? 1 : 0, 0,
                     amax, d_scale);
  HIP_TRY(hipGetLastError());
  char buf[128];
  snprintf(buf, sizeof buf, "absmax_kernel (%s path), quantize_kernel (%s path), %u + %u workgroups", quant_path(v_in),
           quant_path(v_out), quant_grid(t, v_in), quant_grid(t, v_out));
  set_last_launch(buf);
  return MMH_OK;
}

int mmh_qgemm_f32(mmh_handle_t h, int m, int n, int k, const float *dA, int lda, const float *dB,
                  int ldb, float *dC, int ldc, void *stream) {
  if (!h) return MMH_ERR_INVALID_ARG;
  int rc = check_gemm_args(m, n, k, dA, lda, dB, ldb, dC, ldc);
  if (rc != MMH_OK) return rc;
  if (m == 0 || n == 0) return MMH_OK;
  ENTER(h);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (k == 0) {
    HIP_TRY(hipMemset2DAsync(dC, (size_t)ldc * 4, 0, (size_t)n * 4, (size_t)m, s));
    return MMH_OK;
  }
  // the plan's lda / ldb are those of the int8 images; two-pass: its ldc is the int32 image's
  const I8Plan p = plan_igemm_s8(kI8Qgemm, h->igemm_mode, m, n, k, lda, ldb, ldc, base16(dA), base16(dB), base16(dC), cus_of(h),
                                 h->i8_grid_cap);
  rc = reserve_scratch(h, s, "mmh_qgemm_f32", {{&h->qa, p.qa}, {&h->qb, p.qb}, {&h->qs, p.qs}, {&h->qc, p.qc}, {&h->bt, p.bt}});
  if (rc != MMH_OK) return rc;
  int8_t *qa = static_cast<int8_t *>(h->qa.p), *qb = static_cast<int8_t *>(h->qb.p);
  unsigned *amax = static_cast<unsigned *>(h->qs.p);                           // A's words, then B's
  float *scales = reinterpret_cast<float *>(amax + 2 * AMAX_WORDS);       // [0] A, [1] B
  if ((rc = zero_amax(h, amax, s)) != MMH_OK) return rc;
  // A and B share one abs-max launch and one quantisation launch (blockIdx.y picks the tensor)
  const QuantTensor ta{dA, m, k, lda, qa, p.lda}, tb{dB, k, n, ldb, qb, p.ldb};
  const dim3 g(std::max(quant_grid(ta, p.vec_a), quant_grid(tb, p.vec_b)), 2);
  hipLaunchKernelGGL(absmax_kernel, g, dim3(256), 0, s, ta, tb, p.vec_a ? 1 : 0, p.vec_b ? 1 : 0, amax);
  hipLaunchKernelGGL(quantize_kernel, g, dim3(256), 0, s, ta, tb, p.vec_a ? 1 : 0, p.vec_b ? 1 : 0, amax, scales);
  if (p.fused) {   // the int8 GEMM dequantises in its epilogue: no int32 image of C at all
    HIP_TRY(launch_i8(p, qa, qb, reinterpret_cast<int32_t *>(dC), 0, scales, nullptr, s));
  } else {         // int32 C, then the dequantisation pass
    int32_t *qc = static_cast<int32_t *>(h->qc.p);
    HIP_TRY(launch_i8(p, qa, qb, qc, 0, nullptr, static_cast<int8_t *>(h->bt.p), s));
    hipLaunchKernelGGL(dequantize_kernel, dim3(quant_rows_grid(m, 0)), dim3(256), 0, s, qc, m, n, p.ldc, scales, scales + 1, dC, ldc);
    HIP_TRY(hipGetLastError());
  }
  set_last_launch(p.text);
  return MMH_OK;
}

}  // extern "C"
