// internal.hpp -- what the translation units of libmmult_hip.so share on the HOST side: the handle,
// error plumbing, workspace ownership and the launcher entry points each TU exports to the others.
//
// The library is the "thin C-ABI shim" of BASELINE.json's north star around the hand-written gfx950
// kernels of this directory.  Translation units (build.py compiles them in parallel):
//   state.hip        handle life cycle, sticky error, stream-K workspaces and phase tables, mmh_warm
//   policy.hip       sgemm_on(): MMH_KERNEL_AUTO's tile choice -- the reference's `NEW := MMult_xxx`
//                    makefile switch (cuda/makefile:1-3) made a run-time choice; call_on(): the op / ex / batched calls' one front end;
//                    the plans behind mmh_auto_plan* (plan_batched: both batched ones).  Pure host code.
//   launch_reg.hip   register-staged MFMA tiles (sgemm_mfma.hpp): plain, stream-K, split-K
//   launch_dma.hip   LDS-DMA tiles (sgemm_dma.hpp): plain, stream-K; whole and guarded shapes
//   launch_dma5.hip  LDS-DMA tiles with loader waves (K2W, sgemm_dma5.hpp): plain, chained stream-K -- the NN forms;
//   launch_op.hip    ... their transposed-operand forms, launch_ex.hip / launch_ex_t.hip their fused-epilogue forms
//                    (mmh_sgemm_ex): each TU instantiates launch_dma5.hpp's launch_dma5_tile for the kernels of its own form
//                    (NnForm / OpForm / ExForm); launch_batched.hip their strided batched form and launch_batched_ex.hip the
//                    batched form with the epilogue: launch_dma5.hpp's launch_batched_tile for a BatchedForm / BatchedExForm,
//                    and the two naive batched kernels behind its one chunk loop (built in parallel)
//   launch_valu.hip  K1 / K0 (sgemm_valu.hpp)
//   host_flavour.hip mmh_sgemm_host(_timed): the host-pointer MY_MMult, row-panel pipeline
//   shard.hip        mmh_shard_*: single-process row-panel shard over RCCL
//   igemm.hip        int8 GEMM, quantisation passes
//   relu_grad.hip    mmh_relu_grad_colsum: the linear layer's backward beside its GEMMs (ReLU gate, bias gradient)
//   vendor.hip       rocBLAS / hipBLASLt comparators, RCCL loader
//   probes.hip       peak probes
//   abi.hip          the remaining extern "C" entry points -- the GEMM calls' C parameters become a GemmArgs / BatchArgs there,
//                    once per call kind, for the call and its timing twin --; the catalogue of kernel ids; the table of handle options
// No torch, no CPU fallback: without a gfx950 device every compute entry point returns
// MMH_ERR_NO_DEVICE / MMH_ERR_HIP.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "ab_build.hpp"
#include "device_memory.hpp"   // capturing, DeviceGuard, DevBuf / GraphBuf / Retired
#include "../../include/mmult_hip.h"

namespace mmh {

// ---- error text (thread-local, state.hip) ----
void set_last_error(const std::string &s);
void set_last_launch(const std::string &s);
const std::string &last_error_ref();
const std::string &last_launch_ref();
int hip_fail(hipError_t e, const char *what);

#define HIP_TRY(expr)                                        \
  do {                                                       \
    hipError_t e_ = (expr);                                  \
    if (e_ != hipSuccess) return ::mmh::hip_fail(e_, #expr); \
  } while (0)

// A failed allocation of a handle-owned buffer (device_memory.hpp's reserve) as this library's status and text (state.hip)
int alloc_status(hipError_t e);

// Handle-owned scratch that is per handle, not per stream, and grows on demand -- the int8 / quantisation images and the partial
// rows of mmh_relu_grad_colsum -- is a GraphBuf each.  It grows through reserve_scratch (state.hip) only.
struct ScratchNeed {
  GraphBuf *buf;
  size_t bytes;            // 0: the call does not use buf
};

constexpr int kMaxHostPanels = 16;

struct GemmArgs {
  int m, n, k;
  const float *A;
  int lda;
  const float *B;
  int ldb;
  float *C;
  int ldc;
  int acc;          // 0: C = A*B, 1: C = A*B + C
  hipStream_t s;
  // "rim" launches (sgemm_dma.hpp): m x n above is the TRIMMED problem the tiles cover, rim_m x rim_n the whole
  // one -- the strips in between run on the vector ALU in extra workgroups of the same launch.  0: no rim.
  int rim_m = 0, rim_n = 0;
  // launch form: 0 = the launcher's own rule (a kernel the caller forced), 1 = one workgroup per tile, 2 = the
  // persistent stream-K launch -- what MMH_KERNEL_AUTO's cost table decided (policy.hip)
  int form = 0;
  // ... and the persistent workgroups per CU the table priced that launch on (0: whatever the kernel's residency allows)
  int sk_w = 0;
  // operand layouts (mmh_sgemm_op): 1 = stored transposed -- A as k x m (lda >= m), B as n x k (ldb >= k)
  int ta = 0, tb = 0;
  // the fused epilogue (mmh_sgemm_ex, ex = 1): C = act(alpha op(A) op(B) + beta C + bias) on the `ex` kernels (launch_ex.hip);
  // acc is 0 there -- the chain starts at +0, beta C is the epilogue's
  int ex = 0;
  float alpha = 1.0f, beta = 0.0f;
  const float *bias = nullptr;
  int bias_mode = MMH_BIAS_NONE, act = MMH_ACT_NONE;
};
// A call's operands with their stored layouts (mmh_sgemm_op: ta / tb as they came, checked by call_on) ...
inline GemmArgs op_args(int ta, int tb, int m, int n, int k, const float *dA, int lda, const float *dB, int ldb, float *dC, int ldc,
                        int accumulate, hipStream_t s) {
  GemmArgs g{m, n, k, dA, lda, dB, ldb, dC, ldc, accumulate ? 1 : 0, s};
  g.ta = ta;
  g.tb = tb;
  return g;
}
// ... and the fused epilogue of an `ex` call on them: C = act(alpha op(A) op(B) + beta C + bias); acc is 0 -- the chain starts at
// +0, beta C is the epilogue's
inline GemmArgs ex_args_of(GemmArgs g, float alpha, float beta, const float *dBias, int bias_mode, int activation) {
  g.acc = 0;
  g.ex = 1;
  g.alpha = alpha;
  g.beta = beta;
  g.bias = dBias;
  g.bias_mode = bias_mode;
  g.act = activation;
  return g;
}

}  // namespace mmh

struct mmh_context {
  int device = 0;
  int kernel = MMH_KERNEL_AUTO;
  int cu_count = 0;
  mmh::DevBuf a, b, c;     // staging for the host-pointer flavour
  mmh::GraphBuf bt;        // int8 GEMM: packed (transposed, padded) B (tools build)
  int igemm_mode = 0;      // 0 auto, see MMH_OPT_IGEMM_MODE
  int i8_grid_cap = 0;     // test hook (environment MMH_I8_GRID_CAP, read at mmh_create): K3p's persistent grid, so that small shapes walk several tiles per workgroup
  mmh::GraphBuf qa, qb, qc, qs; // quantised GEMM workspace: int8 A, int8 B, int32 C, {amax bits, scales, a zero block}
  void *qs_zeros_of = nullptr;  // the allocation of qs whose zero block has been written (igemm.hip, zero_amax)
  mmh::GraphBuf colsum_parts;   // mmh_relu_grad_colsum: the row blocks' partial column sums (ceil(rows / R) x cols floats)
  // stream-K / split-K workspaces, one set PER STREAM the handle has launched on: launches on different streams
  // never share hand-off words or partial tiles, so nothing has to order one stream behind another and the handle
  // never touches a stream again after the call that used it returns (the caller may destroy it).
  struct StreamWs {
    hipStream_t stream = nullptr;
    mmh::GraphBuf flags;   // per-tile hand-off words; every launch leaves them ZERO (the last reader of a word
                           // resets it), so only a fresh or suspect buffer is memset
    bool flags_dirty = true;
    mmh::GraphBuf parts;   // partial tiles
    unsigned long stamp = 0;
    // a captured launch points at flags / parts (marked together): they retire on growth, and the set is never evicted
    bool captured() const { return flags.captured; }
  };
  std::vector<std::unique_ptr<StreamWs>> ws;
  unsigned long ws_stamp = 0;
  int *sk_stats = nullptr;           // device: [0] stream-K hand-overs finished by the head's owner (diagnostic)
  mmh::Retired retired;              // allocations a captured graph may still point at: freed with the handle
  int streamk = 1;         // allow the persistent stream-K launch for ragged tile counts
  int splitk = 0;          // opt-in split-K: 0 off (default), 1 auto, >= 2 that many parts
  int host_panels = -1;    // host flavour: -1 auto, 0/1 the plain staged form, n pipelined row panels
  void *rocblas = nullptr; // rocblas_handle, created on first use
  void *blaslt = nullptr;  // hipBLASLt bridge state (vendor.hip)
  // the sticky error word: host memory the device can write (an opt-in split-K wait that times out adds
  // to it); every entry point looks at it before doing anything else
  int *sticky = nullptr;       // host view
  int *sticky_dev = nullptr;   // device view of the same word
  long long spin_limit = 1ll << 26;
  int fault = 0;               // MMH_OPT_FAULT_INJECT
  int pin = 1;                 // persistent launches ask for 160 KiB / w of LDS so that exactly w workgroups fit a CU
  int sk_order = 1;            // stream-K launches get the phase-ordered range / tile tables
  int sk_order_min10 = 18;     // ... from this many tiles per workgroup, in tenths (tools build: option 104)
  int dma_edge = 1;            // ragged / 4-byte-aligned shapes may run the guarded LDS-DMA tiles (MMH_OPT_DMA_EDGE)
  int dma_dword_rows = 1;      // ... including operands whose rows are only 4-byte aligned (odd lda / ldb / base)
  int sk_chain = 1;            // stream-K launches of the K2W tiles (launch_dma5.hip) run a range's parts as one stream of slices (MMH_OPT_STREAMK_CHAIN)
  int rim5 = 0;                // tools build only (MMH_OPT_RIM5): the RIM launch of the 64x64 K2W tile -- measured, it loses
  int ab_whole_ranges = 0;     // tools build only (option 106): persistent launches take WHOLE tiles (ranges rounded to tile boundaries: no hand-over)
  int ab_nodefer = 0;          // tools build only (option 102): stream-K heads publish on the spot (no deferred publish)
  int ab_valu_old = 0;         // tools build only (option 105): the K1 ids run the register-staged K1 of rounds 1-4, not K1W
  int ab_own_occ = 0;          // tools build only (option 103): a whole-tile stream-K launch is bounded by ITS OWN instantiation's residency
  int split_tail = 1;          // a plain K2W launch whose last round the dispatcher would pack two per CU goes out as two launches (launch_dma5.hip; tools build: option 107 switches it off)
  int ab_group_m = 0;          // tools build only (option 101): raster group height of the plain K2W launch, 0 = GROUP_M
  int ab_batch_major = 0;      // tools build only (option 108): the batched K2W launch in plain batch-major order, not XCD-contiguous
  int persist = 0;             // whole rounds of the persistent grid run persistent too (MMH_OPT_PERSIST)
  int rim = 0;                 // MMH_KERNEL_AUTO trims up to this many rows / columns past a 64-boundary off the tiles (MMH_OPT_RIM; off: measured, it does not pay)
  // stream-K tables per launch shape (tiles, K-slices, grid): [order: grid ints][place: tiles ints]
  struct SkTable {
    long tiles = 0;
    int nk = 0, grid = 0;
    mmh::DevBuf buf;
    int *host = nullptr;       // pinned staging the asynchronous upload reads from
    size_t host_ints = 0;
    unsigned long stamp = 0;
    bool pinned = false;       // a captured graph points at buf: never evicted
    bool uploaded = false;
    std::vector<hipStream_t> upload_streams;   // the streams in whose order an upload of these bytes already sits
    void drop_host() {
      if (host) (void)hipHostFree(host);
      host = nullptr;
      host_ints = 0;
    }
    ~SkTable() { drop_host(); }
  };
  std::vector<std::unique_ptr<SkTable>> sk_tables;
  unsigned long sk_stamp = 0;
  // resident workgroups per CU of each persistent kernel, per handle (= per device)
  std::vector<std::pair<const void *, int>> per_cu;
  bool warmed = false;
  // host flavour pipeline: copy-in / compute / copy-out streams, per-panel events
  hipStream_t hs_in = nullptr, hs_run = nullptr, hs_out = nullptr;
  hipEvent_t ev_in[mmh::kMaxHostPanels] = {}, ev_run[mmh::kMaxHostPanels] = {}, ev_b = nullptr;
  bool pipeline_ready = false;
  hipEvent_t t0 = nullptr, t1 = nullptr;   // mmh_sgemm_host_timed
};

namespace mmh {

// every compute entry point: refuse a handle whose sticky error word is set
int check_sticky(mmh_context *h);
#define ENTER(h)                                       \
  ::mmh::DeviceGuard guard_;                           \
  HIP_TRY(guard_.enter((h)->device));                  \
  if (int st_ = ::mmh::check_sticky(h); st_ != MMH_OK) return st_

int create_context(mmh_context **out, int device, bool warm = true);   // warm: unless the environment says MMH_LAZY=1
void destroy_context(mmh_context *h);
int warm_context(mmh_context *h);

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// whole tiles, 16-byte aligned operands: the unguarded instantiations
inline bool fast_shape(int BM, int BN, int KB, const GemmArgs &g) {
  return (g.m % BM == 0) && (g.n % BN == 0) && (g.k % KB == 0) && (g.lda % 4 == 0) && (g.ldb % 4 == 0) &&
         (g.ldc % 4 == 0) && aligned16(g.A) && aligned16(g.B) && aligned16(g.C);
}
// the buffer-descriptor path needs every byte offset inside a 2 GiB window
inline bool window_ok(int BM, int BN, int k, int lda, int ldb) {
  const size_t lim = (1ull << 31) - 4096;
  return ((size_t)BM * lda + k) * 4 < lim && ((size_t)k * ldb + BN) * 4 < lim;
}
// ... for the layout the operands are stored in (a tile of A^T is k rows of BM floats, one of B^T BN rows of k floats)
inline bool window_ok(int BM, int BN, const GemmArgs &g) {
  if (!g.ta && !g.tb) return window_ok(BM, BN, g.k, g.lda, g.ldb);
  const size_t lim = (1ull << 31) - 4096;
  const size_t a = g.ta ? (size_t)g.k * g.lda + BM : (size_t)BM * g.lda + g.k;
  const size_t b = g.tb ? (size_t)BN * g.ldb + g.k : (size_t)g.k * g.ldb + BN;
  return a * 4 < lim && b * 4 < lim;
}

// ta / tb: the operand layouts of mmh_sgemm_op (A stored k x m needs lda >= m, B stored n x k ldb >= k)
int check_gemm_args(int m, int n, int k, const void *A, int lda, const void *B, int ldb, const void *C, int ldc, int ta = 0,
                    int tb = 0);

// ---- the catalogue of kernel ids (abi.hip) ----
// One row per id the library accepts: the name mmh_kernel_name returns, the family whose launcher takes the id (sgemm_on,
// policy.hip) and the register-staged tile (an id of reg_tiles) that takes the shape when that launcher answers 1 = "does
// not qualify" (-1: none -- the launcher's answer is the call's).  The tools build appends tools/ab/ab_kernels.inc.
enum class Launcher { Auto, Valu, Naive, Reg, SplitK, K2L, K2W, K2M /* tools/ab/launch_dma32.hip */ };
struct KernelRow {
  int id;
  const char *name;
  Launcher launcher;
  int fallback;
};
const KernelRow *kernel_row(int kernel);   // NULL: no such id in this build
inline bool known_kernel(int kernel) { return kernel_row(kernel) != nullptr; }
inline bool is_family(int kernel, Launcher l) {
  const KernelRow *r = kernel_row(kernel);
  return r && r->launcher == l;
}

// ---- stream-K workspaces (state.hip) ----
// the stream's own hand-off words (>= tiles of them, all zero) and partial-tile slots (>= parts_bytes)
int workspace_for(mmh_context *ctx, hipStream_t s, long tiles, size_t parts_bytes, int **flags, float **parts);
int reserve_stream(mmh_context *ctx, hipStream_t s, int m, int n, int k);   // mmh_reserve_stream
void workspaces_suspect(mmh_context *ctx);   // a launch may have died half-way: every set is memset before its next use
// ---- per-handle scratch (state.hip) ----
// Everything ONE call needs of the handle's scratch, before the call launches or records anything.  On a capturing stream a
// call that would have to allocate or grow any of it is MMH_ERR_UNSUPPORTED (`who` names the entry point in the message) with
// nothing allocated, freed or marked; otherwise every buffer is at least its size when this returns MMH_OK.  From the first
// captured call that uses a buffer, growth retires the old allocation to ctx->retired instead of freeing it (GraphBuf::reserve).
int reserve_scratch(mmh_context *ctx, hipStream_t s, const char *who, std::initializer_list<ScratchNeed> needs);
bool build_sk_tables(long tiles, int nk, int grid, int *order, int *place);
int sk_tables_for(mmh_context *ctx, long tiles, int nk, int grid, hipStream_t s, const int **order, const int **place, int min10 = 0);

// ---- the kernel families (each returns MMH_OK, an error, or 1 = "this shape does not qualify") ----
int auto_plan(int m, int n, int k, int lda, int ldb, int ldc, int base_align, int cu_count, int *kernel, long *tiles,
              int *streamk_grid);   // policy.hip: mmh_auto_plan
int sgemm_on(mmh_context *ctx, int kernel, int m, int n, int k, const float *dA, int lda, const float *dB, int ldb,
             float *dC, int ldc, int accumulate, hipStream_t s);
int auto_plan_op(int ta, int tb, int m, int n, int k, int lda, int ldb, int ldc, int base_align, int cu_count, int *kernel,
                 long *tiles, int *streamk_grid, int ex = 0);   // mmh_auto_plan_op; ex: mmh_auto_plan_ex
// launch_reg.hip: `kernel` is one of the register-staged ids (MFMA, MFMA_TILES, MFMA_256, MFMA_256X256, MFMA_128X64,
// MFMA_64X64, MFMA_SIMPLE, MFMA_PIPE, the split-K ids and, in the A/B build, the ablation ids)
int launch_reg(mmh_context *ctx, int kernel, const GemmArgs &g);
int launch_reg_splitk(mmh_context *ctx, int tile /* MMH_KERNEL_MFMA or MMH_KERNEL_MFMA_128X64 */, int S, const GemmArgs &g);
int warm_reg(mmh_context *ctx, float *scratch, hipStream_t s);
// launch_dma.hip: the tiles of k2l_tiles; returns 1 when the shape does not qualify
int launch_dma(mmh_context *ctx, int kernel, const GemmArgs &g);
bool dma_shape_ok(const mmh_context *ctx, int kernel, const GemmArgs &g);
int warm_dma(mmh_context *ctx, float *scratch, hipStream_t s);
// tools/ab/launch_dma32.hip (tools build only): tile = MMH_KERNEL_MFMA32_*_DMA (tools/ab/sgemm_dma32.hpp); returns 1 when the shape does not qualify
int launch_dma32(mmh_context *ctx, int kernel, const GemmArgs &g);
bool dma32_shape_ok(const mmh_context *ctx, int kernel, const GemmArgs &g);
int warm_dma32(mmh_context *ctx, float *scratch, hipStream_t s);
// Which plain K2W launches go out as two (launch_dma5.hpp, "the tail split"): one whole round of w workgroups per CU and a
// last round of just under one tile per CU, deep enough in K -- and a first launch of a multiple of 8 workgroups (the second
// one's id offset travels / 8).  Shared with the cost table (policy.hip) and tools/policy_fit.py tail_split.
inline bool dma5_tail_split(long tiles, long w, long cus, int k) {
  const long rem = tiles - w * cus;
  return w >= 2 && k >= 512 && 100 * rem > 85 * cus && rem <= cus && (w * cus) % 8 == 0;
}

// The RIM launch of the 64x64 K2W tile (sgemm_dma5.hpp, rim_wave): m and / or n ONE element past a multiple of 64, at
// least one whole tile each way.  *r_m / *r_n: rim rows / columns (0 or 1).
inline bool dma5_rim_dims(int m, int n, int *r_m, int *r_n) {
  const int rm = m % 64, rn = n % 64;
  const int a = (rm == 1 && m > 64) ? 1 : 0, b = (rn == 1 && n > 64) ? 1 : 0;
  if (r_m) *r_m = a;
  if (r_n) *r_n = b;
  return a > 0 || b > 0;
}
// ---- the tile tables: the one place a kernel id meets its template arguments ----
// A table is a list of tile types, each with a static ID; the launchers, the warm-up and the plan code reach a tile's
// configuration through with() / each() and never spell it out again.  A new tile of a family is one row here, one row in
// the catalogue (abi.hip) and its MMH_KERNEL_* number.
template <class... Tile>
struct TileTable {
  // f(Tile{}) for the tile of `kernel`; `none` when the table has no such id
  template <class F>
  static int with(int kernel, F &&f, int none) {
    int r = none;
    (void)((kernel == Tile::ID && ((r = f(Tile{})), true)) || ...);
    return r;
  }
  // f(Tile{}) for every tile in table order, up to the first that does not return MMH_OK
  template <class F>
  static int each(F &&f) {
    int rc = MMH_OK;
    (void)(((rc = f(Tile{})) == MMH_OK) && ...);
    return rc;
  }
};

// The register-staged tiles (sgemm_mfma.hpp) that have a stream-K form and are warmed: what MMH_KERNEL_AUTO falls back to
// and what the LDS-DMA ids run a shape on that they do not take.  Wave tile WTM x WTN MFMA blocks, KB-deep K-slices.
template <int ID_, int BM_, int BN_, int WTN_, int WTM_, int KB_>
struct RegTile {
  static constexpr int ID = ID_, BM = BM_, BN = BN_, WTN = WTN_, WTM = WTM_, KB = KB_;
};
using reg_tiles = TileTable<
    //      id                       BM   BN  WTN WTM KB
    RegTile<MMH_KERNEL_MFMA,         128, 128, 4, 4, 32>,
    RegTile<MMH_KERNEL_MFMA_256X256, 256, 256, 4, 8, 32>,    // 8 waves of 128x64 (one workgroup per CU)
    RegTile<MMH_KERNEL_MFMA_128X64,  128, 64,  2, 4, 32>,    // 4 waves of 64x32
    RegTile<MMH_KERNEL_MFMA_64X64,   64,  64,  2, 2, 128>>;  // 4 waves of 32x32, 128-deep K-slices
// the tiles an m x n shape takes of a register-staged tile (0: no such tile)
inline long reg_tile_count(int kernel, int m, int n) {
  long tiles = 0;
  reg_tiles::with(kernel, [&](auto t) {
    tiles = (long)((m + t.BM - 1) / t.BM) * ((n + t.BN - 1) / t.BN);
    return 0;
  }, 0);
  return tiles;
}

// The K2L tiles (sgemm_dma.hpp): 4 waves, NBUF ring buffers of KB-deep K-slices filled by the consumers' own LDS-DMA.
template <int ID_, int BM_, int BN_, int KB_, int WTM_, int WTN_, int NBUF_>
struct K2lTile {
  static constexpr int ID = ID_, BM = BM_, BN = BN_, KB = KB_, WTM = WTM_, WTN = WTN_, NBUF = NBUF_;
};
using k2l_tiles = TileTable<
    //      id                           BM   BN  KB WTM WTN NBUF
    K2lTile<MMH_KERNEL_MFMA_64X64_DMA,   64,  64,  32, 2, 2, 3>,    // 4 waves of 32x32, 48 KiB ring: 3 workgroups per CU
    K2lTile<MMH_KERNEL_MFMA_128X64_DMA,  128, 64,  32, 4, 2, 3>,    // 4 waves of 64x32, 72 KiB ring: 2 workgroups per CU
    K2lTile<MMH_KERNEL_MFMA_128X128_DMA, 128, 128, 32, 4, 4, 3>>;   // 4 waves of 64x64, 96 KiB ring

// The K2W tiles (sgemm_dma5.hpp) of the product's kernel ids: BM BN, wave
// tile WTM x WTN MFMA blocks, NBUF ring buffers, NL loader waves, fragments D k-steps ahead, RS the fragment reads' form;
// SK: a stream-K form (the whole-round tiles run one workgroup per tile only); OPS: op and batched forms.
// (Loader counts as measured, profiles/r04_notes.md: one loader wave on a consumer's SIMD holds that consumer back -- and
// the workgroup, at every barrier; two or four spread the pieces -- 128x128 under chained stream-K at N = 2560: 127.9 /
// 144.4 / 145.2 TFLOP/s with 1 / 2 / 4 loaders, 128x64 at N = 2432: 139.5 / 139.7 / 143.5.)
template <int ID_, int BM_, int BN_, int WTM_, int WTN_, int NBUF_, int NL_, int D_, bool SK_, bool OPS_, int RS_ = 1>
struct K2wTile {
  static constexpr int ID = ID_, BM = BM_, BN = BN_, WTM = WTM_, WTN = WTN_, NBUF = NBUF_, NL = NL_, D = D_, RS = RS_;
  static constexpr bool SK = SK_, OPS = OPS_;
};
// the template arguments every kernel of sgemm_dma5.hpp starts with, for a K2wTile K (KB = 32): `kernel<MMH_K2W_ARGS(K), ...>` in
// launch_dma5.hpp's forms (the kernels are function templates over bare numbers: no alias can name them)
#define MMH_K2W_ARGS(K) K::BM, K::BN, 32, K::WTM, K::WTN, K::NBUF
using k2w_tiles = TileTable<
    //      id                            BM   BN WTM WTN NBUF NL D  SK     OPS
    K2wTile<MMH_KERNEL_MFMA_64X64_DMA5,   64,  64, 2, 2, 3, 2, 2, true,  true>,    // 32x32 consumers + two loaders, 48 KiB ring: 3 per CU
    K2wTile<MMH_KERNEL_MFMA_128X64_DMA5,  128, 64, 4, 2, 3, 4, 2, true,  true>,    // 64x32 consumers, 72 KiB ring: 2 per CU
    K2wTile<MMH_KERNEL_MFMA_128X128_DMA5, 128, 128, 4, 4, 3, 4, 2, true, true>,    // 64x64 consumers, 96 KiB ring
    K2wTile<MMH_KERNEL_MFMA_96X96_DMA5,   96,  96, 3, 3, 3, 1, 2, false, false>,   // 48x48 (column-blocked B), 72 KiB ring: 2 per CU
    K2wTile<MMH_KERNEL_MFMA_160X160_DMA5, 160, 160, 5, 5, 3, 4, 2, false, false>,  // 80x80 (column-blocked B), 120 KiB ring: 1 per CU (N = 2560: 256 of them)
    K2wTile<MMH_KERNEL_MFMA_96X64_DMA5,   96,  64, 3, 2, 3, 4, 2, false, false>>;  // 48x32, 60 KiB ring: 2 per CU (round 5; N = 1152: 110.5 against 106.6 TFLOP/s)

// launch_batched.hip: mmh_sgemm_batched's one-launch form -- `batch` matrices of g's shape, matrix i at g.A + i sA, g.B + i sB,
// g.C + i sC (elements) -- on the K2W tiles with op forms (1: the matrices do not qualify), and the naive batched kernel
// (every kernel id, k == 0 included: it zeroes C without reading A or B)
struct BatchArgs {
  long long sA = 0, sB = 0, sC = 0;
  long batch = 1;
  long long sBias = 0;   // mmh_sgemm_batched_ex: matrix i's bias at g.bias + i sBias (0: one bias for the whole batch)
};
// one launch never holds more workgroups than this; a larger batch goes out as several launches of the same kernel
constexpr long kBatchedMaxWorkgroups = MMH_BATCHED_MAX_WORKGROUPS;

// A K2W tile's form for a shape (for every matrix of a batch): 0 whole-tile (fast_shape; the bases 16-byte aligned and every
// stride a multiple of 4 floats), 1 guarded (any m, n, k; 4-byte aligned operands unless MMH_OPT_DMA_DWORD_ROWS), -1 not on
// this tile.  g.ta / g.tb: the stored layouts' descriptor window (per matrix: the descriptors are built per tile from the
// matrix's base).
inline int dma5_form(const mmh_context *ctx, int BM, int BN, const GemmArgs &g, const BatchArgs &b = BatchArgs{}) {
  if (!window_ok(BM, BN, g)) return -1;
  const bool s4 = b.batch == 1 || (b.sA % 4 == 0 && b.sB % 4 == 0 && b.sC % 4 == 0);
  if (fast_shape(BM, BN, 32, g) && s4) return 0;
  if (!ctx || !ctx->dma_edge) return -1;
  const bool rows16 = (g.lda % 4 == 0) && (g.ldb % 4 == 0) && aligned16(g.A) && aligned16(g.B) &&
                      (b.batch == 1 || (b.sA % 4 == 0 && b.sB % 4 == 0));
  if (!rows16 && !ctx->dma_dword_rows) return -1;
  return 1;
}
inline bool dma5_shape_ok(const mmh_context *ctx, int kernel, const GemmArgs &g) {
  return k2w_tiles::with(kernel, [&](auto t) { return (int)(dma5_form(ctx, t.BM, t.BN, g) >= 0); }, 0);
}
// launch_dma5.hip: tile = MMH_KERNEL_MFMA_*_DMA5 (sgemm_dma5.hpp); returns 1 when the shape does not qualify
int launch_dma5(mmh_context *ctx, int kernel, const GemmArgs &g);
int warm_dma5(mmh_context *ctx, float *scratch, hipStream_t s);
// launch_op.hip: the op forms (g.ta / g.tb) of the K2W tiles with op forms, and of MMH_KERNEL_NAIVE
int launch_dma5_op(mmh_context *ctx, int kernel, const GemmArgs &g);   // 1: the shape does not qualify
int launch_naive_op(const GemmArgs &g);
int warm_dma5_op();                                                     // LDS opt-ins only (nothing is launched)
// launch_ex.hip: the epilogue forms (g.ex, every g.ta / g.tb) of the same three tiles; the naive kernel with the epilogue
// written out (k == 0 included: A and B are not read)
int launch_dma5_ex(mmh_context *ctx, int kernel, const GemmArgs &g);   // 1: the shape does not qualify
int launch_naive_ex(const GemmArgs &g);
int warm_dma5_ex();                                                     // LDS opt-ins only
// (launch_ex_t.hip: the half of those two with A stored k x m -- launch_ex.hip's own callees)
int launch_dma5_ex_ta(mmh_context *ctx, int kernel, const GemmArgs &g);
int warm_dma5_ex_ta();
int launch_dma5_batched(mmh_context *ctx, int kernel, const GemmArgs &g, const BatchArgs &b);
int launch_naive_batched(const GemmArgs &g, const BatchArgs &b);
int warm_dma5_batched();   // LDS opt-ins only (nothing is launched)
// launch_batched_ex.hip: the same two with the fused epilogue (g.ex, b.sBias) -- mmh_sgemm_batched_ex's one-launch form and its
// naive kernel (k == 0 included: s = +0 through the epilogue, A and B are not read)
int launch_dma5_batched_ex(mmh_context *ctx, int kernel, const GemmArgs &g, const BatchArgs &b);   // 1: the matrices do not qualify
int launch_naive_batched_ex(const GemmArgs &g, const BatchArgs &b);
int warm_dma5_batched_ex();   // LDS opt-ins only
// policy.hip: the one front end of mmh_sgemm_op, _ex, _batched and _batched_ex.  g: the call's arguments as they came (op_args /
// ex_args_of: ta / tb, bias and its mode unchecked; acc 0 / 1), b: a batched call's; (Op, N, N) is sgemm_on
enum class Call { Op, Ex, Batched, BatchedEx };
int call_on(mmh_context *ctx, Call call, int kernel, GemmArgs g, const BatchArgs &b = BatchArgs{});
// ... and the plan of both batched calls: mmh_auto_plan_batched (ex = 0, MMH_BIAS_NONE, sBias = 0) and mmh_auto_plan_batched_ex (ex = 1)
int plan_batched(int ta, int tb, int m, int n, int k, int lda, int ldb, int ldc, long long sA, long long sB, long long sC,
                 long long sBias, int bias_mode, int ex, int batch, int base_align, int cu_count, int *kernel, int *form,
                 long *workgroups);
// relu_grad.hip: mmh_relu_grad_colsum behind its handle checks (argument checks included)
int relu_grad_colsum_on(mmh_context *ctx, int rows, int cols, const float *dG, int ldg, const float *dY, int ldy, float *dZ, int ldz,
                        float *dColsum, int accumulate, hipStream_t s);
// launch_valu.hip
int launch_valu(mmh_context *ctx, int kernel, const GemmArgs &g);
int warm_valu(mmh_context *ctx, float *scratch, hipStream_t s);

// ---- vendor bridges (vendor.hip) ----
int rocblas_sgemm_rowmajor(void **handle, int m, int n, int k, const float *dA, int lda, const float *dB, int ldb,
                           float *dC, int ldc, void *stream);
void rocblas_release(void *&handle);
int hipblaslt_sgemm_rowmajor(void **state, int m, int n, int k, const float *dA, int lda, const float *dB, int ldb,
                             float *dC, int ldc, void *stream);
void hipblaslt_release(void *&state);

struct RcclApi {
  void *lib = nullptr;
  int (*get_version)(int *) = nullptr;
  int (*comm_init_all)(void **, int, const int *) = nullptr;
  int (*comm_destroy)(void *) = nullptr;
  int (*comm_count)(void *, int *) = nullptr;
  int (*group_start)() = nullptr;
  int (*group_end)() = nullptr;
  int (*broadcast)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
  bool ok = false;
};
RcclApi &rccl_api();

}  // namespace mmh
