// The product's memory manager -- csrc/device_memory.hpp and, whole, csrc/state.hip: reserve_scratch, workspace_for,
// workspaces_suspect, reserve_stream, sk_tables_for, create_context / destroy_context -- compiled as host code against
// device_stub/hip/hip_runtime.h and driven through growth, refusal under capture, retirement, eviction, failed allocations and
// destruction.  The stub's own count of live allocations is the leak check; build with -fsanitize=address,undefined for the
// rest (tests/test_device_memory_host_check.py).
#include <memory>

#include "../../how-to-optimize-gemm_amd/csrc/state.hip"

// what state.hip calls in the library's other translation units
extern "C" int mmh_device_count(int *count) {
  *count = 1;
  return MMH_OK;
}
namespace mmh {
int warm_reg(mmh_context *, float *, hipStream_t) { return MMH_OK; }
int warm_dma(mmh_context *, float *, hipStream_t) { return MMH_OK; }
int warm_dma5(mmh_context *, float *, hipStream_t) { return MMH_OK; }
int warm_valu(mmh_context *, float *, hipStream_t) { return MMH_OK; }
int warm_dma5_op() { return MMH_OK; }
int warm_dma5_ex() { return MMH_OK; }
int warm_dma5_batched() { return MMH_OK; }
int warm_dma5_batched_ex() { return MMH_OK; }
void rocblas_release(void *&handle) { handle = nullptr; }
void hipblaslt_release(void *&state) { state = nullptr; }
}  // namespace mmh

namespace {

using namespace mmh;
using hipstub::Fn;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

hipstub::State &S = hipstub::state();
constexpr size_t kMinFlags = 256u << 10, kMinParts = 16u << 20;

hipStream_t stream(int i) { return reinterpret_cast<hipStream_t>((uintptr_t)0x1000 * (uintptr_t)(i + 1)); }
size_t now() { return S.log.size(); }
long since(size_t from, Fn fn) { return hipstub::calls(fn, from); }
long live() { return (long)S.live.size(); }
// the position of the first call of `fn` from `from` on (the log's size: none)
size_t first(size_t from, Fn fn) {
  for (size_t i = from; i < S.log.size(); ++i)
    if (S.log[i].fn == fn) return i;
  return S.log.size();
}
struct Capturing {   // the stream captures while this lives
  hipStream_t s;
  explicit Capturing(hipStream_t s_) : s(s_) { S.capturing.insert(s); }
  ~Capturing() { S.capturing.erase(s); }
};

mmh_context *new_context() {
  mmh_context *ctx = nullptr;
  CHECK(create_context(&ctx, 0, /*warm=*/false) == MMH_OK && ctx);
  CHECK(ctx->sticky && ctx->sk_stats && ctx->cu_count == 256);
  return ctx;
}
// Destruction: one device synchronisation, before the first free; nothing is left; every retired pointer is freed exactly once
void destroy_checked(mmh_context *ctx, long live_before_create = 0) {
  const std::vector<void *> retired = ctx->retired.ptrs;
  const size_t t = now();
  destroy_context(ctx);
  CHECK(since(t, Fn::DeviceSynchronize) == 1);
  CHECK(first(t, Fn::DeviceSynchronize) < first(t, Fn::Free) && first(t, Fn::DeviceSynchronize) < first(t, Fn::HostFree));
  CHECK(live() == live_before_create);
  for (void *p : retired) {
    long frees = 0;
    for (size_t i = t; i < S.log.size(); ++i) frees += (S.log[i].fn == Fn::Free && S.log[i].ptr == p) ? 1 : 0;
    CHECK(frees == 1);
  }
}
int workspace(mmh_context *ctx, hipStream_t s, long tiles = 10, size_t parts = 1000) {
  int *flags = nullptr;
  float *p = nullptr;
  const int rc = workspace_for(ctx, s, tiles, parts, &flags, &p);
  if (rc == MMH_OK) {
    mmh_context::StreamWs *w = nullptr;
    for (auto &e : ctx->ws)
      if (e->stream == s) w = e.get();
    CHECK(w && flags == w->flags.p && p == w->parts.p && w->flags.bytes >= tiles * sizeof(int) && w->parts.bytes >= parts);
  }
  return rc;
}
mmh_context::StreamWs *set_of(mmh_context *ctx, hipStream_t s) {
  for (auto &e : ctx->ws)
    if (e->stream == s) return e.get();
  return nullptr;
}
struct Tables {
  int rc;
  const int *order, *place;
};
Tables tables(mmh_context *ctx, long tiles, hipStream_t s, int nk = 4, int grid = 16) {
  Tables t{0, nullptr, nullptr};
  t.rc = sk_tables_for(ctx, tiles, nk, grid, s, &t.order, &t.place);
  CHECK(!t.order == !t.place && (!t.order || t.place == t.order + grid));
  return t;
}
mmh_context::SkTable *entry_of(mmh_context *ctx, long tiles) {
  for (auto &t : ctx->sk_tables)
    if (t->tiles == tiles && t->uploaded) return t.get();
  return nullptr;
}

// 1. eager growth frees the old allocation; growth after a captured use retires it
void eager_growth_frees_and_captured_growth_retires() {
  mmh_context *ctx = new_context();
  const long base = live();
  hipStream_t s = stream(0);
  CHECK(reserve_scratch(ctx, s, "t", {{&ctx->qa, 300}}) == MMH_OK && ctx->qa.p && ctx->qa.bytes == 300 && live() == base + 1);
  size_t t = now();
  CHECK(reserve_scratch(ctx, s, "t", {{&ctx->qa, 200}, {&ctx->qb, 0}}) == MMH_OK && now() == t);   // fits: nothing happens
  CHECK(reserve_scratch(ctx, s, "t", {{&ctx->qa, 700}}) == MMH_OK && ctx->qa.bytes == 700 && live() == base + 1);
  CHECK(since(t, Fn::Free) == 1 && since(t, Fn::Malloc) == 1 && first(t, Fn::Free) < first(t, Fn::Malloc));   // free first: the lower peak
  CHECK(ctx->retired.size() == 0 && !ctx->qa.captured);
  {
    Capturing cap(s);
    t = now();
    CHECK(reserve_scratch(ctx, s, "t", {{&ctx->qa, 500}}) == MMH_OK && ctx->qa.captured && now() == t);
  }
  char *old = ctx->qa.as<char>();
  memset(old, 7, 700);
  CHECK(reserve_scratch(ctx, s, "t", {{&ctx->qa, 2000}}) == MMH_OK && ctx->qa.bytes == 2000 && ctx->qa.p != old);
  CHECK(ctx->retired.size() == 1 && ctx->retired.ptrs[0] == old && live() == base + 2);
  CHECK(old[0] == 7 && old[699] == 7);   // what the graph points at is still there
  destroy_checked(ctx);
}

// 2. refusal while capturing leaves everything as it was, without a runtime call
void growth_while_capturing_is_refused() {
  mmh_context *ctx = new_context();
  hipStream_t s = stream(0);
  CHECK(reserve_scratch(ctx, s, "t", {{&ctx->qa, 300}, {&ctx->qb, 400}, {&ctx->qc, 500}}) == MMH_OK);
  void *const p[3] = {ctx->qa.p, ctx->qb.p, ctx->qc.p};
  {
    Capturing cap(s);
    const size_t t = now();
    CHECK(reserve_scratch(ctx, s, "mmh_x", {{&ctx->qa, 100}, {&ctx->qb, 400}, {&ctx->qc, 501}}) == MMH_ERR_UNSUPPORTED);
    CHECK(now() == t && last_error_ref().rfind("mmh_x: a handle-owned workspace would have to be allocated or grown", 0) == 0);
    CHECK(ctx->qa.p == p[0] && ctx->qb.p == p[1] && ctx->qc.p == p[2]);
    CHECK(ctx->qa.bytes == 300 && ctx->qb.bytes == 400 && ctx->qc.bytes == 500);
    CHECK(!ctx->qa.captured && !ctx->qb.captured && !ctx->qc.captured && ctx->retired.size() == 0);
    // a stream without a set
    CHECK(workspace(ctx, s) == MMH_ERR_UNSUPPORTED && ctx->ws.empty() && now() == t);
    CHECK(last_error_ref().rfind("a stream-K launch cannot allocate its workspaces while the stream is capturing", 0) == 0);
    CHECK(reserve_stream(ctx, s, 512, 512, 512) == MMH_ERR_UNSUPPORTED && ctx->ws.empty() && now() == t);
    CHECK(last_error_ref() == "mmh_reserve_stream must run before the capture begins (it allocates)");
  }
  CHECK(workspace(ctx, s) == MMH_OK && ctx->ws.size() == 1);
  mmh_context::StreamWs *w = set_of(ctx, s);
  CHECK(w->flags.bytes == kMinFlags && w->parts.bytes == kMinParts && !w->flags_dirty);
  void *const f = w->flags.p, *const q = w->parts.p;
  {
    Capturing cap(s);
    const size_t t = now();
    CHECK(workspace(ctx, s, (long)(kMinFlags / sizeof(int)) + 1, 1000) == MMH_ERR_UNSUPPORTED);   // too few words
    CHECK(workspace(ctx, s, 10, kMinParts + 1) == MMH_ERR_UNSUPPORTED);                            // too few slots
    workspaces_suspect(ctx);
    CHECK(w->flags_dirty && workspace(ctx, s) == MMH_ERR_UNSUPPORTED);                             // a fill outside the graph
    CHECK(now() == t && ctx->ws.size() == 1 && w->flags.p == f && w->parts.p == q && !w->captured() && w->flags_dirty);
    CHECK(w->flags.bytes == kMinFlags && w->parts.bytes == kMinParts && ctx->retired.size() == 0);
  }
  destroy_checked(ctx);
}

// 3. a capturing call that fits marks the set; a later eager growth retires both of its buffers
void a_captured_set_retires_what_it_outgrows() {
  mmh_context *ctx = new_context();
  const long base = live();
  hipStream_t s = stream(0);
  CHECK(workspace(ctx, s) == MMH_OK && live() == base + 2);
  mmh_context::StreamWs *w = set_of(ctx, s);
  void *const f = w->flags.p, *const q = w->parts.p;
  {
    Capturing cap(s);
    const size_t t = now();
    CHECK(!w->captured() && workspace(ctx, s) == MMH_OK && w->captured() && w->parts.captured && now() == t);
  }
  const size_t t = now();
  CHECK(workspace(ctx, s, (long)(kMinFlags / sizeof(int)) + 1, kMinParts + 1) == MMH_OK);
  CHECK(ctx->retired.size() == 2 && ctx->retired.ptrs[0] == f && ctx->retired.ptrs[1] == q && since(t, Fn::Free) == 0);
  CHECK(live() == base + 4 && w->flags.p != f && w->parts.p != q && w->flags.bytes == kMinFlags + 4 && w->parts.bytes == kMinParts + 1);
  CHECK(static_cast<int *>(f)[0] == 0);   // readable
  destroy_checked(ctx);
}

// 4. beyond eight evictable sets the least recently used one goes, after one synchronisation; a captured set never does
void stream_sets_are_evicted_least_recently_used_first() {
  mmh_context *ctx = new_context();
  for (int i = 0; i < 8; ++i) CHECK(workspace(ctx, stream(i)) == MMH_OK);
  CHECK(workspace(ctx, stream(0)) == MMH_OK && ctx->ws.size() == 8);   // stream 1's is now the oldest
  const long before = live();
  size_t t = now();
  CHECK(workspace(ctx, stream(8)) == MMH_OK && ctx->ws.size() == 8 && live() == before);
  CHECK(since(t, Fn::DeviceSynchronize) == 1 && since(t, Fn::Free) == 2 && since(t, Fn::Malloc) == 2 && since(t, Fn::MemsetAsync) == 1);
  CHECK(first(t, Fn::DeviceSynchronize) < first(t, Fn::Free) && first(t, Fn::Free) < first(t, Fn::Malloc));
  CHECK(!set_of(ctx, stream(1)) && set_of(ctx, stream(0)) && set_of(ctx, stream(8)) && !set_of(ctx, stream(8))->flags_dirty);
  destroy_checked(ctx);

  // a captured set is not counted and not taken, however old
  ctx = new_context();
  for (int i = 0; i < 8; ++i) CHECK(workspace(ctx, stream(i)) == MMH_OK);
  {
    Capturing cap(stream(0));
    CHECK(workspace(ctx, stream(0)) == MMH_OK);
  }
  for (int i = 1; i < 8; ++i) CHECK(workspace(ctx, stream(i)) == MMH_OK);   // stream 0's is the oldest again
  t = now();
  CHECK(workspace(ctx, stream(8)) == MMH_OK && ctx->ws.size() == 9 && since(t, Fn::DeviceSynchronize) == 0);   // seven evictable: a new set
  CHECK(workspace(ctx, stream(9)) == MMH_OK && ctx->ws.size() == 9 && since(t, Fn::DeviceSynchronize) == 1);   // eight: stream 1's goes
  CHECK(set_of(ctx, stream(0)) && set_of(ctx, stream(0))->captured() && !set_of(ctx, stream(1)) && set_of(ctx, stream(9)));
  destroy_checked(ctx);

  // eight captured sets and eight eager ones: the seventeenth stream still finds an eager one to take
  ctx = new_context();
  for (int i = 0; i < 8; ++i) {
    CHECK(workspace(ctx, stream(i)) == MMH_OK);
    Capturing cap(stream(i));
    CHECK(workspace(ctx, stream(i)) == MMH_OK);
  }
  for (int i = 8; i < 16; ++i) CHECK(workspace(ctx, stream(i)) == MMH_OK);
  CHECK(ctx->ws.size() == 16);
  t = now();
  CHECK(workspace(ctx, stream(16)) == MMH_OK && ctx->ws.size() == 16 && since(t, Fn::DeviceSynchronize) == 1);
  CHECK(!set_of(ctx, stream(8)) && set_of(ctx, stream(16)) && !set_of(ctx, stream(16))->captured());
  for (int i = 0; i < 8; ++i) CHECK(set_of(ctx, stream(i)) && set_of(ctx, stream(i))->captured());
  {
    Capturing cap(stream(17));   // ... and a capturing stream without a set evicts nobody
    t = now();
    CHECK(workspace(ctx, stream(17)) == MMH_ERR_UNSUPPORTED && now() == t && ctx->ws.size() == 16);
  }
  destroy_checked(ctx);
}

// 5. the hand-off words are zero-filled when the buffer is new, has grown or is suspect -- and not otherwise
void flags_are_filled_once() {
  mmh_context *ctx = new_context();
  hipStream_t s = stream(3);
  size_t t = now();
  CHECK(workspace(ctx, s) == MMH_OK && since(t, Fn::MemsetAsync) == 1);
  mmh_context::StreamWs *w = set_of(ctx, s);
  const hipstub::Call fill = S.log[first(t, Fn::MemsetAsync)];
  CHECK(fill.ptr == w->flags.p && fill.bytes == kMinFlags && fill.stream == s);
  for (size_t i = 0; i < kMinFlags / sizeof(int); ++i) CHECK(w->flags.as<int>()[i] == 0);
  t = now();
  CHECK(workspace(ctx, s) == MMH_OK && now() == t);   // the second call: no fill, nothing
  workspaces_suspect(ctx);
  CHECK(workspace(ctx, s) == MMH_OK && since(t, Fn::MemsetAsync) == 1 && now() == t + 1 && !w->flags_dirty);
  t = now();
  const long words = (long)(kMinFlags / sizeof(int)) + 100;
  CHECK(workspace(ctx, s, words, 1000) == MMH_OK && since(t, Fn::MemsetAsync) == 1 && since(t, Fn::Free) == 1 && since(t, Fn::Malloc) == 1);
  CHECK(S.log.back().fn == Fn::MemsetAsync && S.log.back().bytes == words * sizeof(int) && w->flags.as<int>()[words - 1] == 0);
  t = now();
  CHECK(workspace(ctx, s, words, 1000) == MMH_OK && now() == t);
  // (a capturing call on a suspect set is refused -- scenario 2 -- so no fill is ever recorded into a graph)
  // mmh_reserve_stream: the upper bounds of an m x n x k problem, eagerly, on a stream of its own
  CHECK(reserve_stream(ctx, stream(4), 0, 5, 5) == MMH_ERR_INVALID_ARG);
  CHECK(reserve_stream(ctx, stream(4), 100, 100, 100) == MMH_OK && ctx->ws.size() == 2);
  CHECK(set_of(ctx, stream(4))->flags.bytes == kMinFlags && set_of(ctx, stream(4))->parts.bytes == (size_t)256 * 2 * 128 * 128 * sizeof(float));
  destroy_checked(ctx);
}

// 6. the phase-order tables: built and uploaded once per shape and stream, pinned by a capture, evicted beyond 32
void tables_are_cached_per_shape() {
  mmh_context *ctx = new_context();
  hipStream_t s = stream(0), s2 = stream(1), s3 = stream(2);
  const long base = live();
  size_t t = now();
  long queries = S.capture_queries;
  CHECK(tables(ctx, 17, s).rc == MMH_OK && !tables(ctx, 17, s).order && now() == t && S.capture_queries == queries);   // 1.06 tiles per workgroup: identity
  Tables a = tables(ctx, 40, s);
  CHECK(a.rc == MMH_OK && a.order && live() == base + 2);
  CHECK(since(t, Fn::HostMalloc) == 1 && since(t, Fn::Malloc) == 1 && since(t, Fn::MemcpyAsync) == 1 && now() == t + 3);
  CHECK(S.log.back().stream == s && S.log.back().bytes == (16 + 40) * sizeof(int));
  std::vector<int> want(16 + 40);
  CHECK(build_sk_tables(40, 4, 16, want.data(), want.data() + 16) && memcmp(a.order, want.data(), want.size() * sizeof(int)) == 0);
  t = now();
  Tables b = tables(ctx, 40, s);
  CHECK(b.rc == MMH_OK && b.order == a.order && now() == t);                                    // again: nothing
  CHECK(tables(ctx, 40, s2).order == a.order && now() == t + 1 && S.log.back().fn == Fn::MemcpyAsync && S.log.back().stream == s2);
  CHECK(tables(ctx, 40, s2).order == a.order && tables(ctx, 40, s).order == a.order && now() == t + 1);   // each stream has had its own
  CHECK(!entry_of(ctx, 40)->pinned);
  {
    Capturing cap(s3);
    t = now();
    CHECK(tables(ctx, 40, s3).order == a.order && tables(ctx, 40, s3).order == a.order);
    CHECK(since(t, Fn::MemcpyAsync) == 2 && now() == t + 2 && entry_of(ctx, 40)->pinned);         // a graph carries its own upload
    const Tables n = tables(ctx, 41, s3);                                                          // a shape never seen: identity
    CHECK(n.rc == MMH_OK && !n.order && now() == t + 2 && ctx->sk_tables.size() == 1 && live() == base + 2);
  }
  // 32 unpinned entries beside the pinned one; the next shape takes over the least recently used unpinned one
  for (int i = 0; i < 32; ++i) CHECK(tables(ctx, 100 + i, s).order);
  CHECK(ctx->sk_tables.size() == 33 && since(t, Fn::DeviceSynchronize) == 0);
  CHECK(tables(ctx, 100, s).order);   // shape 101 is now the oldest
  t = now();
  const long before = live();
  const Tables e = tables(ctx, 200, s);
  CHECK(e.rc == MMH_OK && e.order && ctx->sk_tables.size() == 33 && live() == before && since(t, Fn::DeviceSynchronize) == 1);
  CHECK(first(t, Fn::DeviceSynchronize) < first(t, Fn::Free) && first(t, Fn::DeviceSynchronize) < first(t, Fn::HostFree));
  CHECK(since(t, Fn::Free) == 1 && since(t, Fn::HostFree) == 1);   // a larger shape: both of the entry's allocations grow
  CHECK(!entry_of(ctx, 101) && entry_of(ctx, 100) && entry_of(ctx, 200) && entry_of(ctx, 40) && entry_of(ctx, 40)->pinned);
  CHECK(entry_of(ctx, 40)->buf.p == a.order && memcmp(a.order, want.data(), want.size() * sizeof(int)) == 0);
  // an entry whose pinned staging could not be allocated holds nothing and is the first to be reused
  mmh_context::SkTable *victim = entry_of(ctx, 102);   // the oldest now
  S.fail_host_malloc_in = 1;
  const Tables f = tables(ctx, 300, s);
  CHECK(f.rc == MMH_OK && !f.order && !victim->uploaded && !victim->host && victim->host_ints == 0 && ctx->sk_tables.size() == 33);
  t = now();
  CHECK(tables(ctx, 301, s).order && entry_of(ctx, 301) == victim && since(t, Fn::DeviceSynchronize) == 0 && ctx->sk_tables.size() == 33);
  CHECK(entry_of(ctx, 103));   // nobody else was evicted for it
  destroy_checked(ctx);
}

// 7. a failed allocation leaves the buffer owning nothing, its neighbours valid, and a retry works
void a_failed_allocation_leaves_a_usable_object() {
  mmh_context *ctx = new_context();
  const long base = live();
  hipStream_t s = stream(0);
  CHECK(reserve_scratch(ctx, s, "t", {{&ctx->qa, 300}, {&ctx->qb, 300}}) == MMH_OK && live() == base + 2);
  S.fail_malloc_in = 2;
  CHECK(reserve_scratch(ctx, s, "t", {{&ctx->qa, 1000}, {&ctx->qb, 1000}}) == MMH_ERR_ALLOC);
  CHECK(last_error_ref() == "hipMalloc: out of memory");
  CHECK(ctx->qa.p && ctx->qa.bytes == 1000 && !ctx->qb.p && ctx->qb.bytes == 0 && live() == base + 1);
  memset(ctx->qa.p, 1, 1000);
  CHECK(reserve_scratch(ctx, s, "t", {{&ctx->qa, 1000}, {&ctx->qb, 1000}}) == MMH_OK && ctx->qb.p && ctx->qb.bytes == 1000 && live() == base + 2);
  // ... in the middle of a stream set: the words are there, the slots are not, the next call completes the set
  S.fail_malloc_in = 2;
  CHECK(workspace(ctx, s) == MMH_ERR_ALLOC && set_of(ctx, s)->flags.p && !set_of(ctx, s)->parts.p && live() == base + 3);
  CHECK(workspace(ctx, s) == MMH_OK && live() == base + 4);
  destroy_checked(ctx);

  // the same for a graph buffer with an owner of its own (the int8 layer's weight object): a captured use, then a growth that fails
  {
    GraphBuf buf;
    Retired retired;
    hipError_t e = hipErrorInvalidValue;
    CHECK(buf.reserve(300, false, retired, &e) == Growth::Freed && e == hipSuccess && buf.bytes == 300 && live() == 1);
    CHECK(buf.reserve(301, true, retired, &e) == Growth::Refused && e == hipSuccess && buf.bytes == 300 && !buf.captured);
    CHECK(buf.reserve(300, true, retired, &e) == Growth::Fits && e == hipSuccess && buf.captured);
    void *const old = buf.p;
    S.fail_malloc_in = 1;
    CHECK(buf.reserve(1000, false, retired, &e) == Growth::Retired && e == hipErrorOutOfMemory);
    CHECK(!buf.p && buf.bytes == 0 && retired.size() == 1 && retired.ptrs[0] == old && live() == 1);   // retired first, then the allocation failed
    CHECK(buf.reserve(1000, false, retired, &e) == Growth::Retired && e == hipSuccess && buf.bytes == 1000 && retired.size() == 1 && live() == 2);
  }
  CHECK(live() == 0);
}

// 8. a handle that has been through all of it is destroyed in order and leaves nothing
void a_busy_context_is_destroyed_in_order() {
  const long base = live();
  mmh_context *ctx = new_context();
  hipStream_t s = stream(0);
  CHECK(reserve_scratch(ctx, s, "t", {{&ctx->qa, 300}, {&ctx->qs, 64}, {&ctx->colsum_parts, 512}, {&ctx->bt, 100}}) == MMH_OK);
  CHECK(alloc_status(ctx->a.reserve(256)) == MMH_OK && alloc_status(ctx->c.reserve(256)) == MMH_OK);
  for (int i = 0; i < 10; ++i) CHECK(workspace(ctx, stream(i)) == MMH_OK);
  {
    Capturing cap(s);
    CHECK(workspace(ctx, s) == MMH_ERR_UNSUPPORTED);   // stream 0's set went to stream 8
  }
  CHECK(workspace(ctx, s) == MMH_OK);
  for (int i = 0; i < 34; ++i) CHECK(tables(ctx, 50 + i, stream(i % 3)).order);
  {
    Capturing cap(s);
    CHECK(reserve_scratch(ctx, s, "t", {{&ctx->qa, 300}, {&ctx->qs, 64}}) == MMH_OK && workspace(ctx, s) == MMH_OK);
    CHECK(tables(ctx, 83, s).order && entry_of(ctx, 83)->pinned);
  }
  CHECK(reserve_scratch(ctx, s, "t", {{&ctx->qa, 900}, {&ctx->qs, 128}}) == MMH_OK);
  CHECK(workspace(ctx, s, (long)(kMinFlags / sizeof(int)) + 1, 1000) == MMH_OK && ctx->retired.size() == 3);
  S.fail_malloc_in = 1;
  CHECK(reserve_scratch(ctx, s, "t", {{&ctx->qa, 5000}}) == MMH_ERR_ALLOC && ctx->retired.size() == 4 && !ctx->qa.p);
  S.fail_host_malloc_in = 1;
  CHECK(tables(ctx, 400, s).rc == MMH_OK);
  ctx->t0 = reinterpret_cast<hipEvent_t>((uintptr_t)0x10);   // (the stub's destroy calls only log)
  S.device = 3;   // the caller's current device is not the handle's: the guard switches, and switches back after the last free
  destroy_checked(ctx, base);
  CHECK(S.log.back().fn == Fn::SetDevice && S.device == 3 && since(0, Fn::SetDevice) == 2);
  S.device = 0;
}

// 9. what owns nothing makes no runtime call
void empty_owners_make_no_runtime_call() {
  const size_t t = now();
  const long queries = S.capture_queries;
  {
    mmh_context on_the_stack;   // as the plan functions make one, on a machine without a device
    GraphBuf buf;
    Retired retired;
    buf.release();
    CHECK(on_the_stack.retired.size() == 0 && retired.size() == 0);
  }
  CHECK(now() == t && S.capture_queries == queries);
  {
    auto from = std::make_unique<DevBuf>();
    CHECK(from->reserve(64) == hipSuccess && live() == 1);
    void *const p = from->p;
    DevBuf to(std::move(*from));
    CHECK(!from->p && from->bytes == 0 && to.p == p && to.bytes == 64);
    const size_t u = now();
    from.reset();
    CHECK(now() == u && live() == 1);   // the moved-from buffer went without a call
    DevBuf third;
    third = std::move(to);
    CHECK(!to.p && third.p == p && now() == u);
  }
  CHECK(live() == 0 && since(t, Fn::Free) == 1);
}

}  // namespace

int main() {
  void (*const scenarios[])() = {eager_growth_frees_and_captured_growth_retires,
                                 growth_while_capturing_is_refused,
                                 a_captured_set_retires_what_it_outgrows,
                                 stream_sets_are_evicted_least_recently_used_first,
                                 flags_are_filled_once,
                                 tables_are_cached_per_shape,
                                 a_failed_allocation_leaves_a_usable_object,
                                 a_busy_context_is_destroyed_in_order,
                                 empty_owners_make_no_runtime_call};
  int n = 0;
  for (auto scenario : scenarios) {
    scenario();
    CHECK(S.live.empty() && S.capturing.empty() && S.fail_malloc_in == 0 && S.fail_host_malloc_in == 0);
    ++n;
  }
  printf("device memory host check: %d scenarios passed, %zu runtime calls, 0 allocations left\n", n, S.log.size());
  return 0;
}
