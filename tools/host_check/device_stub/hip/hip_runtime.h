// A host stand-in for the part of the HIP runtime that the product's memory code calls, for
// tools/host_check/device_memory_host_check.cpp only: csrc/device_memory.hpp and csrc/state.hip compile against it as plain C++.
// Device and pinned memory are malloc / free, the asynchronous fill and copy are memset / memcpy on the spot; every call is
// written to a log, live allocations are counted, a stream can be switched to "capturing", and the n-th allocation can fail.
#pragma once
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <set>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2 };
enum hipStreamCaptureStatus { hipStreamCaptureStatusNone = 0, hipStreamCaptureStatusActive = 1 };
enum hipMemcpyKind { hipMemcpyHostToHost = 0, hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 };
constexpr unsigned hipHostMallocDefault = 0, hipHostMallocMapped = 2;
typedef struct ihipStream_t *hipStream_t;
typedef struct ihipEvent_t *hipEvent_t;
struct hipDeviceProp_t {
  char gcnArchName[256];
  int multiProcessorCount;
};

namespace hipstub {

enum class Fn { Malloc, Free, HostMalloc, HostFree, Memset, MemsetAsync, MemcpyAsync, DeviceSynchronize, StreamSynchronize,
                GetDevice, SetDevice, DestroyEvent, DestroyStream, Other };
struct Call {
  Fn fn;
  const void *ptr;      // the allocation made, freed, filled or written
  hipStream_t stream;
  size_t bytes;
};
struct State {
  std::vector<Call> log;                 // every runtime call but the capture query, in order
  std::map<void *, size_t> live;         // device and pinned allocations that have not been freed
  std::set<hipStream_t> capturing;       // hipStreamIsCapturing answers Active for these
  long capture_queries = 0;
  int fail_malloc_in = 0;                // n > 0: the n-th hipMalloc from now fails (once)
  int fail_host_malloc_in = 0;           // ... and the n-th hipHostMalloc
  int device = 0;                        // the current device
};
inline State &state() {
  static State s;
  return s;
}
inline void note(Fn fn, const void *ptr = nullptr, hipStream_t s = nullptr, size_t bytes = 0) { state().log.push_back({fn, ptr, s, bytes}); }
inline long calls(Fn fn, size_t from = 0) {
  long n = 0;
  for (size_t i = from; i < state().log.size(); ++i) n += state().log[i].fn == fn ? 1 : 0;
  return n;
}
inline hipError_t allocate(Fn fn, void **p, size_t bytes, int *fail_in) {
  note(fn, nullptr, nullptr, bytes);
  *p = nullptr;
  if (*fail_in > 0 && --*fail_in == 0) return hipErrorOutOfMemory;
  *p = malloc(bytes ? bytes : 1);
  if (!*p) return hipErrorOutOfMemory;
  if (bytes <= (64u << 10)) memset(*p, 0xA5, bytes);   // (the large ones stay untouched pages)
  state().live[*p] = bytes;
  state().log.back().ptr = *p;
  return hipSuccess;
}
inline hipError_t deallocate(Fn fn, void *p) {
  note(fn, p);
  if (!p) return hipSuccess;
  if (!state().live.erase(p)) {
    fprintf(stderr, "hip stub: %p freed twice, or never allocated\n", p);
    abort();
  }
  free(p);
  return hipSuccess;
}
// the fill or copy must lie inside ONE live allocation of the stub's (a host source of the program's own is not checked)
inline void check_range(const void *p, size_t bytes) {
  for (const auto &a : state().live)
    if ((const char *)p >= (const char *)a.first && (const char *)p + bytes <= (const char *)a.first + a.second) return;
  fprintf(stderr, "hip stub: %zu bytes at %p are not inside a live allocation\n", bytes, p);
  abort();
}

}  // namespace hipstub

inline const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory" : "invalid value"; }
inline hipError_t hipGetLastError() { return hipSuccess; }
inline hipError_t hipMalloc(void **p, size_t bytes) { return hipstub::allocate(hipstub::Fn::Malloc, p, bytes, &hipstub::state().fail_malloc_in); }
inline hipError_t hipFree(void *p) { return hipstub::deallocate(hipstub::Fn::Free, p); }
inline hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) {
  return hipstub::allocate(hipstub::Fn::HostMalloc, p, bytes, &hipstub::state().fail_host_malloc_in);
}
inline hipError_t hipHostFree(void *p) { return hipstub::deallocate(hipstub::Fn::HostFree, p); }
inline hipError_t hipHostGetDevicePointer(void **dev, void *host, unsigned) {
  hipstub::note(hipstub::Fn::Other, host);
  *dev = host;
  return hipSuccess;
}
inline hipError_t hipMemset(void *p, int v, size_t bytes) {
  hipstub::note(hipstub::Fn::Memset, p, nullptr, bytes);
  hipstub::check_range(p, bytes);
  memset(p, v, bytes);
  return hipSuccess;
}
inline hipError_t hipMemsetAsync(void *p, int v, size_t bytes, hipStream_t s) {
  hipstub::note(hipstub::Fn::MemsetAsync, p, s, bytes);
  hipstub::check_range(p, bytes);
  memset(p, v, bytes);
  return hipSuccess;
}
inline hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t s) {
  hipstub::note(hipstub::Fn::MemcpyAsync, dst, s, bytes);
  hipstub::check_range(dst, bytes);
  hipstub::check_range(src, bytes);
  memcpy(dst, src, bytes);
  return hipSuccess;
}
inline hipError_t hipDeviceSynchronize() {
  hipstub::note(hipstub::Fn::DeviceSynchronize);
  return hipSuccess;
}
inline hipError_t hipStreamSynchronize(hipStream_t s) {
  hipstub::note(hipstub::Fn::StreamSynchronize, nullptr, s);
  return hipSuccess;
}
inline hipError_t hipStreamIsCapturing(hipStream_t s, hipStreamCaptureStatus *status) {
  ++hipstub::state().capture_queries;
  *status = hipstub::state().capturing.count(s) ? hipStreamCaptureStatusActive : hipStreamCaptureStatusNone;
  return hipSuccess;
}
inline hipError_t hipGetDevice(int *device) {
  hipstub::note(hipstub::Fn::GetDevice);
  *device = hipstub::state().device;
  return hipSuccess;
}
inline hipError_t hipSetDevice(int device) {
  hipstub::note(hipstub::Fn::SetDevice);
  hipstub::state().device = device;
  return hipSuccess;
}
inline hipError_t hipGetDeviceProperties(hipDeviceProp_t *prop, int) {
  hipstub::note(hipstub::Fn::Other);
  snprintf(prop->gcnArchName, sizeof prop->gcnArchName, "gfx950");
  prop->multiProcessorCount = 256;
  return hipSuccess;
}
inline hipError_t hipEventDestroy(hipEvent_t e) {
  hipstub::note(hipstub::Fn::DestroyEvent, e);
  return hipSuccess;
}
inline hipError_t hipStreamDestroy(hipStream_t s) {
  hipstub::note(hipstub::Fn::DestroyStream, nullptr, s);
  return hipSuccess;
}
