// device_memory.hpp -- what the host side of every library here shares about device memory: who owns an allocation, and the one
// rule of stream capture -- nothing is allocated while a stream is capturing, and what a captured graph points at is never
// freed under it.  Header-only and free of error texts: each library words its own refusals (internal.hpp, csrc_q8/q8_host.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <utility>
#include <vector>

namespace mmh {

inline bool capturing(hipStream_t s) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  (void)hipStreamIsCapturing(s, &cap);
  return cap != hipStreamCaptureStatusNone;
}

// Entry points run on their object's device and leave the caller's current device as they found it
// (a torch process whose current device differs from the handle's must not find it changed).
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

// Allocations a captured graph may still point at: kept until their owner goes.
struct Retired {
  std::vector<void *> ptrs;
  Retired() = default;
  Retired(const Retired &) = delete;
  Retired &operator=(const Retired &) = delete;
  ~Retired() {
    for (void *p : ptrs) (void)hipFree(p);
  }
  size_t size() const { return ptrs.size(); }
};

// An owned device allocation, move-only.  One that owns nothing makes no runtime call, in release() or when it goes: a handle
// on the stack of a machine without a device (the plan functions, policy.hip) is free.
struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(void *p_, size_t bytes_) : p(p_), bytes(bytes_) {}   // adopts a hipMalloc'ed allocation
  DevBuf(DevBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      release();
      p = std::exchange(o.p, nullptr);
      bytes = std::exchange(o.bytes, 0);
    }
    return *this;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  template <class T>
  T *as() const { return static_cast<T *>(p); }
  // At least `need` bytes when this returns hipSuccess.  A buffer that has to grow gives up what it has FIRST -- to `retire_to`,
  // else to hipFree (the lower peak) -- and owns nothing when the allocation then fails: it is as usable as a new one.
  hipError_t reserve(size_t need, Retired *retire_to = nullptr) {
    if (need <= bytes) return hipSuccess;
    if (p && retire_to) retire_to->ptrs.push_back(std::exchange(p, nullptr));
    release();
    const hipError_t e = hipMalloc(&p, need);
    if (e == hipSuccess) bytes = need;
    else p = nullptr;
    return e;
  }
};

// A buffer a captured launch may point at, and the capture rule, once.  growth(): what a call that needs `need` bytes on a
// stream that is (not) capturing has to do; reserve() does it.  Neither words a message: the callers' texts differ.
enum class Growth {
  Fits,      // large enough: a capturing call marks it, nothing else happens
  Refused,   // it would have to be allocated or grown while the stream is capturing: nothing is touched
  Freed,     // eager growth of a buffer no graph points at: hipFree, then hipMalloc
  Retired    // eager growth after a captured use: the old allocation goes to the owner's Retired, then hipMalloc
};
struct GraphBuf : DevBuf {
  bool captured = false;   // a captured launch points at p: retire on growth, never free under the graph
  Growth growth(size_t need, bool cap) const {
    if (need <= bytes) return Growth::Fits;
    if (cap) return Growth::Refused;
    return captured ? Growth::Retired : Growth::Freed;
  }
  // *e: the allocation's status where there was one.  A refusal and a failed allocation leave `captured` as it was.
  Growth reserve(size_t need, bool cap, Retired &retired, hipError_t *e) {
    const Growth g = growth(need, cap);
    *e = hipSuccess;
    if (g == Growth::Fits) captured = captured || cap;
    else if (g != Growth::Refused) *e = DevBuf::reserve(need, g == Growth::Retired ? &retired : nullptr);
    return g;
  }
};

}  // namespace mmh
