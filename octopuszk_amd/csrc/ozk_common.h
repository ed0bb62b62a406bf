// Host-side plumbing shared by the C-ABI translation units: thread-local error string,
// HIP error checks, device selection by taskID, a small bump allocator over a caller- or
// library-owned workspace.
#pragma once
#include <hip/hip_runtime.h>

#include <pthread.h>
#include <stdlib.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/ozk.h"
#include "knobs.h"   // the tuning switches: knob(), knob_or(), env_reload()

namespace ozk {

inline char* err_buf() {
  static thread_local char buf[512] = {0};
  return buf;
}
inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err_buf(), 512, fmt, ap);
  va_end(ap);
  return code;
}

#define OZK_HIP(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return ::ozk::fail(e_ == hipErrorOutOfMemory ? OZK_E_NOMEM : OZK_E_NO_DEVICE,         \
                         "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,   \
                         __LINE__);                                                         \
  } while (0)

// argument checks shared by the entry points: the pair count of an MSM (a 24-bit index in the packed sort words),
// and the 4-byte alignment of a buffer the kernels read as words
inline int check_batch_size(int n) {
  if (n <= 0 || n > (1 << 24)) return fail(OZK_E_INVALID, "batch_size %d out of range [1, 2^24]", n);
  return OZK_OK;
}
inline bool misaligned(const void* p) { return ((uintptr_t)p & 3) != 0; }

// select the device the reference would: taskID % num_gpus
// (algebra_msm_VariableBaseMSM.cu:1249-1257)
inline int select_device(int task_id) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(OZK_E_NO_DEVICE, "no HIP device available (%s); this library has no CPU path",
                e == hipSuccess ? "count = 0" : hipGetErrorString(e));
  int dev = ((task_id % n) + n) % n;
  OZK_HIP(hipSetDevice(dev));
  return OZK_OK;
}

struct Bump {
  uint8_t* base;
  size_t size, off;
  Bump(void* p, size_t n) : base((uint8_t*)p), size(n), off(0) {}
  template <class T>
  T* take(size_t count) {
    off = (off + 255) & ~(size_t)255;
    T* r = (T*)(base ? base + off : nullptr);
    off += count * sizeof(T);
    return r;
  }
  bool ok() const { return off <= size; }
};

inline int ilog2(uint32_t v) {
  int r = 0;
  while (v >>= 1) r++;
  return r;
}
// The calling thread's HIP error state may hold an error left by somebody else's call (another native library in
// the same process, torch's probes; the runtime keeps the last NON-success code until it is read —
// hip_runtime_api.h, hipGetLastError).  Every function here that checks its kernel launches with
// hipGetLastError() first drops whatever was there, so that the check reports this library's launches only.
inline void hip_clear_stale() { (void)hipGetLastError(); }

}  // namespace ozk
