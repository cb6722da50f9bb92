// rtj_host_buf.h — device and pinned host memory that frees itself, and how the host layer reports an error.
// Included by mi_rtjpeg.hip (one translation unit); not a kernel header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

#include "../../include/mi_rtjpeg.h"
#include "host_owned.h"

namespace {

// writes the message into the instance (or, without one, into the text mi_rtj_last_error(NULL) returns); returns `code`
int fail(mi_rtj_ctx* c, int code, const char* fmt, ...);

#define HIPCHK(c, call)                                                                       \
  do {                                                                                        \
    hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess)                                                                     \
      return fail((c), MI_RTJ_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                  __FILE__, __LINE__);                                                        \
  } while (0)

// Device memory (Owned: host_owned.h).  It only ever grows.
template <class T>
struct DevBuf : Owned<T, hipFree> {
  // Room for n elements (+ pad_bytes behind them).  Nothing happens if they fit.  Otherwise work queued on `stream` may
  // still use the old buffer: it is waited for (only if there is a buffer; a null stream: the caller has waited), the
  // buffer is freed and the object left empty, and only then is the new one allocated — a failed allocation leaves the
  // object empty.  zero: the new buffer is cleared, on `stream`.
  int grow(mi_rtj_ctx* c, uint64_t n, hipStream_t stream, size_t pad_bytes = 0, bool zero = false) {
    if (n <= this->cap) return MI_RTJ_OK;
    if (this->p && stream) HIPCHK(c, hipStreamSynchronize(stream));
    this->release();
    const size_t bytes = sizeof(T) * (size_t)n + pad_bytes;
    HIPCHK(c, hipMalloc((void**)&this->p, bytes));
    this->cap = n;
    if (zero) HIPCHK(c, hipMemsetAsync(this->p, 0, bytes, stream));
    return MI_RTJ_OK;
  }
};

// buffers that are sized together: one wait for all of them, then every one is empty and grows without waiting again
template <class... B>
int dev_release(mi_rtj_ctx* c, hipStream_t stream, B&... b) {
  if ((... || (b.p != nullptr))) HIPCHK(c, hipStreamSynchronize(stream));
  (..., b.release());
  return MI_RTJ_OK;
}

// Pinned host memory (flags: hipHostMalloc's; mapped memory's device address is the caller's to ask for).
template <class T>
struct PinnedBuf : Owned<T, hipHostFree> {
  hipError_t alloc(uint64_t n, unsigned flags = hipHostMallocDefault) {
    this->release();
    const hipError_t e = hipHostMalloc((void**)&this->p, sizeof(T) * (size_t)n, flags);
    if (e == hipSuccess) this->cap = n;
    else this->p = nullptr;
    return e;
  }
  int grow(mi_rtj_ctx* c, uint64_t n) {
    if (n <= this->cap) return MI_RTJ_OK;
    HIPCHK(c, alloc(n));
    return MI_RTJ_OK;
  }
};

}  // namespace
