// dv_host_buf.h — what a DV instance owns (device and pinned memory, its stream, its events), how the host layer reports an
// error, and the timer around its launches.  Included by mi_dv.hip (one translation unit); not a kernel header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <deque>
#include <vector>

#include "../../include/mi_dv.h"
#include "host_owned.h"

namespace {

// writes the message into the instance (or, without one, into the text mi_dv_last_error(NULL) returns); returns `code`
int fail(mi_dv_ctx* c, int code, const char* fmt, ...);

#define DVCHK(c, call)                                                                                              \
  do {                                                                                                              \
    hipError_t e_ = (call);                                                                                         \
    if (e_ != hipSuccess)                                                                                           \
      return fail((c), MI_DV_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__);   \
  } while (0)

inline hipError_t device_malloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
inline hipError_t pinned_malloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }

// Memory that only ever grows.
template <class T, hipError_t (*Alloc)(void**, size_t), hipError_t (*Free)(void*)>
struct GrowBuf : Owned<T, Free> {
  // Room for n elements.  Nothing happens if they fit.  Otherwise work queued on `stream` may still use the old buffer: it
  // is waited for (only if there is a buffer; a null stream: the caller has waited), the buffer is freed and the object
  // left empty, and only then is the new one allocated — a failed allocation leaves the object empty.
  int grow(mi_dv_ctx* c, uint64_t n, hipStream_t stream) {
    if (n <= this->cap) return MI_DV_OK;
    if (this->p && stream) DVCHK(c, hipStreamSynchronize(stream));
    this->release();
    DVCHK(c, Alloc((void**)&this->p, sizeof(T) * (size_t)n));
    this->cap = n;
    return MI_DV_OK;
  }
};
template <class T>
using DevBuf = GrowBuf<T, device_malloc, hipFree>;
template <class T>
using PinnedBuf = GrowBuf<T, pinned_malloc, hipHostFree>;

// buffers that are sized together: one wait for all of them, then every one is empty and grows without waiting again
template <class... B>
int release_together(mi_dv_ctx* c, hipStream_t stream, B&... b) {
  if ((... || (b.p != nullptr))) DVCHK(c, hipStreamSynchronize(stream));
  (..., b.release());
  return MI_DV_OK;
}

// the stream and the events: owned like memory (the capacity stays 0)
inline hipError_t destroy_stream(void* s) { return hipStreamDestroy((hipStream_t)s); }
inline hipError_t destroy_event(void* e) { return hipEventDestroy((hipEvent_t)e); }
using Stream = Owned<ihipStream_t, destroy_stream>;
using Event = Owned<ihipEvent_t, destroy_event>;

struct EventPair {
  Event start, stop;
};
using EventPool = std::vector<EventPair>;  // pairs nobody uses: one pool an instance, shared by its timers

// Device time of one kind of launch: a pair of events around each since the last collect().  Nobody may ever ask: the
// newest kKeep pairs are kept (include/mi_dv.h states the figure), the oldest goes back to the pool.
struct Timer {
  static constexpr size_t kKeep = 4096;
  EventPool& pool;
  std::deque<EventPair> used;  // recorded on both sides
  EventPair open;              // between begin() and end()

  explicit Timer(EventPool& p) : pool(p) {}

  // a start event, recorded on the stream; the pair is created completely or not at all
  int begin(mi_dv_ctx* c, hipStream_t stream) {
    if (open.start) pool.push_back(std::move(open));  // (a launch failed between begin() and end())
    if (!pool.empty()) {
      open = std::move(pool.back());
      pool.pop_back();
    } else {
      EventPair e;  // (a failure below destroys what it holds)
      DVCHK(c, hipEventCreate(&e.start.p));
      DVCHK(c, hipEventCreate(&e.stop.p));
      open = std::move(e);
    }
    return record(c, open.start, stream);
  }
  // the stop event; only a pair recorded on both sides is one collect() reads
  int end(mi_dv_ctx* c, hipStream_t stream) {
    const int rc = record(c, open.stop, stream);
    if (rc != MI_DV_OK) return rc;
    used.push_back(std::move(open));
    if (used.size() > kKeep) {
      pool.push_back(std::move(used.front()));
      used.pop_front();
    }
    return MI_DV_OK;
  }
  // the sum over the pairs and their number; the caller has waited for the stream.  The pairs go back to the pool whether
  // or not every one could be read
  int collect(mi_dv_ctx* c, float* total_ms, int* pairs) {
    hipError_t bad = hipSuccess;
    float sum = 0.f;
    const int n = (int)used.size();
    for (EventPair& e : used) {
      float ms = 0.f;
      const hipError_t r = hipEventElapsedTime(&ms, e.start, e.stop);
      if (r != hipSuccess) bad = r;
      sum += ms;
      pool.push_back(std::move(e));
    }
    used.clear();
    if (bad != hipSuccess) return fail(c, MI_DV_ERR_HIP, "hipEventElapsedTime failed: %s", hipGetErrorString(bad));
    *total_ms = sum;
    *pairs = n;
    return MI_DV_OK;
  }

 private:
  int record(mi_dv_ctx* c, hipEvent_t e, hipStream_t stream) {
    const hipError_t r = hipEventRecord(e, stream);
    if (r == hipSuccess) return MI_DV_OK;
    pool.push_back(std::move(open));
    return fail(c, MI_DV_ERR_HIP, "hipEventRecord failed: %s", hipGetErrorString(r));
  }
};

}  // namespace
