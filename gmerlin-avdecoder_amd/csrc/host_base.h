// host_base.h — the host layer the device libraries share (libmi_rtjpeg.so, libmi_dv.so, libmi_yuv.so, libmi_rgb.so, libmi_tga.so, libmi_spu.so, libmi_gsm.so, libmi_pcm.so):
// memory, streams and events that free themselves, the base of an instance, how an error becomes a code and a text, the
// checked HIP call, buffers that only grow, the event timer around a launch, and the bodies of the entry points every
// library has.  Host only; depends on HIP and the standard library, on none of the public headers.  Each library is one
// translation unit that includes this once: what the anonymous namespace holds is one per .so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <deque>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

namespace {

// every public header has these two at these values (each .hip asserts it); the codes that differ are passed in
constexpr int kOk = 0, kErrHip = -2;

// `cap` elements at `p`, owned: move-only, freed by the destructor
template <class T, hipError_t (*Free)(void*)>
struct Owned {
  T* p = nullptr;
  uint64_t cap = 0;

  Owned() = default;
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  Owned(Owned&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) {
      release();
      std::swap(p, o.p);
      std::swap(cap, o.cap);
    }
    return *this;
  }
  ~Owned() { release(); }
  operator T*() const { return p; }
  void release() {
    if (p) (void)Free(p);
    p = nullptr;
    cap = 0;
  }
};

// streams and events: owned like memory (the capacity stays 0; created through &x.p)
inline hipError_t destroy_stream(void* s) { return hipStreamDestroy((hipStream_t)s); }
inline hipError_t destroy_event(void* e) { return hipEventDestroy((hipEvent_t)e); }
using Stream = Owned<ihipStream_t, destroy_stream>;
using Event = Owned<ihipEvent_t, destroy_event>;
struct EventPair {
  Event start, stop;
};
using EventPool = std::vector<EventPair>;  // pairs nobody uses: one pool an instance, shared by its timers

// What every instance begins with.  A base is destroyed after the members of the struct derived from it: every buffer
// and event of an instance goes before its stream.
struct HostCtx {
  int device = 0;
  Stream stream;
  std::string err;
};

std::mutex g_err_mu;
std::string g_err;  // what the calls without an instance report

// writes the message into the instance (or, without one, into the text last_error(nullptr) returns); returns `code`
int fail(HostCtx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  else {
    std::lock_guard<std::mutex> l(g_err_mu);
    g_err = buf;
  }
  return code;
}
// the body of *_last_error; without an instance a copy of the calling thread's own, which another thread's fail() leaves alone
const char* last_error(const HostCtx* c) {
  if (c) return c->err.c_str();
  static thread_local std::string copy;
  std::lock_guard<std::mutex> l(g_err_mu);
  copy = g_err;
  return copy.c_str();
}

#define HIPCHK(c, call)                                                                                          \
  do {                                                                                                           \
    hipError_t e_ = (call);                                                                                      \
    if (e_ != hipSuccess)                                                                                        \
      return fail((c), kErrHip, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__);      \
  } while (0)

inline hipError_t device_malloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
inline hipError_t pinned_malloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }

// Memory that only ever grows.
template <class T, hipError_t (*Alloc)(void**, size_t), hipError_t (*Free)(void*)>
struct GrowBuf : Owned<T, Free> {
  // Room for n elements (+ pad_bytes behind them).  Nothing happens if they fit.  Otherwise work queued on `stream` may
  // still use the old buffer: it is waited for (only if there is a buffer; a null stream: the caller has waited), the
  // buffer is freed and the object left empty, and only then is the new one allocated — a failed allocation leaves the
  // object empty.  zero: the new buffer is cleared, on `stream`.
  int grow(HostCtx* c, uint64_t n, hipStream_t stream, size_t pad_bytes = 0, bool zero = false) {
    if (n <= this->cap) return kOk;
    if (this->p && stream) HIPCHK(c, hipStreamSynchronize(stream));
    this->release();
    const size_t bytes = sizeof(T) * (size_t)n + pad_bytes;
    HIPCHK(c, Alloc((void**)&this->p, bytes));
    this->cap = n;
    if (zero) HIPCHK(c, hipMemsetAsync(this->p, 0, bytes, stream));
    return kOk;
  }
};
template <class T>
using DevBuf = GrowBuf<T, device_malloc, hipFree>;
template <class T>
using PinnedBuf = GrowBuf<T, pinned_malloc, hipHostFree>;

// buffers that are sized together: one wait for all of them, then every one is empty and grows without waiting again
template <class... B>
int release_together(HostCtx* c, hipStream_t stream, B&... b) {
  if ((... || (b.p != nullptr))) HIPCHK(c, hipStreamSynchronize(stream));
  (..., b.release());
  return kOk;
}

// Device time of one kind of launch: a pair of events around each since the last collect().  Nobody may ever ask: the
// newest kKeep pairs are kept (the public headers state the figure), the oldest goes back to the pool.
struct Timer {
  static constexpr size_t kKeep = 4096;
  EventPool& pool;
  std::deque<EventPair> used;  // recorded on both sides
  EventPair open;              // between begin() and end()

  explicit Timer(EventPool& p) : pool(p) {}

  // a start event, recorded on the stream; the pair is created completely or not at all
  int begin(HostCtx* c, hipStream_t stream) {
    if (open.start) pool.push_back(std::move(open));  // (a launch failed between begin() and end())
    if (!pool.empty()) {
      open = std::move(pool.back());
      pool.pop_back();
    } else {
      EventPair e;  // (a failure below destroys what it holds)
      HIPCHK(c, hipEventCreate(&e.start.p));
      HIPCHK(c, hipEventCreate(&e.stop.p));
      open = std::move(e);
    }
    return record(c, open.start, stream);
  }
  // the stop event; only a pair recorded on both sides is one collect() reads
  int end(HostCtx* c, hipStream_t stream) {
    const int rc = record(c, open.stop, stream);
    if (rc != kOk) return rc;
    used.push_back(std::move(open));
    if (used.size() > kKeep) {
      pool.push_back(std::move(used.front()));
      used.pop_front();
    }
    return kOk;
  }
  // the sum over the pairs and their number; the caller has waited for the stream.  The pairs go back to the pool whether
  // or not every one could be read
  int collect(HostCtx* c, float* total_ms, int* pairs) {
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
    if (bad != hipSuccess) return fail(c, kErrHip, "hipEventElapsedTime failed: %s", hipGetErrorString(bad));
    *total_ms = sum;
    *pairs = n;
    return kOk;
  }

 private:
  int record(HostCtx* c, hipEvent_t e, hipStream_t stream) {
    const hipError_t r = hipEventRecord(e, stream);
    if (r == hipSuccess) return kOk;
    pool.push_back(std::move(open));
    return fail(c, kErrHip, "hipEventRecord failed: %s", hipGetErrorString(r));
  }
};

// ---- the bodies of the entry points every library has; the refusal of a NULL argument, with the library's own code and
// text, is the entry point's ----
bool is_gfx950(int dev) {
  hipDeviceProp_t p;
  return hipGetDeviceProperties(&p, dev) == hipSuccess && strncmp(p.gcnArchName, "gfx950", 6) == 0;
}
int device_count() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  int ok = 0;
  for (int i = 0; i < n; i++) ok += is_gfx950(i);
  return ok;
}
// *_create of a library without a CPU path, up to `new`: the device to use (negative: the current one), or -1 and the
// message, which names the library as "the <noun>"
int usable_device(int device, const char* noun, int err_arg) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
    fail(nullptr, kErrHip, "no HIP device: the %s has no CPU path", noun);
    return -1;
  }
  if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
  if (device >= n || !is_gfx950(device)) {
    fail(nullptr, err_arg, "device %d is not a gfx950 (MI355X) device", device);
    return -1;
  }
  return device;
}
int stream_sync(HostCtx* c) {
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return kOk;
}
// *_h2d and *_d2h: n bytes on the instance's stream, waited for
int copy_sync(HostCtx* c, void* dst, const void* src, size_t n, hipMemcpyKind kind) {
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemcpyAsync(dst, src, n, kind, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return kOk;
}
void dev_free(HostCtx* c, void* d) {
  if (!c || !d) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  (void)hipFree(d);
}
// the body of the *_times: waits for the stream, then the timer's sum and `per_pair` launches a pair
int times(HostCtx* c, Timer* t, int per_pair, float* total_ms, int* launches, int err_arg) {
  if (!c || !total_ms || !launches) return err_arg;
  int rc = stream_sync(c), pairs = 0;
  if (rc == kOk) rc = t->collect(c, total_ms, &pairs);
  if (rc == kOk) *launches = per_pair * pairs;
  return rc;
}

}  // namespace
