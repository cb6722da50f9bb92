// mi_gsm.hip — C ABI (include/mi_gsm.h) of the MI355X decoder of GSM 06.10 and MS GSM audio.  No CPU path: without a
// gfx950 device every call but the host-only one fails with a message.  The unpacker, the tables and the chain:
// gsm_format.h; the kernels: gsm_kernels.h.  Owned memory, errors, the event timer and the bodies of the calls every
// device library has: host_base.h.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/mi_gsm.h"
#include "host_base.h"
#include "gsm_kernels.h"

using namespace migsm;

static_assert(MI_GSM_OK == kOk && MI_GSM_ERR_HIP == kErrHip, "header and host base agree");
static_assert(MI_GSM_STATE_BYTES == kStateBytes && MI_GSM_PARAMS == kParams && MI_GSM_FRAME_BYTES == kFrameBytes &&
                  MI_GSM_BLOCK_BYTES == kBlockBytes && MI_GSM_FRAME_SAMPLES == kFrameSamples,
              "header and kernels agree");

namespace {
// What one call brings from the host: offsets, pcm_offsets and units, in pinned memory and on the device.  A call takes
// a slot whose last call is over (`done`), so it never touches what a queued launch still reads.
struct CallSlot {
  PinnedBuf<uint8_t> h;
  DevBuf<uint8_t> d;
  Event done;
  bool used = false;
};
constexpr size_t kMaxSlots = 64;  // with this many calls in flight a call waits for the oldest
uint64_t up16(uint64_t x) { return (x + 15u) & ~(uint64_t)15u; }
}  // namespace

// Device, stream and error text are HostCtx's (host_base.h), destroyed after everything here; the timer goes before the
// pool it hands its pairs to.
struct __attribute__((visibility("hidden"))) mi_gsm_ctx : HostCtx {
  EventPool ev_free;
  Timer t_decode{ev_free};     // mi_gsm_times
  std::deque<CallSlot> slots;  // oldest call first
  // mi_gsm_decode_stream's staging: the stream on the device; samples, state and count on the device and in pinned memory
  DevBuf<uint8_t> d_in, d_out;
  PinnedBuf<uint8_t> h_out;
};

namespace {
// a slot no launch reads any more, at the back of the queue: the oldest if its call is over (or if kMaxSlots are in
// flight: after waiting for it), else a new one
int free_slot(mi_gsm_ctx* c, CallSlot** out) {
  if (!c->slots.empty()) {
    CallSlot& old = c->slots.front();
    bool over = !old.used;
    if (!over) {
      const hipError_t q = hipEventQuery(old.done);
      if (q == hipSuccess) over = true;
      else if (q != hipErrorNotReady) return fail(c, MI_GSM_ERR_HIP, "hipEventQuery failed: %s", hipGetErrorString(q));
      (void)hipGetLastError();  // ("not ready" is no error of the launch that follows)
      if (!over && c->slots.size() >= kMaxSlots) {
        HIPCHK(c, hipEventSynchronize(old.done));
        over = true;
      }
    }
    if (over) {
      c->slots.push_back(std::move(old));
      c->slots.pop_front();
      *out = &c->slots.back();
      return MI_GSM_OK;
    }
  }
  CallSlot fresh;
  HIPCHK(c, hipEventCreateWithFlags(&fresh.done.p, hipEventDisableTiming));
  c->slots.push_back(std::move(fresh));
  *out = &c->slots.back();
  return MI_GSM_OK;
}

struct Job {
  const uint8_t* stream;
  const uint64_t* offsets;
  const uint32_t* units;
  int n, fmt;
  uint8_t* pcm;
  const uint64_t* pcm_offsets;
  uint8_t* state;
  uint32_t* bad;
};

// the call's host arrays into the slot and on their way to the device, then the launch; the checks are the caller's
int stage_and_launch(mi_gsm_ctx* c, const Job& j, CallSlot& s) {
  const size_t n = (size_t)j.n, o_pcm = 8u * n, o_units = 16u * n, bytes = 20u * n;
  int rc = s.h.grow(c, bytes, nullptr);  // (no launch uses the slot: nothing is waited for)
  if (rc == MI_GSM_OK) rc = s.d.grow(c, bytes, nullptr);
  if (rc != MI_GSM_OK) return rc;
  uint8_t* h = s.h;
  memcpy(h, j.offsets, 8u * n);
  memcpy(h + o_pcm, j.pcm_offsets, 8u * n);
  memcpy(h + o_units, j.units, 4u * n);
  HIPCHK(c, hipMemcpyAsync(s.d, h, bytes, hipMemcpyHostToDevice, c->stream));
  Call k;
  k.stream = j.stream, k.offsets = (const uint64_t*)s.d.p, k.pcm_offsets = (const uint64_t*)(s.d.p + o_pcm);
  k.units = (const uint32_t*)(s.d.p + o_units);
  k.n = (uint32_t)j.n, k.fmt = (uint32_t)j.fmt, k.pcm = j.pcm, k.state = j.state, k.bad = j.bad;
  rc = c->t_decode.begin(c, c->stream);
  if (rc != MI_GSM_OK) return rc;
  hipLaunchKernelGGL(k_gsm_decode, dim3((k.n + kLanes - 1u) / kLanes), dim3(kLanes), 0, c->stream, k);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(c, MI_GSM_ERR_HIP, "the launch of k_gsm_decode failed: %s", hipGetErrorString(e));
  return c->t_decode.end(c, c->stream);
}

int run(mi_gsm_ctx* c, const Job& j) {
  CallSlot* slot = nullptr;
  int rc = free_slot(c, &slot);
  if (rc != MI_GSM_OK) return rc;
  rc = stage_and_launch(c, j, *slot);
  // whatever became of the launch, the copy may be queued: the slot is free when the stream has passed this point
  slot->used = true;
  const hipError_t e = hipEventRecord(slot->done, c->stream);
  if (e != hipSuccess && rc == MI_GSM_OK) return fail(c, MI_GSM_ERR_HIP, "hipEventRecord failed: %s", hipGetErrorString(e));
  return rc;
}

int reset_states(mi_gsm_ctx* c, void* d_state, int n) {
  const uint32_t pieces = (uint32_t)n * (kStateBytes / 16u);
  hipLaunchKernelGGL(k_gsm_state_reset, dim3((pieces + 255u) / 256u), dim3(256), 0, c->stream, (uint4*)d_state, pieces);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(c, MI_GSM_ERR_HIP, "the launch of k_gsm_state_reset failed: %s", hipGetErrorString(e));
  return MI_GSM_OK;
}
}  // namespace

extern "C" {

int mi_gsm_device_count(void) { return device_count(); }

const char* mi_gsm_last_error(const mi_gsm_ctx* c) { return last_error(c); }

mi_gsm_ctx* mi_gsm_create(int device) {
  if ((device = usable_device(device, "GSM 06.10 decoder", MI_GSM_ERR_ARG)) < 0) return nullptr;
  mi_gsm_ctx* c = new mi_gsm_ctx();
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream.p, hipStreamNonBlocking) != hipSuccess) {
    fail(nullptr, MI_GSM_ERR_HIP, "cannot set up device %d: %s", device, hipGetErrorString(hipGetLastError()));
    mi_gsm_destroy(c);
    return nullptr;
  }
  return c;
}

void mi_gsm_destroy(mi_gsm_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  delete c;
}

void* mi_gsm_dev_alloc(mi_gsm_ctx* c, size_t bytes) {
  if (!c) return nullptr;
  void* d = nullptr;
  if (hipSetDevice(c->device) != hipSuccess || hipMalloc(&d, bytes ? bytes : 1) != hipSuccess) {
    fail(c, MI_GSM_ERR_NOMEM, "hipMalloc(%zu) failed", bytes);
    return nullptr;
  }
  return d;
}
void mi_gsm_dev_free(mi_gsm_ctx* c, void* d) { dev_free(c, d); }
int mi_gsm_h2d(mi_gsm_ctx* c, void* d, const void* h, size_t n) {
  if (!c || (!d && n) || (!h && n)) return fail(c, MI_GSM_ERR_ARG, "mi_gsm_h2d: NULL argument");
  return copy_sync(c, d, h, n, hipMemcpyHostToDevice);
}
int mi_gsm_d2h(mi_gsm_ctx* c, void* h, const void* d, size_t n) {
  if (!c || (!d && n) || (!h && n)) return fail(c, MI_GSM_ERR_ARG, "mi_gsm_d2h: NULL argument");
  return copy_sync(c, h, d, n, hipMemcpyDeviceToHost);
}
int mi_gsm_sync(mi_gsm_ctx* c) { return c ? stream_sync(c) : MI_GSM_ERR_ARG; }

int mi_gsm_state_reset(mi_gsm_ctx* c, void* d_state, int n) {
  const char* who = "mi_gsm_state_reset";
  if (!c || !d_state) return fail(c, MI_GSM_ERR_ARG, "%s: NULL argument", who);
  if (n < 1 || n > MI_GSM_MAX_STREAMS) return fail(c, MI_GSM_ERR_ARG, "%s: %d states; 1 to %d", who, n, (int)MI_GSM_MAX_STREAMS);
  if ((uintptr_t)d_state & 15u) return fail(c, MI_GSM_ERR_ARG, "%s: d_state must be 16-byte aligned", who);
  HIPCHK(c, hipSetDevice(c->device));
  return reset_states(c, d_state, n);
}

int mi_gsm_explode(const uint8_t* block, int fmt, int16_t* params) {
  if (!block || !params || (fmt != 0 && fmt != 1)) {
    fail(nullptr, MI_GSM_ERR_ARG, "mi_gsm_explode: a NULL argument, or fmt %d is neither 0 nor 1", fmt);
    return MI_GSM_ERR_ARG;
  }
  if (fmt == 0) {
    if ((block[0] >> 4) != 0xD) return 1;
    unpack([&](int b) { return (uint32_t)block[b]; }, true, 4, [&](int at, uint8_t v) { params[at] = v; });
    return 0;
  }
  unpack([&](int b) { return (uint32_t)block[b]; }, false, 0, [&](int at, uint8_t v) { params[at] = v; });
  unpack([&](int b) { return (uint32_t)block[32 + b]; }, false, 4, [&](int at, uint8_t v) { params[kParams + at] = v; });
  return 0;
}

int mi_gsm_decode_batch(mi_gsm_ctx* c, const void* d_stream, const uint64_t* offsets, const uint32_t* units, int n, int fmt,
                        void* d_pcm, const uint64_t* pcm_offsets, void* d_state, uint32_t* d_bad) {
  const char* who = "mi_gsm_decode_batch";
  if (!c || !d_stream || !offsets || !units || !d_pcm || !pcm_offsets) return fail(c, MI_GSM_ERR_ARG, "%s: NULL argument", who);
  if (n < 1 || n > MI_GSM_MAX_STREAMS) return fail(c, MI_GSM_ERR_ARG, "%s: %d streams; 1 to %d per call (split the batch)", who, n, (int)MI_GSM_MAX_STREAMS);
  if (fmt != 0 && fmt != 1) return fail(c, MI_GSM_ERR_ARG, "%s: fmt %d; 0 is the plain framing, 1 the Microsoft one", who, fmt);
  if ((uintptr_t)d_pcm & 15u) return fail(c, MI_GSM_ERR_ARG, "%s: d_pcm must be 16-byte aligned", who);
  if ((uintptr_t)d_state & 15u) return fail(c, MI_GSM_ERR_ARG, "%s: d_state must be 16-byte aligned", who);
  if ((uintptr_t)d_bad & 3u) return fail(c, MI_GSM_ERR_ARG, "%s: d_bad must be 4-byte aligned", who);
  if (d_state && d_bad) {
    const uintptr_t s0 = (uintptr_t)d_state, s1 = s0 + (size_t)n * kStateBytes, b0 = (uintptr_t)d_bad, b1 = b0 + 4u * (size_t)n;
    if (s0 < b1 && b0 < s1) return fail(c, MI_GSM_ERR_ARG, "%s: d_bad overlaps d_state", who);
  }
  for (int i = 0; i < n; i++) {
    if (units[i] > (uint32_t)MI_GSM_MAX_UNITS) return fail(c, MI_GSM_ERR_ARG, "%s: stream %d has %u units; at most %d", who, i, units[i], (int)MI_GSM_MAX_UNITS);
    if (pcm_offsets[i] & 15u) return fail(c, MI_GSM_ERR_ARG, "%s: pcm_offsets[%d] must be a multiple of 16", who, i);
  }
  HIPCHK(c, hipSetDevice(c->device));
  const Job j = {(const uint8_t*)d_stream, offsets, units, n, fmt, (uint8_t*)d_pcm, pcm_offsets, (uint8_t*)d_state, d_bad};
  return run(c, j);
}

int mi_gsm_decode_stream(mi_gsm_ctx* c, const uint8_t* bytes, size_t len, int fmt, int16_t* pcm, void* state_or_null, uint32_t* bad) {
  const char* who = "mi_gsm_decode_stream";
  if (!c || (!bytes && len) || (fmt != 0 && fmt != 1)) return fail(c, MI_GSM_ERR_ARG, "%s: a NULL argument, or fmt %d is neither 0 nor 1", who, fmt);
  const size_t unit = fmt ? kBlockBytes : kFrameBytes, n_units = len / unit;
  if (n_units > (size_t)MI_GSM_MAX_UNITS) return fail(c, MI_GSM_ERR_ARG, "%s: %zu units; at most %d a call", who, n_units, (int)MI_GSM_MAX_UNITS);
  if (!pcm && n_units) return fail(c, MI_GSM_ERR_ARG, "%s: NULL argument", who);
  const size_t samples = n_units * (size_t)(kFrameSamples << fmt) * 2u, used = n_units * unit;
  HIPCHK(c, hipSetDevice(c->device));
  // (the stream is idle between these calls: nothing is waited for).  State and count lie behind the samples.
  const size_t o_state = (size_t)up16(samples), o_bad = o_state + kStateBytes, staged = o_bad + 16u;
  int rc = c->d_in.grow(c, up16(used ? used : 1), nullptr);
  if (rc == MI_GSM_OK) rc = c->d_out.grow(c, staged, nullptr);
  if (rc == MI_GSM_OK) rc = c->h_out.grow(c, staged, nullptr);
  if (rc != MI_GSM_OK) return rc;
  if (used) HIPCHK(c, hipMemcpyAsync(c->d_in, bytes, used, hipMemcpyHostToDevice, c->stream));
  uint8_t* d_state = c->d_out.p + o_state;
  if (state_or_null) {
    memcpy(c->h_out.p + o_state, state_or_null, kStateBytes);
    HIPCHK(c, hipMemcpyAsync(d_state, c->h_out.p + o_state, kStateBytes, hipMemcpyHostToDevice, c->stream));
  }
  const uint64_t zero = 0;
  const uint32_t units = (uint32_t)n_units;
  const Job j = {c->d_in, &zero, &units, 1, fmt, c->d_out, &zero, state_or_null ? d_state : nullptr, (uint32_t*)(c->d_out.p + o_bad)};
  rc = run(c, j);
  if (rc != MI_GSM_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(c->h_out, c->d_out, staged, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (samples) memcpy(pcm, c->h_out.p, samples);
  if (state_or_null) memcpy(state_or_null, c->h_out.p + o_state, kStateBytes);
  if (bad) memcpy(bad, c->h_out.p + o_bad, 4);
  return MI_GSM_OK;
}

int mi_gsm_times(mi_gsm_ctx* c, float* ms, int* launches) { return times(c, c ? &c->t_decode : nullptr, 1, ms, launches, MI_GSM_ERR_ARG); }

}  // extern "C"
