// mi_spu.hip — C ABI (include/mi_spu.h) of the MI355X decoder of DVD subpictures.  No CPU path: without a gfx950 device
// every call but the host-only one fails with a message.  The control parser: spu_format.h; the kernels: spu_kernels.h.
// Owned memory, errors, the event timer and the bodies of the calls every device library has: host_base.h.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/mi_spu.h"
#include "host_base.h"
#include "spu_kernels.h"

using namespace mispu;

static_assert(MI_SPU_OK == kOk && MI_SPU_ERR_HIP == kErrHip, "header and host base agree");

namespace {
// What one call brings from the host: offsets, lengths, palette_of and the palettes, in pinned memory and on the device.
// A call takes a slot whose last call is over (`done`), so it never touches what a queued launch still reads.
struct CallSlot {
  PinnedBuf<uint8_t> h;
  DevBuf<uint8_t> d;
  Event done;
  bool used = false;
};
constexpr size_t kMaxSlots = 64;  // with this many calls in flight a call waits for the oldest
constexpr int kMaxSide = 4096;
constexpr uint32_t kMaxPacket = 1u << 30;  // the decoder counts a packet's nibbles in 32 bits
uint64_t up16(uint64_t x) { return (x + 15u) & ~(uint64_t)15u; }
}  // namespace

// Device, stream and error text are HostCtx's (host_base.h), destroyed after everything here; the timers go before the
// pool they hand their pairs to.
struct __attribute__((visibility("hidden"))) mi_spu_ctx : HostCtx {
  EventPool ev_free;
  Timer t_scan{ev_free}, t_decode{ev_free};  // mi_spu_times
  std::deque<CallSlot> slots;  // oldest call first
  // mi_spu_decode_frame's staging: one packet, one picture and one info on the device, picture and info in pinned memory
  DevBuf<uint8_t> d_packet, d_pic;
  PinnedBuf<uint8_t> h_pic;
};

namespace {
// a slot no launch reads any more, at the back of the queue: the oldest if its call is over (or if kMaxSlots are in
// flight: after waiting for it), else a new one
int free_slot(mi_spu_ctx* c, CallSlot** out) {
  if (!c->slots.empty()) {
    CallSlot& old = c->slots.front();
    bool over = !old.used;
    if (!over) {
      const hipError_t q = hipEventQuery(old.done);
      if (q == hipSuccess) over = true;
      else if (q != hipErrorNotReady) return fail(c, MI_SPU_ERR_HIP, "hipEventQuery failed: %s", hipGetErrorString(q));
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
      return MI_SPU_OK;
    }
  }
  CallSlot fresh;
  HIPCHK(c, hipEventCreateWithFlags(&fresh.done.p, hipEventDisableTiming));
  c->slots.push_back(std::move(fresh));
  *out = &c->slots.back();
  return MI_SPU_OK;
}

struct Job {
  const uint8_t* stream;
  const uint64_t* offsets;
  const uint32_t* lengths;
  int n, w, h;
  uint8_t* pics;
  uint64_t pic_stride;
  const uint32_t* palettes;
  int n_palettes;
  const uint16_t* palette_of;
  mi_spu_info* info;
};

template <class K>
int timed(mi_spu_ctx* c, Timer& t, const char* name, K launch) {
  int rc = t.begin(c, c->stream);
  if (rc != MI_SPU_OK) return rc;
  launch();
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(c, MI_SPU_ERR_HIP, "the launch of %s failed: %s", name, hipGetErrorString(e));
  return t.end(c, c->stream);
}

// the call's host arrays into the slot and on their way to the device, then the two launches; the checks are the caller's
int stage_and_launch(mi_spu_ctx* c, const Job& j, CallSlot& s) {
  const size_t n = (size_t)j.n;
  const size_t o_len = 8u * n, o_of = 12u * n, o_pal = up16(14u * n), bytes = o_pal + (size_t)j.n_palettes * 64u;
  int rc = s.h.grow(c, bytes, nullptr);  // (no launch uses the slot: nothing is waited for)
  if (rc == MI_SPU_OK) rc = s.d.grow(c, bytes, nullptr);
  if (rc != MI_SPU_OK) return rc;
  uint8_t* h = s.h;
  memcpy(h, j.offsets, 8u * n);
  memcpy(h + o_len, j.lengths, 4u * n);
  if (j.palette_of) memcpy(h + o_of, j.palette_of, 2u * n);
  memcpy(h + o_pal, j.palettes, (size_t)j.n_palettes * 64u);
  HIPCHK(c, hipMemcpyAsync(s.d, h, bytes, hipMemcpyHostToDevice, c->stream));
  Call k;
  k.stream = j.stream, k.offsets = (const uint64_t*)s.d.p, k.lengths = (const uint32_t*)(s.d.p + o_len);
  k.n = (uint32_t)j.n, k.w = (uint32_t)j.w, k.h = (uint32_t)j.h;
  k.info = j.info, k.pics = j.pics, k.pic_stride = j.pic_stride;
  k.palettes = (const uint32_t*)(s.d.p + o_pal);
  k.palette_of = j.palette_of ? (const uint16_t*)(s.d.p + o_of) : nullptr;
  hipStream_t st = c->stream;
  rc = timed(c, c->t_scan, "k_spu_scan", [&] { hipLaunchKernelGGL(k_spu_scan, dim3((k.n + 63u) / 64u), dim3(64), 0, st, k); });
  if (rc == MI_SPU_OK)
    rc = timed(c, c->t_decode, "k_spu_decode", [&] { hipLaunchKernelGGL(k_spu_decode, dim3(2, k.n), dim3(64), 0, st, k); });
  return rc;
}

int run(mi_spu_ctx* c, const Job& j) {
  CallSlot* slot = nullptr;
  int rc = free_slot(c, &slot);
  if (rc != MI_SPU_OK) return rc;
  rc = stage_and_launch(c, j, *slot);
  // whatever became of the launches, the copy may be queued: the slot is free when the stream has passed this point
  slot->used = true;
  const hipError_t e = hipEventRecord(slot->done, c->stream);
  if (e != hipSuccess && rc == MI_SPU_OK) return fail(c, MI_SPU_ERR_HIP, "hipEventRecord failed: %s", hipGetErrorString(e));
  return rc;
}

int check_size(HostCtx* c, const char* who, int w, int h) {
  if (w < 1 || w > kMaxSide || h < 1 || h > kMaxSide) return fail(c, MI_SPU_ERR_ARG, "%s: %d x %d: width and height are 1 to %d", who, w, h, kMaxSide);
  return MI_SPU_OK;
}
}  // namespace

extern "C" {

int mi_spu_device_count(void) { return device_count(); }

const char* mi_spu_last_error(const mi_spu_ctx* c) { return last_error(c); }

mi_spu_ctx* mi_spu_create(int device) {
  if ((device = usable_device(device, "DVD subpicture decoder", MI_SPU_ERR_ARG)) < 0) return nullptr;
  mi_spu_ctx* c = new mi_spu_ctx();
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream.p, hipStreamNonBlocking) != hipSuccess) {
    fail(nullptr, MI_SPU_ERR_HIP, "cannot set up device %d: %s", device, hipGetErrorString(hipGetLastError()));
    mi_spu_destroy(c);
    return nullptr;
  }
  return c;
}

void mi_spu_destroy(mi_spu_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  delete c;
}

void* mi_spu_dev_alloc(mi_spu_ctx* c, size_t bytes) {
  if (!c) return nullptr;
  void* d = nullptr;
  if (hipSetDevice(c->device) != hipSuccess || hipMalloc(&d, bytes ? bytes : 1) != hipSuccess) {
    fail(c, MI_SPU_ERR_NOMEM, "hipMalloc(%zu) failed", bytes);
    return nullptr;
  }
  return d;
}
void mi_spu_dev_free(mi_spu_ctx* c, void* d) { dev_free(c, d); }
int mi_spu_h2d(mi_spu_ctx* c, void* d, const void* h, size_t n) {
  if (!c || (!d && n) || (!h && n)) return fail(c, MI_SPU_ERR_ARG, "mi_spu_h2d: NULL argument");
  return copy_sync(c, d, h, n, hipMemcpyHostToDevice);
}
int mi_spu_d2h(mi_spu_ctx* c, void* h, const void* d, size_t n) {
  if (!c || (!d && n) || (!h && n)) return fail(c, MI_SPU_ERR_ARG, "mi_spu_d2h: NULL argument");
  return copy_sync(c, h, d, n, hipMemcpyDeviceToHost);
}
int mi_spu_sync(mi_spu_ctx* c) { return c ? stream_sync(c) : MI_SPU_ERR_ARG; }

int mi_spu_parse(const uint8_t* pkt, size_t len, int w, int h, mi_spu_info* info) {
  if (!info || (!pkt && len)) {
    fail(nullptr, MI_SPU_ERR_ARG, "mi_spu_parse: NULL argument");
    return MI_SPU_ERR_ARG;
  }
  if (check_size(nullptr, "mi_spu_parse", w, h) != MI_SPU_OK) return MI_SPU_ERR_ARG;
  return parse_control(pkt, (uint64_t)len, w, h, info);
}

int mi_spu_decode_batch(mi_spu_ctx* c, const void* d_stream, const uint64_t* offsets, const uint32_t* lengths, int n, int w, int h,
                        void* d_pics, size_t pic_stride, const uint32_t* palettes, int n_palettes, const uint16_t* palette_of,
                        mi_spu_info* d_info) {
  const char* who = "mi_spu_decode_batch";
  if (!c || !d_stream || !offsets || !lengths || !d_pics || !palettes || !d_info) return fail(c, MI_SPU_ERR_ARG, "%s: NULL argument", who);
  if (n < 1 || n > 65535) return fail(c, MI_SPU_ERR_ARG, "%s: %d packets; 1 to 65535 per call (split the batch)", who, n);
  int rc = check_size(c, who, w, h);
  if (rc != MI_SPU_OK) return rc;
  if (n_palettes < 1 || n_palettes > n) return fail(c, MI_SPU_ERR_ARG, "%s: %d palettes for %d packets; 1 to n", who, n_palettes, n);
  if (palette_of)
    for (int i = 0; i < n; i++)
      if (palette_of[i] >= n_palettes)
        return fail(c, MI_SPU_ERR_ARG, "%s: palette_of[%d] is palette index %u of %d palettes", who, i, (unsigned)palette_of[i], n_palettes);
  const uint64_t picture = (uint64_t)w * (uint64_t)h * 4u;
  if (((uintptr_t)d_pics | pic_stride) & 15u) return fail(c, MI_SPU_ERR_ARG, "%s: d_pics and pic_stride must be 16-byte aligned", who);
  if (pic_stride < picture)
    return fail(c, MI_SPU_ERR_ARG, "%s: a stride of %zu bytes; %d x %d has pictures of %llu", who, pic_stride, w, h, (unsigned long long)picture);
  const uintptr_t s0 = (uintptr_t)d_stream, q0 = (uintptr_t)d_pics, q1 = q0 + (size_t)(n - 1) * pic_stride + (size_t)picture;
  const uintptr_t t0 = (uintptr_t)d_info, t1 = t0 + sizeof(mi_spu_info) * (size_t)n;
  if (t0 & 3u) return fail(c, MI_SPU_ERR_ARG, "%s: d_info must be 4-byte aligned", who);
  if (t0 < q1 && q0 < t1) return fail(c, MI_SPU_ERR_ARG, "%s: d_info overlaps d_pics", who);
  for (int i = 0; i < n; i++) {
    if (lengths[i] >= kMaxPacket) return fail(c, MI_SPU_ERR_ARG, "%s: packet %d has %u bytes; packets stay below 2^30 bytes", who, i, lengths[i]);
    const uintptr_t p0 = s0 + (uintptr_t)offsets[i], p1 = p0 + lengths[i];
    if (p0 < q1 && q0 < p1) return fail(c, MI_SPU_ERR_ARG, "%s: packet %d overlaps d_pics", who, i);
    if (p0 < t1 && t0 < p1) return fail(c, MI_SPU_ERR_ARG, "%s: packet %d overlaps d_info", who, i);
  }
  HIPCHK(c, hipSetDevice(c->device));
  const Job j = {(const uint8_t*)d_stream, offsets, lengths, n, w, h, (uint8_t*)d_pics, (uint64_t)pic_stride, palettes, n_palettes, palette_of, d_info};
  return run(c, j);
}

int mi_spu_decode_frame(mi_spu_ctx* c, const uint8_t* pkt, size_t len, int w, int h, const uint32_t* palette, uint8_t* plane, int stride,
                        mi_spu_info* info) {
  const char* who = "mi_spu_decode_frame";
  if (!c || !pkt || !palette || !plane || !info) return fail(c, MI_SPU_ERR_ARG, "%s: NULL argument", who);
  if (len >= kMaxPacket) return fail(c, MI_SPU_ERR_ARG, "%s: a packet of %zu bytes; packets stay below 2^30 bytes", who, len);
  int rc = check_size(c, who, w, h);
  if (rc != MI_SPU_OK) return rc;
  const uint32_t row = (uint32_t)w * 4u;
  const uint64_t picture = (uint64_t)row * (uint64_t)h;
  if (stride < 0 || (uint32_t)stride < row) return fail(c, MI_SPU_ERR_ARG, "%s: a stride of %d is below the row of %u bytes", who, stride, row);
  if (parse_control(pkt, (uint64_t)len, w, h, info) != MI_SPU_ST_OK)
    return fail(c, MI_SPU_ERR_FORMAT, "%s: the packet is refused with status %d", who, (int)info->status);
  HIPCHK(c, hipSetDevice(c->device));
  // (the stream is idle between these calls: nothing is waited for).  The info lies behind the picture.
  const size_t staged = (size_t)up16(picture) + up16(sizeof(mi_spu_info));
  rc = c->d_packet.grow(c, up16(len), nullptr);
  if (rc == MI_SPU_OK) rc = c->d_pic.grow(c, staged, nullptr);
  if (rc == MI_SPU_OK) rc = c->h_pic.grow(c, staged, nullptr);
  if (rc != MI_SPU_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(c->d_packet, pkt, len, hipMemcpyHostToDevice, c->stream));
  const uint64_t offset = 0;
  const uint32_t length = (uint32_t)len;
  mi_spu_info* d_info = (mi_spu_info*)(c->d_pic.p + up16(picture));
  const Job j = {c->d_packet, &offset, &length, 1, w, h, c->d_pic, up16(picture), palette, 1, nullptr, d_info};
  rc = run(c, j);
  if (rc != MI_SPU_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(c->h_pic, c->d_pic, staged, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  memcpy(info, c->h_pic.p + up16(picture), sizeof *info);
  if (info->status != MI_SPU_ST_OK) return fail(c, MI_SPU_ERR_FORMAT, "%s: the packet is refused with status %d", who, (int)info->status);
  const uint8_t* tight = c->h_pic;
  for (int y = 0; y < h; y++, tight += row) memcpy(plane + (size_t)y * (size_t)stride, tight, row);
  return MI_SPU_OK;
}

int mi_spu_times(mi_spu_ctx* c, float* ms, int* launches) {
  if (!c || !ms || !launches) return MI_SPU_ERR_ARG;
  int rc = stream_sync(c), total = 0;
  Timer* t[2] = {&c->t_scan, &c->t_decode};
  for (int k = 0; k < 2 && rc == MI_SPU_OK; k++) {
    int pairs = 0;
    rc = t[k]->collect(c, &ms[k], &pairs);
    total += pairs;
  }
  if (rc == MI_SPU_OK) *launches = total;
  return rc;
}

}  // extern "C"
