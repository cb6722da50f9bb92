// mi_rgb.hip — C ABI (include/mi_rgb.h) of the MI355X unpacker of the raw RGB family of QuickTime and AVI.  No CPU path:
// without a gfx950 device every call but the two host-only queries fails with a message.  The kernels and the format
// table: rgb_unpack_kernels.h.  Owned memory, errors, the event timer and the bodies of the calls every device library
// has: host_base.h.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/mi_rgb.h"
#include "host_base.h"
#include "rgb_unpack_kernels.h"

using namespace mirgb;

static_assert(kQt1 == MI_RGB_QT1 && kQt2 == MI_RGB_QT2 && kQt4 == MI_RGB_QT4 && kQt8 == MI_RGB_QT8 && kQt16 == MI_RGB_QT16 &&
                  kQt24 == MI_RGB_QT24 && kQt32 == MI_RGB_QT32 && kAvi8 == MI_RGB_AVI8 && kAvi8Gray == MI_RGB_AVI8_GRAY &&
                  kAvi16 == MI_RGB_AVI16 && kMtv16 == MI_RGB_MTV16 && kAvi24 == MI_RGB_AVI24 && kAvi32 == MI_RGB_AVI32 &&
                  kCodecs == MI_RGB_CODECS,
              "header and kernels agree");
static_assert(MI_RGB_OK == kOk && MI_RGB_ERR_HIP == kErrHip, "header and host base agree");

namespace {
// The palettes of one launch: reduced to 256 x (R G B 0) each, with the launch's palette_of behind them, in pinned
// memory and on the device.  A launch takes a slot whose last launch is over (`done`), so a call never touches what a
// queued launch still reads.
struct PaletteSlot {
  PinnedBuf<uint8_t> h;
  DevBuf<uint8_t> d;
  Event done;
  bool used = false;
};
constexpr size_t kMaxSlots = 64;  // with this many launches in flight a call waits for the oldest
}  // namespace

// Device, stream and error text are HostCtx's (host_base.h), destroyed after everything here; the timer goes before
// the pool it hands its pairs to.
struct __attribute__((visibility("hidden"))) mi_rgb_ctx : HostCtx {
  EventPool ev_free;
  Timer time{ev_free};  // the unpack launches (mi_rgb_times)
  std::deque<PaletteSlot> slots;  // oldest launch first
  // mi_rgb_unpack_frame's staging: one packet and one picture on the device, the picture in pinned memory; they only grow
  DevBuf<uint8_t> d_packet, d_pic;
  PinnedBuf<uint8_t> h_pic;
};

namespace {
// a codec and a size, checked against the format table: the shape, or a message that names the rule
int checked_shape(mi_rgb_ctx* c, const char* who, int codec, int w, int h, Shape* s) {
  if (codec < 0 || codec >= kCodecs) return fail(c, MI_RGB_ERR_ARG, "%s: unknown codec %d", who, codec);
  const Format& f = kFormats[codec];
  if (w <= 0 || h <= 0) return fail(c, MI_RGB_ERR_ARG, "%s: %s at %d x %d: width and height are positive", who, f.name, w, h);
  if ((uint32_t)w % f.w_mult)
    return fail(c, MI_RGB_ERR_ARG, "%s: %s at %d x %d: the width is a multiple of %u", who, f.name, w, h, f.w_mult);
  const bool fits = (uint64_t)w * (uint64_t)h < (1ull << 31);  // (no picture has less than a byte a pixel)
  *s = shape_of(codec, fits ? (uint64_t)w : 65536u, fits ? (uint64_t)h : 32768u);
  if (s->packet_bytes >= (1ull << 31) || s->picture_bytes >= (1ull << 31))
    return fail(c, MI_RGB_ERR_ARG, "%s: %s at %d x %d: packets and pictures stay below 2^31 bytes", who, f.name, w, h);
  return MI_RGB_OK;
}

// ---- the launches; checks, events and errors are their caller's ----
struct Job {
  const uint8_t* packets;
  uint64_t packet_stride;
  int n;
  uint8_t* pics;
  uint64_t pic_stride;
  const uint32_t* d_palettes;     // 256 words a palette, on the device (palette kernels only)
  const uint16_t* d_palette_of;   // n indices on the device, or nullptr
};
template <class P>
void move_launch(hipStream_t st, int codec, const Shape& s, const Job& j) {
  const MoveGeo g = move_geo(codec, s);
  const uint32_t gx = (g.items + kThreads - 1u) / kThreads;
  hipLaunchKernelGGL(k_rgb_move<P>, dim3(gx < kMaxGridX ? gx : kMaxGridX, (unsigned)j.n), dim3(kThreads), 0, st, j.packets,
                     j.packet_stride, j.pics, j.pic_stride, g);
}
template <int Bits>
void palette_launch(hipStream_t st, int codec, const Shape& s, const Job& j) {
  const PaletteGeo g = palette_geo(codec, s);
  hipLaunchKernelGGL(k_rgb_palette<Bits>, dim3(g.chunks < kMaxGridX ? g.chunks : kMaxGridX, (unsigned)j.n), dim3(kThreads), 0, st,
                     j.packets, j.packet_stride, j.pics, j.pic_stride, j.d_palettes, j.d_palette_of, g);
}
using Launch = void (*)(hipStream_t, int, const Shape&, const Job&);
constexpr Launch launch_of(const Format& f) {
  return f.kind == kMove     ? move_launch<None>
         : f.kind == kSwap16 ? move_launch<Swap16>
         : f.kind == kRot32  ? move_launch<Rot32>
         : f.bits == 1       ? palette_launch<1>
         : f.bits == 2       ? palette_launch<2>
         : f.bits == 4       ? palette_launch<4>
                             : palette_launch<8>;
}

// the checked launch over n resident packets, timed (a launch that fails leaves the timer's pair open: it goes back to
// the pool at the next begin())
int run(mi_rgb_ctx* c, int codec, const Shape& s, const Job& j) {
  const int rc = c->time.begin(c, c->stream);
  if (rc != MI_RGB_OK) return rc;
  launch_of(kFormats[codec])(c->stream, codec, s, j);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(c, MI_RGB_ERR_HIP, "the launch of %s failed: %s", kFormats[codec].name, hipGetErrorString(e));
  return c->time.end(c, c->stream);
}

// a slot no launch reads any more, at the back of the queue: the oldest if its launch is over (or if kMaxSlots are in
// flight: after waiting for it), else a new one
int free_slot(mi_rgb_ctx* c, PaletteSlot** out) {
  if (!c->slots.empty()) {
    PaletteSlot& old = c->slots.front();
    bool over = !old.used;
    if (!over) {
      const hipError_t q = hipEventQuery(old.done);
      if (q == hipSuccess) over = true;
      else if (q != hipErrorNotReady) return fail(c, MI_RGB_ERR_HIP, "hipEventQuery failed: %s", hipGetErrorString(q));
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
      return MI_RGB_OK;
    }
  }
  PaletteSlot fresh;
  HIPCHK(c, hipEventCreateWithFlags(&fresh.done.p, hipEventDisableTiming));
  c->slots.push_back(std::move(fresh));
  *out = &c->slots.back();
  return MI_RGB_OK;
}

// the palettes of a call into a slot and on their way to the device; the job gets the device pointers.  The checks are
// the caller's.
int stage_palettes(mi_rgb_ctx* c, const Format& f, const mi_rgb_color* palettes, int n_palettes, const uint16_t* palette_of, int n,
                   PaletteSlot** slot, Job* j) {
  int rc = free_slot(c, slot);
  if (rc != MI_RGB_OK) return rc;
  PaletteSlot& s = **slot;
  const size_t table = (size_t)n_palettes * 1024u, bytes = table + (palette_of ? (size_t)n * 2u : 0u);
  rc = s.h.grow(c, bytes, nullptr);  // (no launch uses the slot: nothing is waited for)
  if (rc == MI_RGB_OK) rc = s.d.grow(c, bytes, nullptr);
  if (rc != MI_RGB_OK) return rc;
  uint8_t* h = s.h;
  memset(h, 0, table);
  for (int k = 0; k < n_palettes; k++)
    for (uint32_t e = 0; e < f.palette; e++) {  // BGAV_PALETTE_2_RGB24, avdec_private.h:122-125
      const mi_rgb_color& col = palettes[(size_t)k * f.palette + e];
      uint8_t* q = h + (size_t)k * 1024u + 4u * e;
      q[0] = (uint8_t)(col.r >> 8), q[1] = (uint8_t)(col.g >> 8), q[2] = (uint8_t)(col.b >> 8);
    }
  if (palette_of) memcpy(h + table, palette_of, (size_t)n * 2u);
  HIPCHK(c, hipMemcpyAsync(s.d, h, bytes, hipMemcpyHostToDevice, c->stream));
  j->d_palettes = (const uint32_t*)s.d.p;
  j->d_palette_of = palette_of ? (const uint16_t*)(s.d.p + table) : nullptr;
  return MI_RGB_OK;
}

// what both entry points check of their palettes, then the staged and timed launch
int check_palettes(mi_rgb_ctx* c, const char* who, const Format& f, const mi_rgb_color* palettes, int n_palettes,
                   const uint16_t* palette_of, int n) {
  if (!f.palette) {
    if (palettes || n_palettes || palette_of) return fail(c, MI_RGB_ERR_ARG, "%s: %s has no palette, and was given one", who, f.name);
    return MI_RGB_OK;
  }
  if (!palettes || n_palettes < 1)
    return fail(c, MI_RGB_ERR_ARG, "%s: %s needs a palette of %u entries, and was given none", who, f.name, f.palette);
  if (n_palettes > n) return fail(c, MI_RGB_ERR_ARG, "%s: %d palettes for %d packets; 1 to n", who, n_palettes, n);
  if (palette_of)
    for (int i = 0; i < n; i++)
      if (palette_of[i] >= n_palettes)
        return fail(c, MI_RGB_ERR_ARG, "%s: palette_of[%d] is palette index %u of %d palettes", who, i, (unsigned)palette_of[i], n_palettes);
  return MI_RGB_OK;
}
int staged_run(mi_rgb_ctx* c, int codec, const Shape& s, Job j, const mi_rgb_color* palettes, int n_palettes, const uint16_t* palette_of) {
  const Format& f = kFormats[codec];
  if (!f.palette) return run(c, codec, s, j);
  PaletteSlot* slot = nullptr;
  int rc = stage_palettes(c, f, palettes, n_palettes, palette_of, j.n, &slot, &j);
  if (rc == MI_RGB_OK) rc = run(c, codec, s, j);
  if (!slot) return rc;
  // whatever became of the launch, the copy may be queued: the slot is free when the stream has passed this point
  slot->used = true;
  const hipError_t e = hipEventRecord(slot->done, c->stream);
  if (e != hipSuccess && rc == MI_RGB_OK) return fail(c, MI_RGB_ERR_HIP, "hipEventRecord failed: %s", hipGetErrorString(e));
  return rc;
}

uint64_t up16(uint64_t x) { return (x + 15u) & ~(uint64_t)15u; }
}  // namespace

extern "C" {

int mi_rgb_device_count(void) { return device_count(); }

const char* mi_rgb_last_error(const mi_rgb_ctx* c) { return last_error(c); }

mi_rgb_ctx* mi_rgb_create(int device) {
  if ((device = usable_device(device, "raw RGB unpacker", MI_RGB_ERR_ARG)) < 0) return nullptr;
  mi_rgb_ctx* c = new mi_rgb_ctx();
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream.p, hipStreamNonBlocking) != hipSuccess) {
    fail(nullptr, MI_RGB_ERR_HIP, "cannot set up device %d: %s", device, hipGetErrorString(hipGetLastError()));
    mi_rgb_destroy(c);
    return nullptr;
  }
  return c;
}

void mi_rgb_destroy(mi_rgb_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  delete c;
}

void* mi_rgb_dev_alloc(mi_rgb_ctx* c, size_t bytes) {
  if (!c) return nullptr;
  void* d = nullptr;
  if (hipSetDevice(c->device) != hipSuccess || hipMalloc(&d, bytes ? bytes : 1) != hipSuccess) {
    fail(c, MI_RGB_ERR_NOMEM, "hipMalloc(%zu) failed", bytes);
    return nullptr;
  }
  return d;
}
void mi_rgb_dev_free(mi_rgb_ctx* c, void* d) { dev_free(c, d); }
int mi_rgb_h2d(mi_rgb_ctx* c, void* d, const void* h, size_t n) {
  if (!c || (!d && n) || (!h && n)) return fail(c, MI_RGB_ERR_ARG, "mi_rgb_h2d: NULL argument");
  return copy_sync(c, d, h, n, hipMemcpyHostToDevice);
}
int mi_rgb_d2h(mi_rgb_ctx* c, void* h, const void* d, size_t n) {
  if (!c || (!d && n) || (!h && n)) return fail(c, MI_RGB_ERR_ARG, "mi_rgb_d2h: NULL argument");
  return copy_sync(c, h, d, n, hipMemcpyDeviceToHost);
}
int mi_rgb_sync(mi_rgb_ctx* c) { return c ? stream_sync(c) : MI_RGB_ERR_ARG; }

int mi_rgb_codec_of(uint32_t fourcc, int depth, int has_palette) {
  if (fourcc == miyuv::fourcc('r', 'a', 'w', ' ')) {  // video_qtraw.c:236-364
    switch (depth) {
      case 1: return has_palette ? kQt1 : -1;
      case 2: return has_palette ? kQt2 : -1;
      case 4: return has_palette ? kQt4 : -1;  // (:276 is inverted upstream: include/mi_rgb.h)
      case 8: return has_palette ? kQt8 : -1;
      case 16: return kQt16;
      case 24: return kQt24;
      case 32: return kQt32;
      case 34: return kQt2;
      case 36: return kQt4;
      case 40: return kQt8;
      default: return -1;
    }
  }
  const bool mtv = fourcc == miyuv::fourcc('M', 'T', 'V', ' ');
  if (mtv || fourcc == miyuv::fourcc('R', 'G', 'B', ' ') || fourcc == miyuv::fourcc('R', 'G', 'B', '3')) {  // video_aviraw.c:211-271
    switch (depth) {
      case 8: return has_palette ? kAvi8 : kAvi8Gray;
      case 16: return mtv ? kMtv16 : kAvi16;
      case 24: return kAvi24;
      case 32: return kAvi32;
      default: return -1;
    }
  }
  return -1;
}

int mi_rgb_layout_of(int codec, int w, int h, mi_rgb_layout* out) {
  if (!out) return fail(nullptr, MI_RGB_ERR_ARG, "mi_rgb_layout_of: NULL argument");
  Shape s;
  const int rc = checked_shape(nullptr, "mi_rgb_layout_of", codec, w, h, &s);
  if (rc != MI_RGB_OK) return rc;
  const Format& f = kFormats[codec];
  memset(out, 0, sizeof *out);
  out->packet_bytes = (int64_t)s.packet_bytes, out->picture_bytes = (int64_t)s.picture_bytes;
  out->packet_stride = (int32_t)s.in_stride, out->bytes_per_pixel = (int32_t)f.bpp;
  out->palette_entries = (int32_t)f.palette, out->bottom_up = f.bottom_up;
  return MI_RGB_OK;
}

int mi_rgb_unpack_batch(mi_rgb_ctx* c, int codec, int w, int h, const void* d_packets, size_t packet_stride, int n, void* d_pics,
                        size_t pic_stride, const mi_rgb_color* palettes, int n_palettes, const uint16_t* palette_of) {
  const char* who = "mi_rgb_unpack_batch";
  if (!c || !d_packets || !d_pics) return fail(c, MI_RGB_ERR_ARG, "%s: NULL argument", who);
  Shape s;
  int rc = checked_shape(c, who, codec, w, h, &s);
  if (rc != MI_RGB_OK) return rc;
  if (n < 1 || n > 65535) return fail(c, MI_RGB_ERR_ARG, "%s: %d packets; 1 to 65535 per call (split the batch)", who, n);
  if (((uintptr_t)d_packets | (uintptr_t)d_pics | packet_stride | pic_stride) & 15u)
    return fail(c, MI_RGB_ERR_ARG, "%s: d_packets, d_pics, packet_stride and pic_stride must be 16-byte aligned", who);
  if (packet_stride < s.packet_bytes || pic_stride < s.picture_bytes)
    return fail(c, MI_RGB_ERR_ARG, "%s: strides of %zu and %zu bytes; %s at %d x %d has packets of %llu and pictures of %llu", who,
                packet_stride, pic_stride, kFormats[codec].name, w, h, (unsigned long long)s.packet_bytes,
                (unsigned long long)s.picture_bytes);
  const uintptr_t p0 = (uintptr_t)d_packets, p1 = p0 + (size_t)(n - 1) * packet_stride + (size_t)s.packet_bytes;
  const uintptr_t q0 = (uintptr_t)d_pics, q1 = q0 + (size_t)(n - 1) * pic_stride + (size_t)s.picture_bytes;
  if (p0 < q1 && q0 < p1) return fail(c, MI_RGB_ERR_ARG, "%s: d_packets overlaps d_pics", who);
  rc = check_palettes(c, who, kFormats[codec], palettes, n_palettes, palette_of, n);
  if (rc != MI_RGB_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const Job j = {(const uint8_t*)d_packets, (uint64_t)packet_stride, n, (uint8_t*)d_pics, (uint64_t)pic_stride, nullptr, nullptr};
  return staged_run(c, codec, s, j, palettes, n_palettes, palette_of);
}

int mi_rgb_unpack_frame(mi_rgb_ctx* c, int codec, int w, int h, const uint8_t* packet, size_t len, const mi_rgb_color* palette,
                        uint8_t* plane, int stride) {
  const char* who = "mi_rgb_unpack_frame";
  if (!c) return fail(c, MI_RGB_ERR_ARG, "%s: NULL argument", who);
  Shape s;
  int rc = checked_shape(c, who, codec, w, h, &s);
  if (rc != MI_RGB_OK) return rc;
  if (!plane) return fail(c, MI_RGB_ERR_ARG, "%s: NULL argument", who);
  if (stride < 0 || (uint32_t)stride < s.row_bytes)
    return fail(c, MI_RGB_ERR_ARG, "%s: a stride of %d is below the picture's row of %u bytes", who, stride, s.row_bytes);
  rc = check_palettes(c, who, kFormats[codec], palette, palette ? 1 : 0, nullptr, 1);
  if (rc != MI_RGB_OK) return rc;
  if (len == 0) return MI_RGB_OK;  // lib/video_aviraw.c:160-161
  if (!packet) return fail(c, MI_RGB_ERR_ARG, "%s: NULL argument", who);
  if (len < s.packet_bytes)
    return fail(c, MI_RGB_ERR_FORMAT, "%s: a packet of %zu bytes; %s at %d x %d has %llu", who, len, kFormats[codec].name, w, h,
                (unsigned long long)s.packet_bytes);
  HIPCHK(c, hipSetDevice(c->device));
  // (the stream is idle between these calls: nothing is waited for)
  rc = c->d_packet.grow(c, up16(s.packet_bytes), nullptr);
  if (rc == MI_RGB_OK) rc = c->d_pic.grow(c, up16(s.picture_bytes), nullptr);
  if (rc == MI_RGB_OK) rc = c->h_pic.grow(c, s.picture_bytes, nullptr);
  if (rc != MI_RGB_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(c->d_packet, packet, (size_t)s.packet_bytes, hipMemcpyHostToDevice, c->stream));
  const Job j = {c->d_packet, up16(s.packet_bytes), 1, c->d_pic, up16(s.picture_bytes), nullptr, nullptr};
  rc = staged_run(c, codec, s, j, palette, palette ? 1 : 0, nullptr);
  if (rc != MI_RGB_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(c->h_pic, c->d_pic, (size_t)s.picture_bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint8_t* tight = c->h_pic;
  for (uint32_t y = 0; y < s.h; y++, tight += s.row_bytes) memcpy(plane + (size_t)y * (size_t)stride, tight, s.row_bytes);
  return MI_RGB_OK;
}

int mi_rgb_times(mi_rgb_ctx* c, float* total_ms, int* launches) {
  return times(c, c ? &c->time : nullptr, 1, total_ms, launches, MI_RGB_ERR_ARG);
}

}  // extern "C"
