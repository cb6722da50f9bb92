// mi_yuv.hip — C ABI (include/mi_yuv.h) of the MI355X unpacker of the uncompressed QuickTime YUV family.  No CPU path:
// without a gfx950 device every call but the three host-only queries fails with a message.  The kernels and the format
// table: yuv_unpack_kernels.h.  Owned memory, errors, the event timer and the bodies of the calls every device library
// has: host_base.h.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/mi_yuv.h"
#include "host_base.h"
#include "yuv_unpack_kernels.h"

using namespace miyuv;

static_assert(kYuv2 == MI_YUV_YUV2 && k2vuy == MI_YUV_2VUY && kYv12Lower == MI_YUV_YV12_LOWER && kYv12Upper == MI_YUV_YV12_UPPER &&
                  kVyuy == MI_YUV_VYUY && kYvu9 == MI_YUV_YVU9 && kV308 == MI_YUV_V308 && kV408 == MI_YUV_V408 &&
                  kV410 == MI_YUV_V410 && kV210 == MI_YUV_V210 && kYuv4 == MI_YUV_YUV4 && kCodecs == MI_YUV_CODECS,
              "header and kernels agree");
static_assert(MI_YUV_OK == kOk && MI_YUV_ERR_HIP == kErrHip, "header and host base agree");

// Device, stream and error text are HostCtx's (host_base.h), destroyed after everything here; the timer goes before
// the pool it hands its pairs to.
struct __attribute__((visibility("hidden"))) mi_yuv_ctx : HostCtx {
  EventPool ev_free;
  Timer time{ev_free};  // the unpack launches (mi_yuv_times)
  // mi_yuv_unpack_frame's staging: one packet and one picture on the device, the picture in pinned memory; they only grow
  DevBuf<uint8_t> d_packet, d_pic;
  PinnedBuf<uint8_t> h_pic;
};

namespace {
// a codec and a size, checked against the format table: the shape, or a message that names the rule
int checked_shape(mi_yuv_ctx* c, const char* who, int codec, int w, int h, Shape* s) {
  if (codec < 0 || codec >= kCodecs) return fail(c, MI_YUV_ERR_ARG, "%s: unknown codec %d", who, codec);
  const Format& f = kFormats[codec];
  if (w <= 0 || h <= 0) return fail(c, MI_YUV_ERR_ARG, "%s: %s at %d x %d: width and height are positive", who, f.name, w, h);
  if ((uint32_t)w % f.w_mult || (uint32_t)h % f.h_mult)
    return fail(c, MI_YUV_ERR_ARG, "%s: %s at %d x %d: the width is a multiple of %u and the height a multiple of %u", who,
                f.name, w, h, f.w_mult, f.h_mult);
  const bool fits = (uint64_t)w * (uint64_t)h < (1ull << 31);  // (no packet has less than a byte a pixel)
  *s = shape_of(codec, fits ? (uint64_t)w : 65536u, fits ? (uint64_t)h : 32768u);
  if (s->packet_bytes >= (1ull << 31) || s->picture_bytes >= (1ull << 31))
    return fail(c, MI_YUV_ERR_ARG, "%s: %s at %d x %d: packets and pictures stay below 2^31 bytes", who, f.name, w, h);
  return MI_YUV_OK;
}

// ---- the launches; checks, events and errors are their caller's ----
dim3 grid_for(uint32_t items, int n) {
  const uint32_t gx = (items + kThreads - 1u) / kThreads;
  return dim3(gx < kMaxGridX ? gx : kMaxGridX, (unsigned)n);
}
template <class C>
void unpack_launch(hipStream_t st, const Shape& s, const uint8_t* packets, uint64_t ps, int n, uint8_t* pics, uint64_t qs) {
  const Geo g = unpack_geo<C>(s);
  hipLaunchKernelGGL(k_yuv_unpack<C>, grid_for(g.items, n), dim3(kThreads), 0, st, packets, ps, pics, qs, g);
}
void move_launch(hipStream_t st, const Shape& s, const uint8_t* packets, uint64_t ps, int n, uint8_t* pics, uint64_t qs) {
  const MoveGeo g = move_geo(s);
  hipLaunchKernelGGL(k_yuv_move, grid_for(g.items, n), dim3(kThreads), 0, st, packets, ps, pics, qs, g);
}
using Launch = void (*)(hipStream_t, const Shape&, const uint8_t*, uint64_t, int, uint8_t*, uint64_t);
constexpr Launch kLaunch[kCodecs] = {unpack_launch<Yuv2>, move_launch, move_launch,         move_launch,
                                     move_launch,         move_launch, unpack_launch<V308>, unpack_launch<V408>,
                                     unpack_launch<V410>, unpack_launch<V210>, unpack_launch<Yuv4>};
constexpr bool launches_agree() {
  for (int i = 0; i < kCodecs; i++)
    if ((kLaunch[i] == move_launch) != kFormats[i].moves) return false;
  return true;
}
static_assert(launches_agree(), "the plane mover has the codecs the format table gives it");

// the checked launch over n resident packets, timed (a launch that fails leaves the timer's pair open: it goes back to
// the pool at the next begin())
int run(mi_yuv_ctx* c, int codec, const Shape& s, const void* d_packets, size_t packet_stride, int n, void* d_pics, size_t pic_stride) {
  const int rc = c->time.begin(c, c->stream);
  if (rc != MI_YUV_OK) return rc;
  kLaunch[codec](c->stream, s, (const uint8_t*)d_packets, (uint64_t)packet_stride, n, (uint8_t*)d_pics, (uint64_t)pic_stride);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(c, MI_YUV_ERR_HIP, "the launch of %s failed: %s", kFormats[codec].name, hipGetErrorString(e));
  return c->time.end(c, c->stream);
}

uint64_t up16(uint64_t x) { return (x + 15u) & ~(uint64_t)15u; }
}  // namespace

extern "C" {

int mi_yuv_device_count(void) { return device_count(); }

const char* mi_yuv_last_error(const mi_yuv_ctx* c) { return last_error(c); }

mi_yuv_ctx* mi_yuv_create(int device) {
  if ((device = usable_device(device, "YUV unpacker", MI_YUV_ERR_ARG)) < 0) return nullptr;
  mi_yuv_ctx* c = new mi_yuv_ctx();
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream.p, hipStreamNonBlocking) != hipSuccess) {
    fail(nullptr, MI_YUV_ERR_HIP, "cannot set up device %d: %s", device, hipGetErrorString(hipGetLastError()));
    mi_yuv_destroy(c);
    return nullptr;
  }
  return c;
}

void mi_yuv_destroy(mi_yuv_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  delete c;
}

void* mi_yuv_dev_alloc(mi_yuv_ctx* c, size_t bytes) {
  if (!c) return nullptr;
  void* d = nullptr;
  if (hipSetDevice(c->device) != hipSuccess || hipMalloc(&d, bytes ? bytes : 1) != hipSuccess) {
    fail(c, MI_YUV_ERR_NOMEM, "hipMalloc(%zu) failed", bytes);
    return nullptr;
  }
  return d;
}
void mi_yuv_dev_free(mi_yuv_ctx* c, void* d) { dev_free(c, d); }
int mi_yuv_h2d(mi_yuv_ctx* c, void* d, const void* h, size_t n) {
  if (!c || (!d && n) || (!h && n)) return fail(c, MI_YUV_ERR_ARG, "mi_yuv_h2d: NULL argument");
  return copy_sync(c, d, h, n, hipMemcpyHostToDevice);
}
int mi_yuv_d2h(mi_yuv_ctx* c, void* h, const void* d, size_t n) {
  if (!c || (!d && n) || (!h && n)) return fail(c, MI_YUV_ERR_ARG, "mi_yuv_d2h: NULL argument");
  return copy_sync(c, h, d, n, hipMemcpyDeviceToHost);
}
int mi_yuv_sync(mi_yuv_ctx* c) { return c ? stream_sync(c) : MI_YUV_ERR_ARG; }

int mi_yuv_codec_of(uint32_t fourcc) {  // the first decoder registered for a fourcc wins: '2vuy' is the UYVY one's
  for (int i = 0; i < kCodecs; i++)
    if (kFormats[i].fourcc == fourcc) return i;
  return -1;
}

int mi_yuv_layout_of(int codec, int w, int h, mi_yuv_layout* layout) {
  if (!layout) return fail(nullptr, MI_YUV_ERR_ARG, "mi_yuv_layout_of: NULL argument");
  Shape s;
  const int rc = checked_shape(nullptr, "mi_yuv_layout_of", codec, w, h, &s);
  if (rc != MI_YUV_OK) return rc;
  memset(layout, 0, sizeof *layout);
  layout->packet_bytes = (int64_t)s.packet_bytes, layout->picture_bytes = (int64_t)s.picture_bytes;
  layout->planes = (int32_t)s.planes;
  const bool planar_packet = kFormats[codec].moves && s.planes == 3;
  for (uint32_t p = 0; p < s.planes; p++) {
    layout->plane_w[p] = (int32_t)s.w[p], layout->plane_h[p] = (int32_t)s.h[p], layout->plane_bps[p] = (int32_t)s.bps[p];
    if (p == 0 || planar_packet) layout->packet_strides[p] = (int32_t)s.src_stride[p];
  }
  return MI_YUV_OK;
}

int mi_yuv_alpha_v408(uint8_t out[256]) {
  if (!out) return fail(nullptr, MI_YUV_ERR_ARG, "mi_yuv_alpha_v408: NULL argument");
  for (uint32_t x = 0; x < 256; x++) out[x] = (uint8_t)alpha_v408(x);
  return MI_YUV_OK;
}

int mi_yuv_unpack_batch(mi_yuv_ctx* c, int codec, int w, int h, const void* d_packets, size_t packet_stride, int n, void* d_pics,
                        size_t pic_stride) {
  const char* who = "mi_yuv_unpack_batch";
  if (!c || !d_packets || !d_pics) return fail(c, MI_YUV_ERR_ARG, "%s: NULL argument", who);
  Shape s;
  const int rc = checked_shape(c, who, codec, w, h, &s);
  if (rc != MI_YUV_OK) return rc;
  if (n < 1 || n > 65535) return fail(c, MI_YUV_ERR_ARG, "%s: %d packets; 1 to 65535 per call (split the batch)", who, n);
  if (((uintptr_t)d_packets | (uintptr_t)d_pics | packet_stride | pic_stride) & 15u)
    return fail(c, MI_YUV_ERR_ARG, "%s: d_packets, d_pics, packet_stride and pic_stride must be 16-byte aligned", who);
  if (packet_stride < s.packet_bytes || pic_stride < s.picture_bytes)
    return fail(c, MI_YUV_ERR_ARG, "%s: strides of %zu and %zu bytes; %s at %d x %d has packets of %llu and pictures of %llu", who,
                packet_stride, pic_stride, kFormats[codec].name, w, h, (unsigned long long)s.packet_bytes,
                (unsigned long long)s.picture_bytes);
  const uintptr_t p0 = (uintptr_t)d_packets, p1 = p0 + (size_t)(n - 1) * packet_stride + (size_t)s.packet_bytes;
  const uintptr_t q0 = (uintptr_t)d_pics, q1 = q0 + (size_t)(n - 1) * pic_stride + (size_t)s.picture_bytes;
  if (p0 < q1 && q0 < p1) return fail(c, MI_YUV_ERR_ARG, "%s: d_packets overlaps d_pics", who);
  HIPCHK(c, hipSetDevice(c->device));
  return run(c, codec, s, d_packets, packet_stride, n, d_pics, pic_stride);
}

int mi_yuv_unpack_frame(mi_yuv_ctx* c, int codec, int w, int h, const uint8_t* packet, size_t len, uint8_t* const planes[3],
                        const int strides[3]) {
  const char* who = "mi_yuv_unpack_frame";
  if (!c) return fail(c, MI_YUV_ERR_ARG, "%s: NULL argument", who);
  Shape s;
  int rc = checked_shape(c, who, codec, w, h, &s);
  if (rc != MI_YUV_OK) return rc;
  if (!planes || !strides) return fail(c, MI_YUV_ERR_ARG, "%s: NULL argument", who);
  for (uint32_t p = 0; p < s.planes; p++) {
    if (!planes[p]) return fail(c, MI_YUV_ERR_ARG, "%s: plane %u is NULL", who, p);
    if (strides[p] < 0 || (uint64_t)strides[p] < (uint64_t)s.w[p] * s.bps[p])
      return fail(c, MI_YUV_ERR_ARG, "%s: stride %d of plane %u is below its row of %u bytes", who, strides[p], p, s.w[p] * s.bps[p]);
  }
  if (len == 0) return MI_YUV_OK;  // lib/video_yuv.c:623-624
  if (!packet) return fail(c, MI_YUV_ERR_ARG, "%s: NULL argument", who);
  if (len < s.packet_bytes)
    return fail(c, MI_YUV_ERR_FORMAT, "%s: a packet of %zu bytes; %s at %d x %d has %llu", who, len, kFormats[codec].name, w, h,
                (unsigned long long)s.packet_bytes);
  HIPCHK(c, hipSetDevice(c->device));
  // (the stream is idle between these calls: nothing is waited for)
  rc = c->d_packet.grow(c, up16(s.packet_bytes), nullptr);
  if (rc == MI_YUV_OK) rc = c->d_pic.grow(c, up16(s.picture_bytes), nullptr);
  if (rc == MI_YUV_OK) rc = c->h_pic.grow(c, s.picture_bytes, nullptr);
  if (rc != MI_YUV_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(c->d_packet, packet, (size_t)s.packet_bytes, hipMemcpyHostToDevice, c->stream));
  rc = run(c, codec, s, c->d_packet, (size_t)up16(s.packet_bytes), 1, c->d_pic, (size_t)up16(s.picture_bytes));
  if (rc != MI_YUV_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(c->h_pic, c->d_pic, (size_t)s.picture_bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint8_t* tight = c->h_pic;
  for (uint32_t p = 0; p < s.planes; p++) {
    const size_t row = (size_t)s.w[p] * s.bps[p];
    for (uint32_t y = 0; y < s.h[p]; y++, tight += row) memcpy(planes[p] + (size_t)y * (size_t)strides[p], tight, row);
  }
  return MI_YUV_OK;
}

int mi_yuv_times(mi_yuv_ctx* c, float* total_ms, int* launches) {
  return times(c, c ? &c->time : nullptr, 1, total_ms, launches, MI_YUV_ERR_ARG);
}

}  // extern "C"
