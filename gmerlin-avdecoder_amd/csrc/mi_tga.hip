// mi_tga.hip — C ABI (include/mi_tga.h) of the MI355X decoder of Targa packets.  No CPU path: without a gfx950 device every
// call but the two host-only ones fails with a message.  The header parser: tga_format.h; the kernels: tga_kernels.h.
// Owned memory, errors, the event timer and the bodies of the calls every device library has: host_base.h.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/mi_tga.h"
#include "host_base.h"
#include "tga_kernels.h"

using namespace mitga;

static_assert(MI_TGA_OK == kOk && MI_TGA_ERR_HIP == kErrHip, "header and host base agree");

namespace {
// What one call brings from the host: offsets, lengths, palette_of and the palettes reduced to 4 bytes an entry, in
// pinned memory and on the device.  A call takes a slot whose last call is over (`done`), so it never touches what a
// queued launch still reads.
struct CallSlot {
  PinnedBuf<uint8_t> h;
  DevBuf<uint8_t> d;
  Event done;
  bool used = false;
};
constexpr size_t kMaxSlots = 64;  // with this many calls in flight a call waits for the oldest
uint64_t up16(uint64_t x) { return (x + 15u) & ~(uint64_t)15u; }
}  // namespace

// Device, stream and error text are HostCtx's (host_base.h), destroyed after everything here; the timers go before the
// pool they hand their pairs to.
struct __attribute__((visibility("hidden"))) mi_tga_ctx : HostCtx {
  EventPool ev_free;
  Timer t_scan{ev_free}, t_index{ev_free}, t_expand{ev_free};  // mi_tga_times
  std::deque<CallSlot> slots;  // oldest call first
  // the descriptors and the checkpoints of a call: launches of one stream use them one after the other; they only grow
  DevBuf<mi_tga_info> d_info;
  DevBuf<uint2> d_index;
  // mi_tga_decode_frame's staging: one packet, one picture and one status on the device, picture and status in pinned memory
  DevBuf<uint8_t> d_packet, d_pic;
  PinnedBuf<uint8_t> h_pic;
};

namespace {
// a slot no launch reads any more, at the back of the queue: the oldest if its call is over (or if kMaxSlots are in
// flight: after waiting for it), else a new one
int free_slot(mi_tga_ctx* c, CallSlot** out) {
  if (!c->slots.empty()) {
    CallSlot& old = c->slots.front();
    bool over = !old.used;
    if (!over) {
      const hipError_t q = hipEventQuery(old.done);
      if (q == hipSuccess) over = true;
      else if (q != hipErrorNotReady) return fail(c, MI_TGA_ERR_HIP, "hipEventQuery failed: %s", hipGetErrorString(q));
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
      return MI_TGA_OK;
    }
  }
  CallSlot fresh;
  HIPCHK(c, hipEventCreateWithFlags(&fresh.done.p, hipEventDisableTiming));
  c->slots.push_back(std::move(fresh));
  *out = &c->slots.back();
  return MI_TGA_OK;
}

struct Job {
  const uint8_t* stream;
  const uint64_t* offsets;
  const uint32_t* lengths;
  int n, w, h, format;
  uint8_t* pics;
  uint64_t pic_stride;
  const mi_tga_color* palettes;
  int palette_entries, n_palettes;
  const uint16_t* palette_of;
  int32_t* status;
};

template <class K>
int timed(mi_tga_ctx* c, Timer& t, const char* name, K launch) {
  int rc = t.begin(c, c->stream);
  if (rc != MI_TGA_OK) return rc;
  launch();
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(c, MI_TGA_ERR_HIP, "the launch of %s failed: %s", name, hipGetErrorString(e));
  return t.end(c, c->stream);
}

// the call's host arrays into the slot and on their way to the device, then the three launches; the checks are the caller's
int stage_and_launch(mi_tga_ctx* c, const Job& j, CallSlot& s) {
  const size_t n = (size_t)j.n;
  const uint32_t pal_entries = j.palettes ? (j.palette_entries < 256 ? (uint32_t)j.palette_entries : 256u) : 0u;
  const size_t o_len = 8u * n, o_of = 12u * n, o_pal = up16(14u * n), bytes = o_pal + (size_t)j.n_palettes * pal_entries * 4u;
  int rc = s.h.grow(c, bytes, nullptr);  // (no launch uses the slot: nothing is waited for)
  if (rc == MI_TGA_OK) rc = s.d.grow(c, bytes, nullptr);
  const uint32_t npix = (uint32_t)j.w * (uint32_t)j.h, tiles = (npix + kTile - 1u) / kTile;
  if (rc == MI_TGA_OK) rc = c->d_info.grow(c, n, c->stream);
  if (rc == MI_TGA_OK) rc = c->d_index.grow(c, (uint64_t)n * tiles, c->stream);
  if (rc != MI_TGA_OK) return rc;
  uint8_t* h = s.h;
  memcpy(h, j.offsets, 8u * n);
  memcpy(h + o_len, j.lengths, 4u * n);
  if (j.palette_of) memcpy(h + o_of, j.palette_of, 2u * n);
  for (int k = 0; k < j.n_palettes; k++)
    for (uint32_t e = 0; e < pal_entries; e++) {  // V:111-117
      const mi_tga_color& col = j.palettes[(size_t)k * (size_t)j.palette_entries + e];
      uint8_t* q = h + o_pal + ((size_t)k * pal_entries + e) * 4u;
      q[0] = (uint8_t)(col.r >> 8), q[1] = (uint8_t)(col.g >> 8), q[2] = (uint8_t)(col.b >> 8), q[3] = (uint8_t)(col.a >> 8);
    }
  HIPCHK(c, hipMemcpyAsync(s.d, h, bytes, hipMemcpyHostToDevice, c->stream));
  Call k;
  k.stream = j.stream, k.offsets = (const uint64_t*)s.d.p, k.lengths = (const uint32_t*)(s.d.p + o_len);
  k.n = (uint32_t)j.n, k.w = (uint32_t)j.w, k.h = (uint32_t)j.h, k.format = (uint32_t)j.format;
  k.palette_entries = j.palettes ? (uint32_t)j.palette_entries : 0u;
  k.info = c->d_info, k.status = j.status, k.index = c->d_index, k.tiles = tiles;
  k.pics = j.pics, k.pic_stride = j.pic_stride;
  k.palettes = j.palettes ? s.d.p + o_pal : nullptr, k.pal_entries = pal_entries;
  k.palette_of = j.palette_of ? (const uint16_t*)(s.d.p + o_of) : nullptr;
  hipStream_t st = c->stream;
  rc = timed(c, c->t_scan, "k_tga_scan", [&] { hipLaunchKernelGGL(k_tga_scan, dim3((k.n + 63u) / 64u), dim3(64), 0, st, k); });
  if (rc == MI_TGA_OK)
    rc = timed(c, c->t_index, "k_tga_index", [&] { hipLaunchKernelGGL(k_tga_index, dim3(k.n), dim3(64), 0, st, k); });
  if (rc == MI_TGA_OK)
    rc = timed(c, c->t_expand, "k_tga_expand", [&] {
      const dim3 grid(tiles, k.n), block(kThreads);
      switch (j.format) {
        case MI_TGA_GRAY8: hipLaunchKernelGGL(k_tga_expand<1u>, grid, block, 0, st, k); break;
        case MI_TGA_RGB15: hipLaunchKernelGGL(k_tga_expand<2u>, grid, block, 0, st, k); break;
        case MI_TGA_BGR24: hipLaunchKernelGGL(k_tga_expand<3u>, grid, block, 0, st, k); break;
        default: hipLaunchKernelGGL(k_tga_expand<4u>, grid, block, 0, st, k); break;
      }
    });
  return rc;
}

int run(mi_tga_ctx* c, const Job& j) {
  CallSlot* slot = nullptr;
  int rc = free_slot(c, &slot);
  if (rc != MI_TGA_OK) return rc;
  rc = stage_and_launch(c, j, *slot);
  // whatever became of the launches, the copy may be queued: the slot is free when the stream has passed this point
  slot->used = true;
  const hipError_t e = hipEventRecord(slot->done, c->stream);
  if (e != hipSuccess && rc == MI_TGA_OK) return fail(c, MI_TGA_ERR_HIP, "hipEventRecord failed: %s", hipGetErrorString(e));
  return rc;
}

// what both entry points check of a size, a format and the palettes
int check_common(mi_tga_ctx* c, const char* who, int w, int h, int format, const mi_tga_color* palettes, int palette_entries,
                 int n_palettes, const uint16_t* palette_of, int n) {
  if (w < 1 || w > 65535 || h < 1 || h > 65535) return fail(c, MI_TGA_ERR_ARG, "%s: %d x %d: width and height are 1 to 65535", who, w, h);
  if (format < 0 || format >= MI_TGA_FORMATS) return fail(c, MI_TGA_ERR_ARG, "%s: unknown format %d", who, format);
  if ((uint64_t)w * (uint64_t)h * (uint64_t)(format + 1) >= (1ull << 31))
    return fail(c, MI_TGA_ERR_ARG, "%s: %d x %d at %d bytes a pixel: pictures stay below 2^31 bytes", who, w, h, format + 1);
  if (!palettes) {
    if (palette_entries || n_palettes || palette_of)
      return fail(c, MI_TGA_ERR_ARG, "%s: without palettes, palette_entries and n_palettes are 0 and palette_of is NULL", who);
    return MI_TGA_OK;
  }
  if (palette_entries < 1 || palette_entries > 65535)
    return fail(c, MI_TGA_ERR_ARG, "%s: palettes of %d entries; 1 to 65535", who, palette_entries);
  if (n_palettes < 1 || n_palettes > n) return fail(c, MI_TGA_ERR_ARG, "%s: %d palettes for %d packets; 1 to n", who, n_palettes, n);
  if (palette_of)
    for (int i = 0; i < n; i++)
      if (palette_of[i] >= n_palettes)
        return fail(c, MI_TGA_ERR_ARG, "%s: palette_of[%d] is palette index %u of %d palettes", who, i, (unsigned)palette_of[i], n_palettes);
  return MI_TGA_OK;
}
}  // namespace

extern "C" {

int mi_tga_device_count(void) { return device_count(); }

const char* mi_tga_last_error(const mi_tga_ctx* c) { return last_error(c); }

mi_tga_ctx* mi_tga_create(int device) {
  if ((device = usable_device(device, "Targa decoder", MI_TGA_ERR_ARG)) < 0) return nullptr;
  mi_tga_ctx* c = new mi_tga_ctx();
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream.p, hipStreamNonBlocking) != hipSuccess) {
    fail(nullptr, MI_TGA_ERR_HIP, "cannot set up device %d: %s", device, hipGetErrorString(hipGetLastError()));
    mi_tga_destroy(c);
    return nullptr;
  }
  return c;
}

void mi_tga_destroy(mi_tga_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  delete c;
}

void* mi_tga_dev_alloc(mi_tga_ctx* c, size_t bytes) {
  if (!c) return nullptr;
  void* d = nullptr;
  if (hipSetDevice(c->device) != hipSuccess || hipMalloc(&d, bytes ? bytes : 1) != hipSuccess) {
    fail(c, MI_TGA_ERR_NOMEM, "hipMalloc(%zu) failed", bytes);
    return nullptr;
  }
  return d;
}
void mi_tga_dev_free(mi_tga_ctx* c, void* d) { dev_free(c, d); }
int mi_tga_h2d(mi_tga_ctx* c, void* d, const void* h, size_t n) {
  if (!c || (!d && n) || (!h && n)) return fail(c, MI_TGA_ERR_ARG, "mi_tga_h2d: NULL argument");
  return copy_sync(c, d, h, n, hipMemcpyHostToDevice);
}
int mi_tga_d2h(mi_tga_ctx* c, void* h, const void* d, size_t n) {
  if (!c || (!d && n) || (!h && n)) return fail(c, MI_TGA_ERR_ARG, "mi_tga_d2h: NULL argument");
  return copy_sync(c, h, d, n, hipMemcpyDeviceToHost);
}
int mi_tga_sync(mi_tga_ctx* c) { return c ? stream_sync(c) : MI_TGA_ERR_ARG; }

int mi_tga_parse(const uint8_t* pkt, size_t len, int palette_entries, mi_tga_info* info) {
  if (!info || (!pkt && len) || palette_entries < 0 || palette_entries > 65535) {
    fail(nullptr, MI_TGA_ERR_ARG, "mi_tga_parse: NULL argument, or a palette of %d entries", palette_entries);
    return MI_TGA_ERR_ARG;
  }
  return parse_header(pkt, (uint64_t)len, (uint32_t)palette_entries, info);
}

int mi_tga_tile_pixels(void) { return (int)kTile; }

int mi_tga_decode_batch(mi_tga_ctx* c, const void* d_stream, const uint64_t* offsets, const uint32_t* lengths, int n, int w, int h,
                        int format, void* d_pics, size_t pic_stride, const mi_tga_color* palettes, int palette_entries, int n_palettes,
                        const uint16_t* palette_of, int32_t* d_status) {
  const char* who = "mi_tga_decode_batch";
  if (!c || !d_stream || !offsets || !lengths || !d_pics || !d_status) return fail(c, MI_TGA_ERR_ARG, "%s: NULL argument", who);
  if (n < 1 || n > 65535) return fail(c, MI_TGA_ERR_ARG, "%s: %d packets; 1 to 65535 per call (split the batch)", who, n);
  int rc = check_common(c, who, w, h, format, palettes, palette_entries, n_palettes, palette_of, n);
  if (rc != MI_TGA_OK) return rc;
  const uint64_t picture = (uint64_t)w * (uint64_t)h * (uint64_t)(format + 1);
  if (((uintptr_t)d_pics | pic_stride) & 15u) return fail(c, MI_TGA_ERR_ARG, "%s: d_pics and pic_stride must be 16-byte aligned", who);
  if (pic_stride < picture)
    return fail(c, MI_TGA_ERR_ARG, "%s: a stride of %zu bytes; %d x %d at %d bytes a pixel has pictures of %llu", who, pic_stride, w, h,
                format + 1, (unsigned long long)picture);
  const uintptr_t s0 = (uintptr_t)d_stream, q0 = (uintptr_t)d_pics, q1 = q0 + (size_t)(n - 1) * pic_stride + (size_t)picture;
  const uintptr_t t0 = (uintptr_t)d_status, t1 = t0 + 4u * (size_t)n;
  if (t0 & 3u) return fail(c, MI_TGA_ERR_ARG, "%s: d_status must be 4-byte aligned", who);
  if (t0 < q1 && q0 < t1) return fail(c, MI_TGA_ERR_ARG, "%s: d_status overlaps d_pics", who);
  for (int i = 0; i < n; i++) {
    if (lengths[i] >= (1u << 31)) return fail(c, MI_TGA_ERR_ARG, "%s: packet %d has %u bytes; packets stay below 2^31 bytes", who, i, lengths[i]);
    const uintptr_t p0 = s0 + (uintptr_t)offsets[i], p1 = p0 + lengths[i];
    if (p0 < q1 && q0 < p1) return fail(c, MI_TGA_ERR_ARG, "%s: packet %d overlaps d_pics", who, i);
    if (p0 < t1 && t0 < p1) return fail(c, MI_TGA_ERR_ARG, "%s: packet %d overlaps d_status", who, i);
  }
  HIPCHK(c, hipSetDevice(c->device));
  const Job j = {(const uint8_t*)d_stream, offsets, lengths, n, w, h, format, (uint8_t*)d_pics, (uint64_t)pic_stride,
                 palettes, palette_entries, n_palettes, palette_of, d_status};
  return run(c, j);
}

int mi_tga_decode_frame(mi_tga_ctx* c, const uint8_t* pkt, size_t len, const mi_tga_color* palette, int palette_entries, uint8_t* plane,
                        int stride, mi_tga_info* info) {
  const char* who = "mi_tga_decode_frame";
  if (!c || !pkt || !plane || !info) return fail(c, MI_TGA_ERR_ARG, "%s: NULL argument", who);
  if (len >= (1ull << 31)) return fail(c, MI_TGA_ERR_ARG, "%s: a packet of %zu bytes; packets stay below 2^31 bytes", who, len);
  if (palette ? (palette_entries < 1 || palette_entries > 65535) : palette_entries != 0)
    return fail(c, MI_TGA_ERR_ARG, "%s: a palette of %d entries; 1 to 65535, and 0 without one", who, palette_entries);
  if (parse_header(pkt, (uint64_t)len, (uint32_t)palette_entries, info) != MI_TGA_ST_OK)
    return fail(c, MI_TGA_ERR_FORMAT, "%s: the header is refused with status %d", who, (int)info->status);
  const int w = info->width, h = info->height, format = info->format;
  int rc = check_common(c, who, w, h, format, palette, palette_entries, palette ? 1 : 0, nullptr, 1);
  if (rc != MI_TGA_OK) return rc;
  const uint32_t row = (uint32_t)w * (uint32_t)(format + 1);
  const uint64_t picture = (uint64_t)row * (uint64_t)h;
  if (stride < 0 || (uint32_t)stride < row)
    return fail(c, MI_TGA_ERR_ARG, "%s: a stride of %d is below the picture's row of %u bytes", who, stride, row);
  HIPCHK(c, hipSetDevice(c->device));
  // (the stream is idle between these calls: nothing is waited for).  The status lies behind the picture.
  rc = c->d_packet.grow(c, up16(len), nullptr);
  if (rc == MI_TGA_OK) rc = c->d_pic.grow(c, up16(picture) + 16u, nullptr);
  if (rc == MI_TGA_OK) rc = c->h_pic.grow(c, up16(picture) + 16u, nullptr);
  if (rc != MI_TGA_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(c->d_packet, pkt, len, hipMemcpyHostToDevice, c->stream));
  const uint64_t offset = 0;
  const uint32_t length = (uint32_t)len;
  int32_t* d_status = (int32_t*)(c->d_pic.p + up16(picture));
  const Job j = {c->d_packet, &offset, &length, 1, w, h, format, c->d_pic, up16(picture), palette, palette_entries, palette ? 1 : 0,
                 nullptr, d_status};
  rc = run(c, j);
  if (rc != MI_TGA_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(c->h_pic, c->d_pic, (size_t)up16(picture) + 16u, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int32_t st;
  memcpy(&st, c->h_pic.p + up16(picture), 4);
  if (st != MI_TGA_ST_OK) {
    info->status = st;
    return fail(c, MI_TGA_ERR_FORMAT, "%s: the packet is refused with status %d", who, (int)st);
  }
  const uint8_t* tight = c->h_pic;
  for (int y = 0; y < h; y++, tight += row) memcpy(plane + (size_t)y * (size_t)stride, tight, row);
  return MI_TGA_OK;
}

int mi_tga_times(mi_tga_ctx* c, float* ms, int* launches) {
  if (!c || !ms || !launches) return MI_TGA_ERR_ARG;
  int rc = stream_sync(c), total = 0;
  Timer* t[3] = {&c->t_scan, &c->t_index, &c->t_expand};
  for (int k = 0; k < 3 && rc == MI_TGA_OK; k++) {
    int pairs = 0;
    rc = t[k]->collect(c, &ms[k], &pairs);
    total += pairs;
  }
  if (rc == MI_TGA_OK) *launches = total;
  return rc;
}

}  // extern "C"
