// mi_dv.hip — C ABI (include/mi_dv.h) of the MI355X DV decoder (25 Mbit/s: 525/60 4:1:1, 625/50 4:2:0, 625/50 4:1:1;
// 50 Mbit/s: both line systems in 4:2:2).  No CPU path: without a gfx950 device every call fails with a message.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mi_dv.h"
#include "dv_common.h"
#include "dv_decode_kernels.h"

using namespace midv;

// header and kernels agree: a system's id, frame, picture and planes as include/mi_dv.h states them
template <class S, int Id, int FrameBytes, int PicBytes, int H, int CW, int CH>
constexpr bool kAgrees = S::kId == Id && S::kFrameBytes == FrameBytes && S::kPicBytes == PicBytes && S::kW == MI_DV_WIDTH &&
                         S::kH == H && S::kCW == CW && S::kCH == CH;
static_assert(kAgrees<Sys525, MI_DV_SYS_525_60, MI_DV_FRAME_BYTES, MI_DV_PICTURE_BYTES, MI_DV_HEIGHT, MI_DV_CHROMA_WIDTH, MI_DV_HEIGHT> &&
                  MI_DV_FRAME_BYTES == kFrameBytes && MI_DV_PICTURE_BYTES == kPicBytes, "header and kernels agree");
static_assert(kAgrees<Sys625, MI_DV_SYS_625_50, MI_DV_625_FRAME_BYTES, MI_DV_625_PICTURE_BYTES, MI_DV_625_HEIGHT,
                      MI_DV_625_CHROMA_WIDTH, MI_DV_625_CHROMA_HEIGHT>, "header and kernels agree (625/50)");
static_assert(kAgrees<Sys625_411, MI_DV_SYS_625_50_411, MI_DV_625_FRAME_BYTES, MI_DV_625_411_PICTURE_BYTES, MI_DV_625_HEIGHT,
                      MI_DV_625_411_CHROMA_WIDTH, MI_DV_625_HEIGHT>, "header and kernels agree (625/50 4:1:1)");
static_assert(kAgrees<Sys525_422, MI_DV_SYS_525_60_422, MI_DV_525_422_FRAME_BYTES, MI_DV_525_422_PICTURE_BYTES, MI_DV_HEIGHT,
                      MI_DV_422_CHROMA_WIDTH, MI_DV_HEIGHT>, "header and kernels agree (525/60 4:2:2)");
static_assert(kAgrees<Sys625_422, MI_DV_SYS_625_50_422, MI_DV_625_422_FRAME_BYTES, MI_DV_625_422_PICTURE_BYTES, MI_DV_625_HEIGHT,
                      MI_DV_422_CHROMA_WIDTH, MI_DV_625_HEIGHT>, "header and kernels agree (625/50 4:2:2)");
static_assert(MI_DV_SYS_525_60_422 == (0x4 | 0) && MI_DV_SYS_625_50_422 == (0x4 | 1), "4:2:2 system = stype | DSF");

namespace {
std::mutex g_mu;
std::string g_err;
}  // namespace

struct mi_dv_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  Tables* d_tab = nullptr;
  // one pair of events around every launch since the last mi_dv_kernel_times (recycled there)
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_used, ev_free;
  // the one-frame path's buffers: as large as the largest system this instance has seen needs them
  uint8_t* d_frame = nullptr;
  uint8_t* d_pic = nullptr;
  uint8_t* h_pic = nullptr;  // pinned
  size_t cap_frame = 0, cap_pic = 0;
  std::string err;
};

namespace {
int fail(mi_dv_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  else {
    std::lock_guard<std::mutex> l(g_mu);
    g_err = buf;
  }
  return code;
}
#define DVCHK(c, call)                                                                                              \
  do {                                                                                                              \
    hipError_t e_ = (call);                                                                                         \
    if (e_ != hipSuccess)                                                                                           \
      return fail((c), MI_DV_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__);   \
  } while (0)

bool is_gfx950(int dev) {
  hipDeviceProp_t p;
  return hipGetDeviceProperties(&p, dev) == hipSuccess && strncmp(p.gcnArchName, "gfx950", 6) == 0;
}
}  // namespace

extern "C" {

int mi_dv_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  int ok = 0;
  for (int i = 0; i < n; i++) ok += is_gfx950(i);
  return ok;
}

const char* mi_dv_last_error(const mi_dv_ctx* c) {
  if (c) return c->err.c_str();
  std::lock_guard<std::mutex> l(g_mu);
  return g_err.c_str();
}

mi_dv_ctx* mi_dv_create(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) {
    fail(nullptr, MI_DV_ERR_HIP, "no HIP device: the DV decoder has no CPU path");
    return nullptr;
  }
  if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
  if (device >= n || !is_gfx950(device)) {
    fail(nullptr, MI_DV_ERR_ARG, "device %d is not a gfx950 (MI355X) device", device);
    return nullptr;
  }
  Tables t;
  if (!build_tables(&t)) {
    fail(nullptr, MI_DV_ERR_ARG, "internal: the variable-length code's tables are inconsistent");
    return nullptr;
  }
  mi_dv_ctx* c = new mi_dv_ctx();
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipMalloc((void**)&c->d_tab, sizeof(Tables)) != hipSuccess ||
      hipMemcpy(c->d_tab, &t, sizeof t, hipMemcpyHostToDevice) != hipSuccess) {
    fail(nullptr, MI_DV_ERR_HIP, "cannot set up device %d: %s", device, hipGetErrorString(hipGetLastError()));
    mi_dv_destroy(c);
    return nullptr;
  }
  return c;
}

void mi_dv_destroy(mi_dv_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->d_tab) (void)hipFree(c->d_tab);
  if (c->d_frame) (void)hipFree(c->d_frame);
  if (c->d_pic) (void)hipFree(c->d_pic);
  if (c->h_pic) (void)hipHostFree(c->h_pic);
  for (auto* v : {&c->ev_used, &c->ev_free})
    for (auto& e : *v) {
      (void)hipEventDestroy(e.first);
      (void)hipEventDestroy(e.second);
    }
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

void* mi_dv_dev_alloc(mi_dv_ctx* c, size_t bytes) {
  if (!c) return nullptr;
  void* d = nullptr;
  if (hipSetDevice(c->device) != hipSuccess || hipMalloc(&d, bytes ? bytes : 1) != hipSuccess) {
    fail(c, MI_DV_ERR_NOMEM, "hipMalloc(%zu) failed", bytes);
    return nullptr;
  }
  return d;
}
void mi_dv_dev_free(mi_dv_ctx* c, void* d) {
  if (!c || !d) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  (void)hipFree(d);
}
int mi_dv_h2d(mi_dv_ctx* c, void* d, const void* h, size_t n) {
  if (!c || (!d && n) || (!h && n)) return fail(c, MI_DV_ERR_ARG, "mi_dv_h2d: NULL argument");
  DVCHK(c, hipSetDevice(c->device));
  DVCHK(c, hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, c->stream));
  DVCHK(c, hipStreamSynchronize(c->stream));
  return MI_DV_OK;
}
int mi_dv_d2h(mi_dv_ctx* c, void* h, const void* d, size_t n) {
  if (!c || (!d && n) || (!h && n)) return fail(c, MI_DV_ERR_ARG, "mi_dv_d2h: NULL argument");
  DVCHK(c, hipSetDevice(c->device));
  DVCHK(c, hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, c->stream));
  DVCHK(c, hipStreamSynchronize(c->stream));
  return MI_DV_OK;
}
int mi_dv_sync(mi_dv_ctx* c) {
  if (!c) return MI_DV_ERR_ARG;
  DVCHK(c, hipSetDevice(c->device));
  DVCHK(c, hipStreamSynchronize(c->stream));
  return MI_DV_OK;
}

#ifdef MIDV_DEBUG
static void* g_dbg = nullptr;
extern "C" void mi_dv_debug_buffer(void* d) { g_dbg = d; }
#endif
}  // extern "C"

namespace {
// the launch of either system's kernel, with its events (`who`: the entry point the messages name)
template <class Sys>
int launch(mi_dv_ctx* c, const char* who, const void* d_frames, int n, void* d_pics) {
  if (!c || !d_frames || !d_pics || n <= 0) return fail(c, MI_DV_ERR_ARG, "%s: bad argument", who);
  if (n > 65535) return fail(c, MI_DV_ERR_ARG, "%s: %d frames; at most 65535 per call (split the batch)", who, n);
  if (((uintptr_t)d_frames & 3u) || ((uintptr_t)d_pics & 7u))
    return fail(c, MI_DV_ERR_ARG, "%s: d_frames must be 4-byte and d_pics 8-byte aligned", who);
  DVCHK(c, hipSetDevice(c->device));
  std::pair<hipEvent_t, hipEvent_t> ev;
  if (!c->ev_free.empty()) {
    ev = c->ev_free.back();
    c->ev_free.pop_back();
  } else {
    DVCHK(c, hipEventCreate(&ev.first));
    DVCHK(c, hipEventCreate(&ev.second));
  }
  c->ev_used.push_back(ev);
  if (c->ev_used.size() > 4096) {  // nobody asks for times: keep the newest
    c->ev_free.push_back(c->ev_used.front());
    c->ev_used.erase(c->ev_used.begin());
  }
  DVCHK(c, hipEventRecord(ev.first, c->stream));
  hipLaunchKernelGGL(k_dv_decode<Sys>, dim3(kDvGridX<Sys>, (unsigned)n), dim3(64 * kDvWaves), 0, c->stream,
                     (const uint8_t*)d_frames, (uint8_t*)d_pics, c->d_tab
#ifdef MIDV_DEBUG
                     , (int16_t*)g_dbg
#endif
  );
  DVCHK(c, hipGetLastError());
  DVCHK(c, hipEventRecord(ev.second, c->stream));
  return MI_DV_OK;
}

// the one-frame path's buffers hold a frame and a picture of these sizes (they only grow; the stream is idle between calls)
int one_frame_buffers(mi_dv_ctx* c, size_t frame_bytes, size_t pic_bytes) {
  if (frame_bytes > c->cap_frame) {
    if (c->d_frame) DVCHK(c, hipFree(c->d_frame));
    c->d_frame = nullptr;
    c->cap_frame = 0;
    DVCHK(c, hipMalloc((void**)&c->d_frame, frame_bytes));
    c->cap_frame = frame_bytes;
  }
  if (pic_bytes > c->cap_pic) {
    if (c->d_pic) DVCHK(c, hipFree(c->d_pic));
    if (c->h_pic) DVCHK(c, hipHostFree(c->h_pic));
    c->d_pic = c->h_pic = nullptr;
    c->cap_pic = 0;
    DVCHK(c, hipMalloc((void**)&c->d_pic, pic_bytes));
    DVCHK(c, hipHostMalloc((void**)&c->h_pic, pic_bytes, hipHostMallocDefault));
    c->cap_pic = pic_bytes;
  }
  return MI_DV_OK;
}

// ---- the five systems, once: what the entry points below need of each (generated from csrc/dv_common.h's Sys*) ----
struct Row {
  int id, frame_bytes, pic_bytes, w[3], h[3];  // the planes Y, Cb, Cr
  int place_seqs;                              // the sequences mi_dv_mb_place takes: both channels', in byte order
  // what the one-frame path's messages say: "<frames> frames have ...", "not a <what> (DSF ..., [APT ...,] stype ...<expected>)"
  const char *frames, *what, *expected;
  bool says_apt;
  int (*launch)(mi_dv_ctx*, const char*, const void*, int, void*);
  void (*place)(uint32_t, uint32_t, uint32_t, uint32_t&, uint32_t&);
};
// a host function of its own: the kernels' S::place stays what dv_common.h makes of it
template <class S>
void place_thunk(uint32_t seq, uint32_t slot, uint32_t m, uint32_t& x, uint32_t& y) {
  S::place(seq, slot, m, x, y);
}
template <class S>
constexpr Row row(const char* frames, const char* what, bool says_apt, const char* expected) {
  return {S::kId, S::kFrameBytes, S::kPicBytes, {S::kW, S::kCW, S::kCW}, {S::kH, S::kCH, S::kCH}, S::kChans * S::kSeqs,
          frames, what, expected, says_apt, launch<S>, place_thunk<S>};
}
constexpr Row kSystems[] = {
    row<Sys525>("525/60", "525/60 25 Mbit/s DV frame", false, ""),
    row<Sys625>("625/50", "625/50 25 Mbit/s 4:2:0 DV frame", true, ""),
    row<Sys625_411>("625/50 4:1:1", "625/50 25 Mbit/s 4:1:1 (DVCPRO) DV frame", true, "; expected DSF 1, APT not 0, stype 0x00"),
    row<Sys525_422>("525/60 50 Mbit/s 4:2:2", "525/60 50 Mbit/s 4:2:2 DV frame of 240000 bytes", false, "; expected DSF 0, stype 0x04"),
    row<Sys625_422>("625/50 50 Mbit/s 4:2:2", "625/50 50 Mbit/s 4:2:2 DV frame of 288000 bytes", false, "; expected DSF 1, stype 0x04"),
};
const Row* find(int system) {  // nullptr: 2, 6 and the like are no systems
  for (const Row& r : kSystems)
    if (r.id == system) return &r;
  return nullptr;
}

// dv_frame_profile (lib/dvframe.c:298-316) over the five systems: DSF = byte 3 bit 7, APT = byte 5 & 7, stype = byte
// 80*5+48+3 & 0x1f.  stype 0 is 25 Mbit/s: 525/60 for DSF 0; for DSF 1 the IEC 4:2:0 profile with APT 0 and DVCPRO 625/50
// 4:1:1 with any other (:303).  stype 4 is DVCPRO50, two DIF channels, 4:2:2 (:170-211): the system is stype | DSF.  -1: the
// HD profiles, and a frame shorter than its system's
int classify(const uint8_t* frame, size_t len) {
  if (!frame || len < 80 * 6) return -1;
  const int dsf = frame[3] >> 7, apt = frame[5] & 7, stype = frame[80 * 5 + 48 + 3] & 0x1f;
  if (stype != 0 && stype != 0x4) return -1;
  const int system = stype ? stype | dsf : !dsf ? MI_DV_SYS_525_60 : !apt ? MI_DV_SYS_625_50 : MI_DV_SYS_625_50_411;
  return len >= (size_t)find(system)->frame_bytes ? system : -1;
}

// one host frame of system r, checked (arguments, length, announcement: in this order), through the kernel into the
// caller's planes
int decode_one(mi_dv_ctx* c, const Row& r, const char* who, const uint8_t* frame, size_t len, uint8_t* const planes[3],
               const int strides[3]) {
  if (!c || !frame || !planes || !strides || !planes[0] || !planes[1] || !planes[2])
    return fail(c, MI_DV_ERR_ARG, "%s: NULL argument", who);
  if (len < (size_t)r.frame_bytes)
    return fail(c, MI_DV_ERR_FORMAT, "DIF frame of %zu bytes: %s frames have %d", len, r.frames, r.frame_bytes);
  if (classify(frame, len) != r.id) {
    const int dsf = frame[3] >> 7, apt = frame[5] & 7, stype = frame[80 * 5 + 48 + 3] & 0x1f;
    char seen[64];
    if (r.says_apt) snprintf(seen, sizeof seen, "DSF %d, APT %d, stype 0x%02x", dsf, apt, stype);
    else snprintf(seen, sizeof seen, "DSF %d, stype 0x%02x", dsf, stype);
    return fail(c, MI_DV_ERR_FORMAT, "not a %s (%s%s)", r.what, seen, r.expected);
  }
  if (strides[0] < r.w[0] || strides[1] < r.w[1] || strides[2] < r.w[2]) return fail(c, MI_DV_ERR_ARG, "strides below the picture's width");
  DVCHK(c, hipSetDevice(c->device));
  int rc = one_frame_buffers(c, (size_t)r.frame_bytes, (size_t)r.pic_bytes);
  if (rc != MI_DV_OK) return rc;
  DVCHK(c, hipMemcpyAsync(c->d_frame, frame, (size_t)r.frame_bytes, hipMemcpyHostToDevice, c->stream));
  rc = r.launch(c, who, c->d_frame, 1, c->d_pic);
  if (rc != MI_DV_OK) return rc;
  DVCHK(c, hipMemcpyAsync(c->h_pic, c->d_pic, (size_t)r.pic_bytes, hipMemcpyDeviceToHost, c->stream));
  DVCHK(c, hipStreamSynchronize(c->stream));
  const uint8_t* src = c->h_pic;
  for (int pl = 0; pl < 3; pl++) {
    const int w = r.w[pl], h = r.h[pl];
    for (int y = 0; y < h; y++) memcpy(planes[pl] + (size_t)y * strides[pl], src + (size_t)y * w, (size_t)w);
    src += (size_t)w * h;
  }
  return MI_DV_OK;
}
}  // namespace

extern "C" {

int mi_dv_decode_batch(mi_dv_ctx* c, const void* d_frames, int n, void* d_pics) {
  return launch<Sys525>(c, "mi_dv_decode_batch", d_frames, n, d_pics);
}

int mi_dv_decode_batch_sys(mi_dv_ctx* c, int system, const void* d_frames, int n, void* d_pics) {
  const Row* r = find(system);
  if (!r) return fail(c, MI_DV_ERR_ARG, "mi_dv_decode_batch_sys: unknown system %d", system);
  return r->launch(c, "mi_dv_decode_batch_sys", d_frames, n, d_pics);
}

int mi_dv_kernel_times(mi_dv_ctx* c, float* total_ms, int* launches) {
  if (!c || !total_ms || !launches) return MI_DV_ERR_ARG;
  DVCHK(c, hipSetDevice(c->device));
  DVCHK(c, hipStreamSynchronize(c->stream));
  float sum = 0.f;
  for (auto& e : c->ev_used) {
    float ms = 0.f;
    DVCHK(c, hipEventElapsedTime(&ms, e.first, e.second));
    sum += ms;
  }
  *total_ms = sum;
  *launches = (int)c->ev_used.size();
  for (auto& e : c->ev_used) c->ev_free.push_back(e);
  c->ev_used.clear();
  return MI_DV_OK;
}

size_t mi_dv_copy_tables(void* out, size_t cap) {
  Tables t;
  if (!build_tables(&t)) return 0;
  if (out && cap >= sizeof t) memcpy(out, &t, sizeof t);
  return sizeof t;
}

int mi_dv_decode_frame(mi_dv_ctx* c, const uint8_t* frame, size_t len, uint8_t* const planes[3], const int strides[3]) {
  return decode_one(c, *find(MI_DV_SYS_525_60), "mi_dv_decode_frame", frame, len, planes, strides);
}

int mi_dv_decode_frame_sys(mi_dv_ctx* c, int system, const uint8_t* frame, size_t len, uint8_t* const planes[3],
                           const int strides[3]) {
  if (system == MI_DV_SYS_525_60) return mi_dv_decode_frame(c, frame, len, planes, strides);  // under its own name
  const Row* r = find(system);
  if (!r) return fail(c, MI_DV_ERR_ARG, "mi_dv_decode_frame_sys: unknown system %d", system);
  return decode_one(c, *r, "mi_dv_decode_frame_sys", frame, len, planes, strides);
}

// the three queries are one classification, each with the systems it was written to know (include/mi_dv.h)
int mi_dv_kind_of(const uint8_t* frame, size_t len) { return classify(frame, len); }

int mi_dv_profile_of(const uint8_t* frame, size_t len) {
  const int k = classify(frame, len);
  return k == MI_DV_SYS_625_50_411 ? -1 : k;
}

int mi_dv_system_of(const uint8_t* frame, size_t len) {
  const int k = classify(frame, len);
  return k == MI_DV_SYS_525_60 || k == MI_DV_SYS_625_50 ? k : -1;
}

int mi_dv_mb_place(int system, int seq, int slot, int m, int* x, int* y) {
  const Row* r = find(system);
  if (!x || !y || !r || seq < 0 || seq >= r->place_seqs || slot < 0 || slot >= 27 || m < 0 || m >= 5)
    return fail(nullptr, MI_DV_ERR_ARG, "mi_dv_mb_place: system %d, sequence %d, segment %d, macroblock %d out of range", system, seq, slot, m);
  uint32_t ux, uy;
  r->place((uint32_t)seq, (uint32_t)slot, (uint32_t)m, ux, uy);
  *x = (int)ux;
  *y = (int)uy;
  return MI_DV_OK;
}

}  // extern "C"
