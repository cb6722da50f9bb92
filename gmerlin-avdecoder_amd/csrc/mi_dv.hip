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

static_assert(MI_DV_FRAME_BYTES == kFrameBytes && MI_DV_PICTURE_BYTES == kPicBytes, "header and kernels agree");
static_assert(MI_DV_625_FRAME_BYTES == Sys625::kFrameBytes && MI_DV_625_PICTURE_BYTES == Sys625::kPicBytes &&
                  MI_DV_625_HEIGHT == Sys625::kH && MI_DV_625_CHROMA_WIDTH == Sys625::kCW &&
                  MI_DV_625_CHROMA_HEIGHT == Sys625::kCH && MI_DV_SYS_525_60 == Sys525::kId && MI_DV_SYS_625_50 == Sys625::kId,
              "header and kernels agree (625/50)");
static_assert(MI_DV_SYS_525_60_422 == Sys525_422::kId && MI_DV_525_422_FRAME_BYTES == Sys525_422::kFrameBytes &&
                  MI_DV_525_422_PICTURE_BYTES == Sys525_422::kPicBytes && MI_DV_HEIGHT == Sys525_422::kH &&
                  MI_DV_SYS_625_50_422 == Sys625_422::kId && MI_DV_625_422_FRAME_BYTES == Sys625_422::kFrameBytes &&
                  MI_DV_625_422_PICTURE_BYTES == Sys625_422::kPicBytes && MI_DV_625_HEIGHT == Sys625_422::kH &&
                  MI_DV_422_CHROMA_WIDTH == Sys525_422::kCW && MI_DV_422_CHROMA_WIDTH == Sys625_422::kCW &&
                  Sys525_422::kCH == Sys525_422::kH && Sys625_422::kCH == Sys625_422::kH && MI_DV_WIDTH == Sys525_422::kW &&
                  MI_DV_WIDTH == Sys625_422::kW,
              "header and kernels agree (4:2:2)");
static_assert(MI_DV_SYS_625_50_411 == Sys625_411::kId && MI_DV_625_FRAME_BYTES == Sys625_411::kFrameBytes &&
                  MI_DV_625_411_PICTURE_BYTES == Sys625_411::kPicBytes && MI_DV_625_411_CHROMA_WIDTH == Sys625_411::kCW &&
                  MI_DV_625_HEIGHT == Sys625_411::kH && MI_DV_625_HEIGHT == Sys625_411::kCH && MI_DV_WIDTH == Sys625_411::kW,
              "header and kernels agree (625/50 4:1:1)");
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

// one checked host frame of system S through the kernel into the caller's planes
template <class S>
int decode_one(mi_dv_ctx* c, const char* who, const uint8_t* frame, uint8_t* const planes[3], const int strides[3]) {
  if (strides[0] < S::kW || strides[1] < S::kCW || strides[2] < S::kCW) return fail(c, MI_DV_ERR_ARG, "strides below the picture's width");
  DVCHK(c, hipSetDevice(c->device));
  int rc = one_frame_buffers(c, S::kFrameBytes, S::kPicBytes);
  if (rc != MI_DV_OK) return rc;
  DVCHK(c, hipMemcpyAsync(c->d_frame, frame, S::kFrameBytes, hipMemcpyHostToDevice, c->stream));
  rc = launch<S>(c, who, c->d_frame, 1, c->d_pic);
  if (rc != MI_DV_OK) return rc;
  DVCHK(c, hipMemcpyAsync(c->h_pic, c->d_pic, S::kPicBytes, hipMemcpyDeviceToHost, c->stream));
  DVCHK(c, hipStreamSynchronize(c->stream));
  const uint8_t* src = c->h_pic;
  for (int pl = 0; pl < 3; pl++) {
    const int w = pl ? S::kCW : S::kW, h = pl ? S::kCH : S::kH;
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
  if (system == MI_DV_SYS_525_60) return launch<Sys525>(c, "mi_dv_decode_batch_sys", d_frames, n, d_pics);
  if (system == MI_DV_SYS_625_50) return launch<Sys625>(c, "mi_dv_decode_batch_sys", d_frames, n, d_pics);
  if (system == MI_DV_SYS_625_50_411) return launch<Sys625_411>(c, "mi_dv_decode_batch_sys", d_frames, n, d_pics);
  if (system == MI_DV_SYS_525_60_422) return launch<Sys525_422>(c, "mi_dv_decode_batch_sys", d_frames, n, d_pics);
  if (system == MI_DV_SYS_625_50_422) return launch<Sys625_422>(c, "mi_dv_decode_batch_sys", d_frames, n, d_pics);
  return fail(c, MI_DV_ERR_ARG, "mi_dv_decode_batch_sys: unknown system %d", system);
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
  if (!c || !frame || !planes || !strides || !planes[0] || !planes[1] || !planes[2])
    return fail(c, MI_DV_ERR_ARG, "mi_dv_decode_frame: NULL argument");
  if (len < (size_t)kFrameBytes) return fail(c, MI_DV_ERR_FORMAT, "DIF frame of %zu bytes: 525/60 frames have %d", len, kFrameBytes);
  // dv_frame_profile (lib/dvframe.c:298-316): DSF = byte 3 bit 7, stype = byte 80*5+48+3 & 0x1f; only 525/60 25 Mbit/s here
  if ((frame[3] & 0x80) || (frame[80 * 5 + 48 + 3] & 0x1f) != 0)
    return fail(c, MI_DV_ERR_FORMAT, "not a 525/60 25 Mbit/s DV frame (DSF %d, stype 0x%02x)", frame[3] >> 7, frame[80 * 5 + 48 + 3] & 0x1f);
  return decode_one<Sys525>(c, "mi_dv_decode_frame", frame, planes, strides);
}

int mi_dv_system_of(const uint8_t* frame, size_t len) {
  // dv_frame_profile (lib/dvframe.c:298-316): DSF = byte 3 bit 7, APT = byte 5 & 7, stype = byte 80*5+48+3 & 0x1f
  if (!frame || len < 80 * 6) return -1;
  const int dsf = frame[3] >> 7, apt = frame[5] & 7, stype = frame[80 * 5 + 48 + 3] & 0x1f;
  if (stype != 0) return -1;  // DVCPRO50 (mi_dv_profile_of knows it) and the HD profiles
  if (dsf == 0) return len >= (size_t)Sys525::kFrameBytes ? MI_DV_SYS_525_60 : -1;
  if (apt != 0) return -1;  // DVCPRO 625/50 4:1:1 (lib/dvframe.c:303)
  return len >= (size_t)Sys625::kFrameBytes ? MI_DV_SYS_625_50 : -1;
}

int mi_dv_profile_of(const uint8_t* frame, size_t len) {
  if (!frame || len < 80 * 6) return -1;
  const int dsf = frame[3] >> 7, stype = frame[80 * 5 + 48 + 3] & 0x1f;
  if (stype == 0x4) {  // DVCPRO50: two DIF channels, 4:2:2 (lib/dvframe.c:170-211)
    if (dsf == 0) return len >= (size_t)Sys525_422::kFrameBytes ? MI_DV_SYS_525_60_422 : -1;
    return len >= (size_t)Sys625_422::kFrameBytes ? MI_DV_SYS_625_50_422 : -1;
  }
  return mi_dv_system_of(frame, len);
}

int mi_dv_kind_of(const uint8_t* frame, size_t len) {
  // lib/dvframe.c:303: DSF 1 with stype 0 is the IEC 4:2:0 profile for APT 0 and DVCPRO 625/50 4:1:1 for any other APT
  if (!frame || len < 80 * 6) return -1;
  const int dsf = frame[3] >> 7, apt = frame[5] & 7, stype = frame[80 * 5 + 48 + 3] & 0x1f;
  if (dsf == 1 && stype == 0 && apt != 0) return len >= (size_t)Sys625_411::kFrameBytes ? MI_DV_SYS_625_50_411 : -1;
  return mi_dv_profile_of(frame, len);
}

int mi_dv_decode_frame_sys(mi_dv_ctx* c, int system, const uint8_t* frame, size_t len, uint8_t* const planes[3],
                           const int strides[3]) {
  if (system == MI_DV_SYS_525_60) return mi_dv_decode_frame(c, frame, len, planes, strides);
  if (system != MI_DV_SYS_625_50 && system != MI_DV_SYS_625_50_411 && system != MI_DV_SYS_525_60_422 &&
      system != MI_DV_SYS_625_50_422)
    return fail(c, MI_DV_ERR_ARG, "mi_dv_decode_frame_sys: unknown system %d", system);
  if (!c || !frame || !planes || !strides || !planes[0] || !planes[1] || !planes[2])
    return fail(c, MI_DV_ERR_ARG, "mi_dv_decode_frame_sys: NULL argument");
  if (system == MI_DV_SYS_625_50) {
    using S = Sys625;
    if (len < (size_t)S::kFrameBytes) return fail(c, MI_DV_ERR_FORMAT, "DIF frame of %zu bytes: 625/50 frames have %d", len, S::kFrameBytes);
    if (mi_dv_system_of(frame, len) != MI_DV_SYS_625_50)
      return fail(c, MI_DV_ERR_FORMAT, "not a 625/50 25 Mbit/s 4:2:0 DV frame (DSF %d, APT %d, stype 0x%02x)", frame[3] >> 7,
                  frame[5] & 7, frame[80 * 5 + 48 + 3] & 0x1f);
    return decode_one<S>(c, "mi_dv_decode_frame_sys", frame, planes, strides);
  }
  if (system == MI_DV_SYS_625_50_411) {
    using S = Sys625_411;
    if (len < (size_t)S::kFrameBytes)
      return fail(c, MI_DV_ERR_FORMAT, "DIF frame of %zu bytes: 625/50 4:1:1 frames have %d", len, S::kFrameBytes);
    if (mi_dv_kind_of(frame, len) != MI_DV_SYS_625_50_411)
      return fail(c, MI_DV_ERR_FORMAT, "not a 625/50 25 Mbit/s 4:1:1 (DVCPRO) DV frame (DSF %d, APT %d, stype 0x%02x; expected DSF 1, "
                  "APT not 0, stype 0x00)", frame[3] >> 7, frame[5] & 7, frame[80 * 5 + 48 + 3] & 0x1f);
    return decode_one<S>(c, "mi_dv_decode_frame_sys", frame, planes, strides);
  }
  // the 50 Mbit/s systems: DSF = byte 3 bit 7, stype = byte 80*5+48+3 & 0x1f must be 0x4 (lib/dvframe.c:298-316)
  const bool pal = system == MI_DV_SYS_625_50_422;
  const char* name = pal ? "625/50" : "525/60";
  const int need = pal ? Sys625_422::kFrameBytes : Sys525_422::kFrameBytes;
  if (len < (size_t)need)
    return fail(c, MI_DV_ERR_FORMAT, "DIF frame of %zu bytes: %s 50 Mbit/s 4:2:2 frames have %d", len, name, need);
  if (mi_dv_profile_of(frame, len) != system)
    return fail(c, MI_DV_ERR_FORMAT, "not a %s 50 Mbit/s 4:2:2 DV frame of %d bytes (DSF %d, stype 0x%02x; expected DSF %d, stype 0x04)",
                name, need, frame[3] >> 7, frame[80 * 5 + 48 + 3] & 0x1f, pal ? 1 : 0);
  if (pal) return decode_one<Sys625_422>(c, "mi_dv_decode_frame_sys", frame, planes, strides);
  return decode_one<Sys525_422>(c, "mi_dv_decode_frame_sys", frame, planes, strides);
}

int mi_dv_mb_place(int system, int seq, int slot, int m, int* x, int* y) {
  const int seqs = system == MI_DV_SYS_525_60       ? Sys525::kSeqs
                   : system == MI_DV_SYS_625_50     ? Sys625::kSeqs
                   : system == MI_DV_SYS_625_50_411 ? Sys625_411::kSeqs
                   : system == MI_DV_SYS_525_60_422 ? 2 * Sys525_422::kSeqs  // (both channels' sequences, in byte order)
                   : system == MI_DV_SYS_625_50_422 ? 2 * Sys625_422::kSeqs
                                                    : 0;
  if (!x || !y || seq < 0 || seq >= seqs || slot < 0 || slot >= 27 || m < 0 || m >= 5)
    return fail(nullptr, MI_DV_ERR_ARG, "mi_dv_mb_place: system %d, sequence %d, segment %d, macroblock %d out of range", system, seq, slot, m);
  uint32_t ux, uy;
  if (system == MI_DV_SYS_525_60) Sys525::place((uint32_t)seq, (uint32_t)slot, (uint32_t)m, ux, uy);
  else if (system == MI_DV_SYS_625_50) Sys625::place((uint32_t)seq, (uint32_t)slot, (uint32_t)m, ux, uy);
  else if (system == MI_DV_SYS_625_50_411) Sys625_411::place((uint32_t)seq, (uint32_t)slot, (uint32_t)m, ux, uy);
  else if (system == MI_DV_SYS_525_60_422) Sys525_422::place((uint32_t)seq, (uint32_t)slot, (uint32_t)m, ux, uy);
  else Sys625_422::place((uint32_t)seq, (uint32_t)slot, (uint32_t)m, ux, uy);
  *x = (int)ux;
  *y = (int)uy;
  return MI_DV_OK;
}

}  // extern "C"
