// mi_dv.hip — C ABI (include/mi_dv.h) of the MI355X DV decoder and encoder (25 Mbit/s: 525/60 4:1:1, 625/50 4:2:0, 625/50 4:1:1;
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
#include "dv_hold_kernels.h"
#include "dv_encode_kernels.h"

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
  // the encoder (mi_dv_encode_*): its tables, the last batch's counts (kEncStats), one pair of events around every launch
  // since the last mi_dv_encode_times
  EncTables* d_enc = nullptr;
  unsigned long long* d_enc_stats = nullptr;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> enc_ev_used;
  // one pair of events around every launch since the last mi_dv_kernel_times (recycled there)
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_used, ev_free;
  // the one-frame path's buffers: as large as the largest system this instance has seen needs them
  uint8_t* d_frame = nullptr;
  uint8_t* d_pic = nullptr;
  uint8_t* h_pic = nullptr;  // pinned
  size_t cap_frame = 0, cap_pic = 0;
  // the held calls (mi_dv_decode_batch_held, mi_dv_decode_frame_held).  Everything only grows.
  struct Hold {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_used;  // one pair around every phase 2 since the last mi_dv_hold_times
    uint8_t* h_desc = nullptr;                               // pinned: the chunks, then the runs, of the last batch
    uint8_t* d_desc = nullptr;
    size_t cap_desc = 0;
    hipEvent_t desc_done = nullptr;  // behind the last upload of h_desc
    uint64_t* d_mask = nullptr;      // [chunk][macroblock]
    int32_t* d_carry = nullptr;
    size_t cap_rows = 0;
    unsigned long long* d_held = nullptr;  // kHoldCounters partial counts
    bool counted = false;  // the last held batch ran phase 2: d_held is its count (else the count is 0)
    // the one-frame path: per system the last picture and the one being made, in turns; the system whose keep[][cur] is
    // the picture of the frame decoded last (-1: none; the next frame has no source)
    uint8_t* keep[6][2] = {};
    int cur[6] = {};
    int kept = -1;
  } hold;
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
  EncTables et;
  if (!build_enc_tables(&et)) {
    fail(nullptr, MI_DV_ERR_ARG, "internal: the variable-length code lists a pair outside the encoder's table");
    return nullptr;
  }
  mi_dv_ctx* c = new mi_dv_ctx();
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipMalloc((void**)&c->d_tab, sizeof(Tables)) != hipSuccess ||
      hipMemcpy(c->d_tab, &t, sizeof t, hipMemcpyHostToDevice) != hipSuccess ||
      hipMalloc((void**)&c->d_enc, sizeof(EncTables)) != hipSuccess ||
      hipMemcpy(c->d_enc, &et, sizeof et, hipMemcpyHostToDevice) != hipSuccess ||
      hipMalloc((void**)&c->d_enc_stats, kEncStats * sizeof(unsigned long long)) != hipSuccess ||
      hipMemset(c->d_enc_stats, 0, kEncStats * sizeof(unsigned long long)) != hipSuccess) {
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
  if (c->d_enc) (void)hipFree(c->d_enc);
  if (c->d_enc_stats) (void)hipFree(c->d_enc_stats);
  if (c->d_frame) (void)hipFree(c->d_frame);
  if (c->d_pic) (void)hipFree(c->d_pic);
  if (c->h_pic) (void)hipHostFree(c->h_pic);
  if (c->hold.h_desc) (void)hipHostFree(c->hold.h_desc);
  for (void* d : {(void*)c->hold.d_desc, (void*)c->hold.d_mask, (void*)c->hold.d_carry, (void*)c->hold.d_held})
    if (d) (void)hipFree(d);
  for (auto& k : c->hold.keep)
    for (uint8_t* d : k)
      if (d) (void)hipFree(d);
  if (c->hold.desc_done) (void)hipEventDestroy(c->hold.desc_done);
  for (auto* v : {&c->ev_used, &c->ev_free, &c->hold.ev_used, &c->enc_ev_used})
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

// the launch of a system's encoder kernel with its events; the arguments are checked by encode_batch below
template <class Sys>
int encode_launch(mi_dv_ctx* c, const void* d_pics, int n, void* d_frames, int flags) {
  std::pair<hipEvent_t, hipEvent_t> ev;
  if (!c->ev_free.empty()) {
    ev = c->ev_free.back();
    c->ev_free.pop_back();
  } else {
    DVCHK(c, hipEventCreate(&ev.first));
    DVCHK(c, hipEventCreate(&ev.second));
  }
  c->enc_ev_used.push_back(ev);
  if (c->enc_ev_used.size() > 4096) {  // nobody asks for times: keep the newest
    c->ev_free.push_back(c->enc_ev_used.front());
    c->enc_ev_used.erase(c->enc_ev_used.begin());
  }
  DVCHK(c, hipMemsetAsync(c->d_enc_stats, 0, kEncStats * sizeof(unsigned long long), c->stream));
  DVCHK(c, hipEventRecord(ev.first, c->stream));
  hipLaunchKernelGGL(k_dv_encode<Sys>, dim3(kEncGridX<Sys>, (unsigned)n), dim3(64), 0, c->stream, (const uint8_t*)d_pics,
                     (uint8_t*)d_frames, (const EncTables*)c->d_enc, (uint32_t)flags, c->d_enc_stats);
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
  // the held calls: macroblocks per frame, a macroblock's three rectangles, the launch of k_dv_hold_copy<Sys>
  int nmb;
  void (*rects)(uint32_t, uint32_t, uint32_t, Rect*);
  void (*hold_copy)(hipStream_t, const HoldChunkDev*, uint32_t, const uint64_t*, const int32_t*, uint8_t*, const uint8_t*,
                    unsigned long long*);
  int (*encode)(mi_dv_ctx*, const void*, int, void*, int);  // the launch of k_dv_encode<Sys>
};
// a host function of its own: the kernels' S::place stays what dv_common.h makes of it
template <class S>
void place_thunk(uint32_t seq, uint32_t slot, uint32_t m, uint32_t& x, uint32_t& y) {
  S::place(seq, slot, m, x, y);
}
template <class S>
void rects_thunk(uint32_t seq, uint32_t slot, uint32_t m, Rect* r) {
  S::rects(seq, slot, m, r);
}
// one workgroup per (super block, kHoldSub pictures of a chunk); past 65535 items the kernel strides
template <class S>
void hold_copy_launch(hipStream_t st, const HoldChunkDev* chunks, uint32_t nitems, const uint64_t* mask, const int32_t* carry,
                      uint8_t* pics, const uint8_t* prev, unsigned long long* held) {
  hipLaunchKernelGGL(k_dv_hold_copy<S>, dim3((unsigned)(S::kChans * S::kSeqs * 5), nitems < kHoldMaxGridY ? nitems : kHoldMaxGridY),
                     dim3(kHoldCopyThreads), 0, st, chunks, nitems, mask, carry, pics, prev, held);
}
template <class S>
constexpr Row row(const char* frames, const char* what, bool says_apt, const char* expected) {
  return {S::kId, S::kFrameBytes, S::kPicBytes, {S::kW, S::kCW, S::kCW}, {S::kH, S::kCH, S::kCH}, S::kChans * S::kSeqs,
          frames, what, expected, says_apt, launch<S>, place_thunk<S>, S::kSegments * 5, rects_thunk<S>, hold_copy_launch<S>,
          encode_launch<S>};
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

// one host frame of system r, checked: arguments, length, announcement, strides, in this order
int check_one(mi_dv_ctx* c, const Row& r, const char* who, const uint8_t* frame, size_t len, uint8_t* const planes[3],
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
  return MI_DV_OK;
}

// the device picture d_pic of system r through the pinned buffer into the caller's planes; synchronises
int planes_out(mi_dv_ctx* c, const Row& r, const uint8_t* d_pic, uint8_t* const planes[3], const int strides[3]) {
  DVCHK(c, hipMemcpyAsync(c->h_pic, d_pic, (size_t)r.pic_bytes, hipMemcpyDeviceToHost, c->stream));
  DVCHK(c, hipStreamSynchronize(c->stream));
  const uint8_t* src = c->h_pic;
  for (int pl = 0; pl < 3; pl++) {
    const int w = r.w[pl], h = r.h[pl];
    for (int y = 0; y < h; y++) memcpy(planes[pl] + (size_t)y * strides[pl], src + (size_t)y * w, (size_t)w);
    src += (size_t)w * h;
  }
  return MI_DV_OK;
}

// one host frame of system r, checked, through the kernel into the caller's planes
int decode_one(mi_dv_ctx* c, const Row& r, const char* who, const uint8_t* frame, size_t len, uint8_t* const planes[3],
               const int strides[3]) {
  int rc = check_one(c, r, who, frame, len, planes, strides);
  if (rc != MI_DV_OK) return rc;
  DVCHK(c, hipSetDevice(c->device));
  rc = one_frame_buffers(c, (size_t)r.frame_bytes, (size_t)r.pic_bytes);
  if (rc != MI_DV_OK) return rc;
  DVCHK(c, hipMemcpyAsync(c->d_frame, frame, (size_t)r.frame_bytes, hipMemcpyHostToDevice, c->stream));
  rc = r.launch(c, who, c->d_frame, 1, c->d_pic);
  if (rc != MI_DV_OK) return rc;
  return planes_out(c, r, c->d_pic, planes, strides);
}

// ---- the held calls ----
// room for `desc` bytes of descriptors and `rows` mask / carry entries (they only grow; growing waits for the stream)
int hold_buffers(mi_dv_ctx* c, size_t desc, size_t rows) {
  mi_dv_ctx::Hold& h = c->hold;
  if (!h.d_held) DVCHK(c, hipMalloc((void**)&h.d_held, kHoldCounters * kHoldCounterStride * sizeof(unsigned long long)));
  if (!h.desc_done) DVCHK(c, hipEventCreateWithFlags(&h.desc_done, hipEventDisableTiming));
  if (desc > h.cap_desc) {
    DVCHK(c, hipStreamSynchronize(c->stream));
    if (h.h_desc) DVCHK(c, hipHostFree(h.h_desc));
    if (h.d_desc) DVCHK(c, hipFree(h.d_desc));
    h.h_desc = h.d_desc = nullptr;
    h.cap_desc = 0;
    DVCHK(c, hipHostMalloc((void**)&h.h_desc, desc, hipHostMallocDefault));
    DVCHK(c, hipMalloc((void**)&h.d_desc, desc));
    h.cap_desc = desc;
  }
  if (rows > h.cap_rows) {
    DVCHK(c, hipStreamSynchronize(c->stream));
    if (h.d_mask) DVCHK(c, hipFree(h.d_mask));
    if (h.d_carry) DVCHK(c, hipFree(h.d_carry));
    h.d_mask = nullptr;
    h.d_carry = nullptr;
    h.cap_rows = 0;
    if (hipMalloc((void**)&h.d_mask, rows * sizeof(uint64_t)) != hipSuccess || hipMalloc((void**)&h.d_carry, rows * sizeof(int32_t)) != hipSuccess)
      return fail(c, MI_DV_ERR_NOMEM, "mi_dv_decode_batch_held: no device memory for %zu mask entries", rows);
    h.cap_rows = rows;
  }
  return MI_DV_OK;
}

void hold_forget(mi_dv_ctx* c) {
  if (c) c->hold.kept = -1;
}

// phase 1 (k_dv_decode over all n frames), then phase 2 for the runs that have a source: every argument is checked
// before anything is launched
int decode_held(mi_dv_ctx* c, const Row& r, const char* who, const void* d_frames, int n, void* d_pics, int n_runs,
                const int* run_len, const void* d_prev, unsigned sta_mask) {
  if (sta_mask > 0xFFFFu) return fail(c, MI_DV_ERR_ARG, "%s: STA mask 0x%x: one bit per STA value, at most 0xFFFF", who, sta_mask);
  if (!d_frames || !d_pics || n <= 0 || n_runs < 0) return fail(c, MI_DV_ERR_ARG, "%s: bad argument", who);
  if (n > 65535) return fail(c, MI_DV_ERR_ARG, "%s: %d frames; at most 65535 per call (split the batch)", who, n);
  if (((uintptr_t)d_frames & 3u) || ((uintptr_t)d_pics & 7u) || ((uintptr_t)d_prev & 7u))
    return fail(c, MI_DV_ERR_ARG, "%s: d_frames must be 4-byte, d_pics and d_prev 8-byte aligned", who);
  if (n_runs == 0 || !run_len) {  // one run
    n_runs = 1;
    run_len = &n;
  }
  long long sum = 0;
  for (int i = 0; i < n_runs; i++) {
    if (run_len[i] <= 0) return fail(c, MI_DV_ERR_ARG, "%s: run %d has %d frames", who, i, run_len[i]);
    sum += run_len[i];
  }
  if (sum != n) return fail(c, MI_DV_ERR_ARG, "%s: the %d runs hold %lld frames, the batch %d", who, n_runs, sum, n);
  if (d_prev) {
    const uintptr_t p0 = (uintptr_t)d_prev, p1 = p0 + (size_t)n_runs * r.pic_bytes, q0 = (uintptr_t)d_pics, q1 = q0 + (size_t)n * r.pic_bytes;
    if (p0 < q1 && q0 < p1) return fail(c, MI_DV_ERR_ARG, "%s: d_prev overlaps d_pics", who);
  }
  if (!c) return fail(c, MI_DV_ERR_ARG, "%s: NULL instance", who);
  if (!sta_mask) sta_mask = MI_DV_STA_ERRORS;
  DVCHK(c, hipSetDevice(c->device));
  mi_dv_ctx::Hold& h = c->hold;
  // a run has a source when it has an earlier picture of its own or one of d_prev
  std::vector<HoldChunkDev> chunks;
  std::vector<HoldRunDev> runs;
  uint32_t frame0 = 0;
  for (int i = 0; i < n_runs; i++) {
    const uint32_t len = (uint32_t)run_len[i];
    if (len >= 2u || d_prev) {
      runs.push_back({(uint32_t)chunks.size(), (len + kHoldChunk - 1u) / kHoldChunk});
      for (uint32_t rel = 0; rel < len; rel += kHoldChunk)
        chunks.push_back({frame0, rel, len - rel < (uint32_t)kHoldChunk ? len - rel : (uint32_t)kHoldChunk, (uint32_t)i});
    }
    frame0 += len;
  }
  const size_t chunk_bytes = chunks.size() * sizeof(HoldChunkDev), run_bytes = runs.size() * sizeof(HoldRunDev);
  if (!chunks.empty()) {
    const int rc = hold_buffers(c, chunk_bytes + run_bytes, chunks.size() * (size_t)r.nmb);
    if (rc != MI_DV_OK) return rc;
  }
  int rc = r.launch(c, who, d_frames, n, d_pics);
  if (rc != MI_DV_OK) return rc;
  h.counted = false;
  if (chunks.empty()) return MI_DV_OK;
  DVCHK(c, hipEventSynchronize(h.desc_done));  // (the last upload has left the pinned buffer; at once if there was none)
  memcpy(h.h_desc, chunks.data(), chunk_bytes);
  memcpy(h.h_desc + chunk_bytes, runs.data(), run_bytes);
  DVCHK(c, hipMemcpyAsync(h.d_desc, h.h_desc, chunk_bytes + run_bytes, hipMemcpyHostToDevice, c->stream));
  DVCHK(c, hipEventRecord(h.desc_done, c->stream));
  std::pair<hipEvent_t, hipEvent_t> ev;
  if (!c->ev_free.empty()) {
    ev = c->ev_free.back();
    c->ev_free.pop_back();
  } else {
    DVCHK(c, hipEventCreate(&ev.first));
    DVCHK(c, hipEventCreate(&ev.second));
  }
  h.ev_used.push_back(ev);
  if (h.ev_used.size() > 4096) {  // nobody asks for times: keep the newest
    c->ev_free.push_back(h.ev_used.front());
    h.ev_used.erase(h.ev_used.begin());
  }
  const HoldChunkDev* d_chunks = (const HoldChunkDev*)h.d_desc;
  const HoldRunDev* d_runs = (const HoldRunDev*)(h.d_desc + chunk_bytes);
  const uint32_t nchunks = (uint32_t)chunks.size(), nruns = (uint32_t)runs.size(), nmb = (uint32_t)r.nmb;
  const unsigned gx = (nmb + kHoldScanThreads - 1) / kHoldScanThreads;
  DVCHK(c, hipEventRecord(ev.first, c->stream));
  hipLaunchKernelGGL(k_dv_hold_mask, dim3((nmb + kHoldMaskMbs - 1u) / kHoldMaskMbs, nchunks < kHoldMaxGridY ? nchunks : kHoldMaxGridY), dim3(kHoldScanThreads), 0, c->stream,
                     (const uint8_t*)d_frames, (uint32_t)r.frame_bytes, nmb, d_chunks, nchunks, (uint32_t)sta_mask, h.d_mask);
  hipLaunchKernelGGL(k_dv_hold_carry, dim3(gx, nruns < kHoldMaxGridY ? nruns : kHoldMaxGridY), dim3(kHoldScanThreads), 0, c->stream,
                     d_runs, nruns, d_chunks, nmb, (const uint64_t*)h.d_mask, h.d_carry, h.d_held);
  r.hold_copy(c->stream, d_chunks, nchunks * (uint32_t)kHoldSubs, h.d_mask, h.d_carry, (uint8_t*)d_pics, (const uint8_t*)d_prev, h.d_held);
  DVCHK(c, hipGetLastError());
  DVCHK(c, hipEventRecord(ev.second, c->stream));
  h.counted = true;
  return MI_DV_OK;
}

// ---- the encoder ----
// n resident pictures of system r into n resident frames: every argument is checked before anything is launched
int encode_batch(mi_dv_ctx* c, const Row& r, const char* who, const void* d_pics, int n, void* d_frames, int flags) {
  if (!c || !d_pics || !d_frames || n <= 0) return fail(c, MI_DV_ERR_ARG, "%s: bad argument", who);
  if (n > 65535) return fail(c, MI_DV_ERR_ARG, "%s: %d pictures; at most 65535 per call (split the batch)", who, n);
  if (flags < 0 || flags > 3) return fail(c, MI_DV_ERR_ARG, "%s: flags %d; bit 0: 2-4-8 blocks, bit 1: classes", who, flags);
  if (((uintptr_t)d_frames & 3u) || ((uintptr_t)d_pics & 7u))
    return fail(c, MI_DV_ERR_ARG, "%s: d_frames must be 4-byte and d_pics 8-byte aligned", who);
  const uintptr_t p0 = (uintptr_t)d_pics, p1 = p0 + (size_t)n * r.pic_bytes, q0 = (uintptr_t)d_frames, q1 = q0 + (size_t)n * r.frame_bytes;
  if (p0 < q1 && q0 < p1) return fail(c, MI_DV_ERR_ARG, "%s: d_frames overlaps d_pics", who);
  DVCHK(c, hipSetDevice(c->device));
  return r.encode(c, d_pics, n, d_frames, flags);
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

// ---- macroblocks flagged as errors keep the stream's last good pixels ----

int mi_dv_mb_rects(int system, int seq, int slot, int m, int rect[3][4]) {
  const Row* r = find(system);
  if (!rect || !r || seq < 0 || seq >= r->place_seqs || slot < 0 || slot >= 27 || m < 0 || m >= 5)
    return fail(nullptr, MI_DV_ERR_ARG, "mi_dv_mb_rects: system %d, sequence %d, segment %d, macroblock %d out of range", system, seq, slot, m);
  Rect q[3];
  r->rects((uint32_t)seq, (uint32_t)slot, (uint32_t)m, q);
  for (int pl = 0; pl < 3; pl++) {
    rect[pl][0] = (int)q[pl].x;
    rect[pl][1] = (int)q[pl].y;
    rect[pl][2] = (int)q[pl].w;
    rect[pl][3] = (int)q[pl].h;
  }
  return MI_DV_OK;
}

int mi_dv_held_macroblocks(int system, const uint8_t* frame, size_t len, unsigned sta_mask) {
  const Row* r = find(system);
  if (!r) return fail(nullptr, MI_DV_ERR_ARG, "mi_dv_held_macroblocks: unknown system %d", system);
  if (sta_mask > 0xFFFFu) return fail(nullptr, MI_DV_ERR_ARG, "mi_dv_held_macroblocks: STA mask 0x%x: at most 0xFFFF", sta_mask);
  if (!frame || len < (size_t)r->frame_bytes)
    return fail(nullptr, MI_DV_ERR_ARG, "mi_dv_held_macroblocks: %s frames have %d bytes", r->frames, r->frame_bytes);
  if (!sta_mask) sta_mask = MI_DV_STA_ERRORS;
  int held = 0;
  for (int seq = 0; seq < r->place_seqs; seq++)
    for (int v = 0; v < 135; v++) held += (int)(sta_mask >> (frame[(size_t)(seq * 150 + 7 + v + v / 15) * 80 + 3] >> 4) & 1u);
  return held;
}

int mi_dv_decode_batch_held(mi_dv_ctx* c, int system, const void* d_frames, int n, void* d_pics, int n_runs, const int* run_len,
                            const void* d_prev, unsigned sta_mask) {
  const Row* r = find(system);
  if (!r) return fail(c, MI_DV_ERR_ARG, "mi_dv_decode_batch_held: unknown system %d", system);
  return decode_held(c, *r, "mi_dv_decode_batch_held", d_frames, n, d_pics, n_runs, run_len, d_prev, sta_mask);
}

int mi_dv_hold_stats(mi_dv_ctx* c, long long* held) {
  if (!c || !held) return MI_DV_ERR_ARG;
  DVCHK(c, hipSetDevice(c->device));
  DVCHK(c, hipStreamSynchronize(c->stream));
  unsigned long long v = 0;
  if (c->hold.counted) {  // the partial counts (dv_hold_kernels.h: kHoldCounters)
    std::vector<unsigned long long> part((size_t)kHoldCounters * kHoldCounterStride);
    DVCHK(c, hipMemcpyAsync(part.data(), c->hold.d_held, part.size() * sizeof part[0], hipMemcpyDeviceToHost, c->stream));
    DVCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < kHoldCounters; i++) v += part[(size_t)i * kHoldCounterStride];
  }
  *held = (long long)v;
  return MI_DV_OK;
}

int mi_dv_hold_times(mi_dv_ctx* c, float* total_ms, int* launches) {
  if (!c || !total_ms || !launches) return MI_DV_ERR_ARG;
  DVCHK(c, hipSetDevice(c->device));
  DVCHK(c, hipStreamSynchronize(c->stream));
  float sum = 0.f;
  for (auto& e : c->hold.ev_used) {
    float ms = 0.f;
    DVCHK(c, hipEventElapsedTime(&ms, e.first, e.second));
    sum += ms;
  }
  *total_ms = sum;
  *launches = 3 * (int)c->hold.ev_used.size();  // k_dv_hold_mask, k_dv_hold_carry, k_dv_hold_copy
  for (auto& e : c->hold.ev_used) c->ev_free.push_back(e);
  c->hold.ev_used.clear();
  return MI_DV_OK;
}

int mi_dv_hold_reset(mi_dv_ctx* c) {
  if (!c) return MI_DV_ERR_ARG;
  hold_forget(c);
  return MI_DV_OK;
}

int mi_dv_decode_frame_held(mi_dv_ctx* c, int system, const uint8_t* frame, size_t len, uint8_t* const planes[3],
                            const int strides[3], unsigned sta_mask, int* held) {
  const char* who = "mi_dv_decode_frame_held";
  // a refused frame, and one that failed on the way, leave no picture behind: the next frame has no source
  const Row* r = find(system);
  int rc = !r ? fail(c, MI_DV_ERR_ARG, "%s: unknown system %d", who, system)
           : sta_mask > 0xFFFFu ? fail(c, MI_DV_ERR_ARG, "%s: STA mask 0x%x: one bit per STA value, at most 0xFFFF", who, sta_mask)
                                : check_one(c, *r, who, frame, len, planes, strides);
  if (rc != MI_DV_OK) {
    hold_forget(c);
    return rc;
  }
  mi_dv_ctx::Hold& h = c->hold;
  const int id = r->id;
  const bool had = h.kept == id;
  hold_forget(c);  // (until this frame's picture is there; a picture of another system is no source for a later frame)
  DVCHK(c, hipSetDevice(c->device));
  rc = one_frame_buffers(c, (size_t)r->frame_bytes, (size_t)r->pic_bytes);
  if (rc != MI_DV_OK) return rc;
  for (uint8_t*& d : h.keep[id])
    if (!d) DVCHK(c, hipMalloc((void**)&d, (size_t)r->pic_bytes));
  uint8_t* const last = h.keep[id][h.cur[id]];
  uint8_t* const now = h.keep[id][h.cur[id] ^ 1];
  DVCHK(c, hipMemcpyAsync(c->d_frame, frame, (size_t)r->frame_bytes, hipMemcpyHostToDevice, c->stream));
  rc = decode_held(c, *r, who, c->d_frame, 1, now, 0, nullptr, had ? last : nullptr, sta_mask);
  if (rc != MI_DV_OK) return rc;
  rc = planes_out(c, *r, now, planes, strides);
  if (rc != MI_DV_OK) return rc;
  if (held) {
    long long v = 0;
    rc = mi_dv_hold_stats(c, &v);
    if (rc != MI_DV_OK) return rc;
    *held = (int)v;
  }
  h.cur[id] ^= 1;
  h.kept = id;
  return MI_DV_OK;
}

// ---- the encoder ----

int mi_dv_encode_batch(mi_dv_ctx* c, int system, const void* d_pics, int n, void* d_frames, int flags) {
  const Row* r = find(system);
  if (!r) return fail(c, MI_DV_ERR_ARG, "mi_dv_encode_batch: unknown system %d", system);
  return encode_batch(c, *r, "mi_dv_encode_batch", d_pics, n, d_frames, flags);
}

int mi_dv_encode_frame(mi_dv_ctx* c, int system, const uint8_t* const planes[3], const int strides[3], uint8_t* frame, size_t cap,
                       int flags) {
  const char* who = "mi_dv_encode_frame";
  const Row* r = find(system);
  if (!r) return fail(c, MI_DV_ERR_ARG, "%s: unknown system %d", who, system);
  if (!c || !frame || !planes || !strides || !planes[0] || !planes[1] || !planes[2]) return fail(c, MI_DV_ERR_ARG, "%s: NULL argument", who);
  if (cap < (size_t)r->frame_bytes)
    return fail(c, MI_DV_ERR_ARG, "%s: room for %zu bytes: %s frames have %d", who, cap, r->frames, r->frame_bytes);
  if (flags < 0 || flags > 3) return fail(c, MI_DV_ERR_ARG, "%s: flags %d; bit 0: 2-4-8 blocks, bit 1: classes", who, flags);
  if (strides[0] < r->w[0] || strides[1] < r->w[1] || strides[2] < r->w[2]) return fail(c, MI_DV_ERR_ARG, "strides below the picture's width");
  DVCHK(c, hipSetDevice(c->device));
  int rc = one_frame_buffers(c, (size_t)r->frame_bytes, (size_t)r->pic_bytes);
  if (rc != MI_DV_OK) return rc;
  DVCHK(c, hipStreamSynchronize(c->stream));  // (the pinned picture is free)
  uint8_t* dst = c->h_pic;
  for (int pl = 0; pl < 3; pl++) {
    const int w = r->w[pl], h = r->h[pl];
    for (int y = 0; y < h; y++) memcpy(dst + (size_t)y * w, planes[pl] + (size_t)y * strides[pl], (size_t)w);
    dst += (size_t)w * h;
  }
  DVCHK(c, hipMemcpyAsync(c->d_pic, c->h_pic, (size_t)r->pic_bytes, hipMemcpyHostToDevice, c->stream));
  rc = encode_batch(c, *r, who, c->d_pic, 1, c->d_frame, flags);
  if (rc != MI_DV_OK) return rc;
  DVCHK(c, hipMemcpyAsync(frame, c->d_frame, (size_t)r->frame_bytes, hipMemcpyDeviceToHost, c->stream));
  DVCHK(c, hipStreamSynchronize(c->stream));
  return MI_DV_OK;
}

int mi_dv_encode_times(mi_dv_ctx* c, float* total_ms, int* launches) {
  if (!c || !total_ms || !launches) return MI_DV_ERR_ARG;
  DVCHK(c, hipSetDevice(c->device));
  DVCHK(c, hipStreamSynchronize(c->stream));
  float sum = 0.f;
  for (auto& e : c->enc_ev_used) {
    float ms = 0.f;
    DVCHK(c, hipEventElapsedTime(&ms, e.first, e.second));
    sum += ms;
  }
  *total_ms = sum;
  *launches = (int)c->enc_ev_used.size();
  for (auto& e : c->enc_ev_used) c->ev_free.push_back(e);
  c->enc_ev_used.clear();
  return MI_DV_OK;
}

int mi_dv_encode_stats(mi_dv_ctx* c, long long qno_hist[16], long long* dropped) {
  if (!c || !qno_hist || !dropped) return MI_DV_ERR_ARG;
  DVCHK(c, hipSetDevice(c->device));
  DVCHK(c, hipStreamSynchronize(c->stream));
  unsigned long long v[kEncStats];
  DVCHK(c, hipMemcpyAsync(v, c->d_enc_stats, sizeof v, hipMemcpyDeviceToHost, c->stream));
  DVCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < 16; i++) qno_hist[i] = (long long)v[i];
  *dropped = (long long)v[16];
  return MI_DV_OK;
}

}  // extern "C"
