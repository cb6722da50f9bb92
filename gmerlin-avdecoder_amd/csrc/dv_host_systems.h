// dv_host_systems.h — the five systems as the host layer sees them (one table), the instance, and the decoder's calls:
// the checks of a resident batch, the decode launch, the one-frame path.  Included by mi_dv.hip; not a kernel header.
// (The held calls, the encoder, the sound and the timecode have headers of their own behind this one.)
#pragma once
#include <stdio.h>
#include <string.h>

#include <iterator>

#include "dv_common.h"
#include "dv_decode_kernels.h"
#include "dv_hold_kernels.h"
#include "dv_encode_kernels.h"
#include "dv_audio_kernels.h"
#include "dv_meta_kernels.h"
#include "../../include/mi_dv.h"
#include "host_base.h"

using namespace midv;

namespace {
#ifdef MIDV_DEBUG
void* g_dbg = nullptr;  // mi_dv_debug_buffer
#endif

// ---- the five systems, once: what the entry points need of each (generated from csrc/dv_common.h's Sys*) ----
struct Row {
  int id, frame_bytes, pic_bytes, w[3], h[3];  // the planes Y, Cb, Cr
  int place_seqs;                              // the sequences mi_dv_mb_place takes: both channels', in byte order
  // what the one-frame path's messages say: "<frames> frames have ...", "not a <what> (DSF ..., [APT ...,] stype ...<expected>)"
  const char *frames, *what, *expected;
  bool says_apt;
  void (*decode)(hipStream_t, const uint8_t*, unsigned, uint8_t*, const Tables*);  // the launch of k_dv_decode<Sys>
  void (*place)(uint32_t, uint32_t, uint32_t, uint32_t&, uint32_t&);
  // the held calls: macroblocks per frame, a macroblock's three rectangles, the launch of k_dv_hold_copy<Sys>
  int nmb;
  void (*rects)(uint32_t, uint32_t, uint32_t, Rect*);
  void (*hold_copy)(hipStream_t, const HoldChunkDev*, uint32_t, const uint64_t*, const int32_t*, uint8_t*, const uint8_t*,
                    unsigned long long*);
  // the launch of k_dv_encode<Sys>
  void (*encode)(hipStream_t, const uint8_t*, unsigned, uint8_t*, const EncTables*, uint32_t, unsigned long long*);
  // the sound: DIF channels (the stereo pairs of 16-bit sound), the line system (the row of AudioTables), the frame rate
  // as a fraction, the launches of k_dv_audio_extract<Sys> and k_dv_audio_write<Sys>
  int chans, line, rate_num, rate_den;
  void (*audio_extract)(hipStream_t, const uint8_t*, unsigned, uint8_t*, uint32_t, int32_t*, const AudioTables*);
  void (*audio_write)(hipStream_t, uint8_t*, unsigned, const uint8_t*, uint32_t, uint32_t, const int32_t*, const AudioTables*);
  // timecode, recording date and time, aspect: the launches of k_dv_meta_extract<Sys> and k_dv_meta_write<Sys>
  void (*meta_extract)(hipStream_t, const uint8_t*, unsigned, int32_t*);
  void (*meta_write)(hipStream_t, uint8_t*, unsigned, unsigned long long, uint32_t, long long, uint32_t);
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
// the launches: all that depends on the system's type.  Checks, events and errors are their callers'
template <class S>
void decode_launch(hipStream_t st, const uint8_t* frames, unsigned n, uint8_t* pics, const Tables* tab) {
  hipLaunchKernelGGL(k_dv_decode<S>, dim3(kDvGridX<S>, n), dim3(64 * kDvWaves), 0, st, frames, pics, tab
#ifdef MIDV_DEBUG
                     , (int16_t*)g_dbg
#endif
  );
}
// one workgroup per (super block, kHoldSub pictures of a chunk); past 65535 items the kernel strides
template <class S>
void hold_copy_launch(hipStream_t st, const HoldChunkDev* chunks, uint32_t nitems, const uint64_t* mask, const int32_t* carry,
                      uint8_t* pics, const uint8_t* prev, unsigned long long* held) {
  hipLaunchKernelGGL(k_dv_hold_copy<S>, dim3((unsigned)(S::kChans * S::kSeqs * 5), nitems < kHoldMaxGridY ? nitems : kHoldMaxGridY),
                     dim3(kHoldCopyThreads), 0, st, chunks, nitems, mask, carry, pics, prev, held);
}
template <class S>
void encode_launch(hipStream_t st, const uint8_t* pics, unsigned n, uint8_t* frames, const EncTables* tab, uint32_t flags,
                   unsigned long long* stats) {
  hipLaunchKernelGGL(k_dv_encode<S>, dim3(kEncGridX<S>, n), dim3(64), 0, st, pics, frames, tab, flags, stats);
}
// one workgroup per (pair of the output, frame) / per (channel, frame)
template <class S>
void audio_extract_launch(hipStream_t st, const uint8_t* frames, unsigned n, uint8_t* pcm, uint32_t pairs, int32_t* info,
                          const AudioTables* tab) {
  hipLaunchKernelGGL(k_dv_audio_extract<S>, dim3(pairs, n), dim3(kAudioThreads), 0, st, frames, pcm, pairs, info, tab);
}
template <class S>
void audio_write_launch(hipStream_t st, uint8_t* frames, unsigned n, const uint8_t* pcm, uint32_t pairs, uint32_t freq,
                        const int32_t* samples, const AudioTables* tab) {
  hipLaunchKernelGGL(k_dv_audio_write<S>, dim3((unsigned)S::kChans, n), dim3(kAudioThreads), 0, st, frames, pcm, pairs, freq, samples, tab);
}
// one wave per frame, kMetaExtractWaves of them a workgroup (the last may be partly idle) / one workgroup per frame
template <class S>
void meta_extract_launch(hipStream_t st, const uint8_t* frames, unsigned n, int32_t* meta) {
  hipLaunchKernelGGL(k_dv_meta_extract<S>, dim3((n + kMetaExtractWaves - 1u) / kMetaExtractWaves), dim3(64 * kMetaExtractWaves), 0, st,
                     frames, (uint32_t)n, meta);
}
template <class S>
void meta_write_launch(hipStream_t st, uint8_t* frames, unsigned n, unsigned long long first_frame, uint32_t drop,
                       long long rec_seconds, uint32_t wide) {
  hipLaunchKernelGGL(k_dv_meta_write<S>, dim3(n), dim3(kMetaWriteThreads), 0, st, frames, first_frame, drop, rec_seconds, wide);
}
template <class S>
constexpr Row row(const char* frames, const char* what, bool says_apt, const char* expected) {
  return {S::kId, S::kFrameBytes, S::kPicBytes, {S::kW, S::kCW, S::kCW}, {S::kH, S::kCH, S::kCH}, S::kChans * S::kSeqs,
          frames, what, expected, says_apt, decode_launch<S>, place_thunk<S>, S::kSegments * 5, rects_thunk<S>, hold_copy_launch<S>,
          encode_launch<S>, S::kChans, S::kSeqs == 12 ? 1 : 0, S::kSeqs == 12 ? 25 : 30000, S::kSeqs == 12 ? 1 : 1001,
          audio_extract_launch<S>, audio_write_launch<S>, meta_extract_launch<S>, meta_write_launch<S>};
}
constexpr Row kSystems[] = {
    row<Sys525>("525/60", "525/60 25 Mbit/s DV frame", false, ""),
    row<Sys625>("625/50", "625/50 25 Mbit/s 4:2:0 DV frame", true, ""),
    row<Sys625_411>("625/50 4:1:1", "625/50 25 Mbit/s 4:1:1 (DVCPRO) DV frame", true, "; expected DSF 1, APT not 0, stype 0x00"),
    row<Sys525_422>("525/60 50 Mbit/s 4:2:2", "525/60 50 Mbit/s 4:2:2 DV frame of 240000 bytes", false, "; expected DSF 0, stype 0x04"),
    row<Sys625_422>("625/50 50 Mbit/s 4:2:2", "625/50 50 Mbit/s 4:2:2 DV frame of 288000 bytes", false, "; expected DSF 1, stype 0x04"),
};
constexpr size_t kNumSystems = std::size(kSystems);
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
}  // namespace

// ---- the instance: device, stream and error text are HostCtx's (host_base.h), destroyed after everything here.  The
// timers go before the pool they hand their pairs to.  (Hidden: the library exports the C ABI, not this struct's
// constructor and destructor) ----
struct __attribute__((visibility("hidden"))) mi_dv_ctx : HostCtx {
  EventPool ev_free;
  DevBuf<Tables> d_tab;
  Timer decode_time{ev_free};  // k_dv_decode (mi_dv_kernel_times)
  // the encoder (mi_dv_encode_*): its tables, the last batch's counts (kEncStats)
  DevBuf<EncTables> d_enc;
  DevBuf<unsigned long long> d_enc_stats;
  Timer encode_time{ev_free};  // k_dv_encode (mi_dv_encode_times)
  // the sound (mi_dv_audio_*): its table; the sample counts of the last written batch on their way to the device
  struct Audio {
    explicit Audio(EventPool& pool) : time(pool) {}
    Timer time;  // k_dv_audio_extract and k_dv_audio_write (mi_dv_audio_times)
    DevBuf<AudioTables> d_tab;
    PinnedBuf<int32_t> h_samples;
    DevBuf<int32_t> d_samples;
    Event samples_done;  // behind the last upload of h_samples
  } audio{ev_free};
  // timecode, recording date and time, aspect (mi_dv_meta_*)
  struct Meta {
    explicit Meta(EventPool& pool) : time(pool) {}
    Timer time;  // k_dv_meta_extract and k_dv_meta_write (mi_dv_meta_times)
  } meta{ev_free};
  // the one-frame paths' buffers, shared by mi_dv_decode_frame*, mi_dv_decode_frame_held and mi_dv_encode_frame: as large
  // as the largest system this instance has seen needs them
  DevBuf<uint8_t> d_frame, d_pic;
  PinnedBuf<uint8_t> h_pic;
  // the held calls (mi_dv_decode_batch_held, mi_dv_decode_frame_held).  Everything only grows.
  struct Hold {
    explicit Hold(EventPool& pool) : time(pool) {}
    Timer time;                 // phase 2 (mi_dv_hold_times)
    PinnedBuf<uint8_t> h_desc;  // the chunks, then the runs, of the last batch
    DevBuf<uint8_t> d_desc;
    Event desc_done;            // behind the last upload of h_desc
    DevBuf<uint64_t> d_mask;    // [chunk][macroblock]
    DevBuf<int32_t> d_carry;
    DevBuf<unsigned long long> d_held;  // kHoldCounters partial counts
    bool counted = false;  // the last held batch ran phase 2: d_held is its count (else the count is 0)
    // the one-frame path, per row of kSystems: the last picture and the one being made, in turns; the row whose
    // keep[][cur] is the picture of the frame decoded last (-1: none; the next frame has no source)
    DevBuf<uint8_t> keep[kNumSystems][2];
    int cur[kNumSystems] = {};
    int kept = -1;
  } hold{ev_free};
};

namespace {
// ---- a resident batch, checked.  Every entry point makes these checks in this order, with its own between them ----
struct BatchCheck {
  mi_dv_ctx* c;
  const char* who;  // the entry point the messages name
  // have: the instance (where it is named here) and the buffers are there; items: "frames" / "pictures"
  int count(bool have, int n, const char* items) const {
    if (!have || n <= 0) return fail(c, MI_DV_ERR_ARG, "%s: bad argument", who);
    if (n > 65535) return fail(c, MI_DV_ERR_ARG, "%s: %d %s; at most 65535 per call (split the batch)", who, n, items);
    return MI_DV_OK;
  }
  // frames on 4 bytes, pictures (d_prev: NULL or more pictures) on 8; rule: how the message puts it
  int aligned(const void* d_frames, const void* d_pics, const void* d_prev, const char* rule) const {
    if (((uintptr_t)d_frames & 3u) || (((uintptr_t)d_pics | (uintptr_t)d_prev) & 7u))
      return fail(c, MI_DV_ERR_ARG, "%s: d_frames must be %s aligned", who, rule);
    return MI_DV_OK;
  }
  // p on `to` bytes (a power of two)
  int on(const void* p, unsigned to, const char* name) const {
    if ((uintptr_t)p & (uintptr_t)(to - 1u)) return fail(c, MI_DV_ERR_ARG, "%s: %s must be %u-byte aligned", who, name, to);
    return MI_DV_OK;
  }
  // `a_bytes` at a and `b_bytes` at b share no byte
  int apart(const void* a, size_t a_bytes, const char* a_name, const void* b, size_t b_bytes, const char* b_name) const {
    const uintptr_t p0 = (uintptr_t)a, p1 = p0 + a_bytes, q0 = (uintptr_t)b, q1 = q0 + b_bytes;
    if (p0 < q1 && q0 < p1) return fail(c, MI_DV_ERR_ARG, "%s: %s overlaps %s", who, a_name, b_name);
    return MI_DV_OK;
  }
};

// ---- the decoder ----
// k_dv_decode of system r over n resident frames, timed; the arguments are checked by the caller
int decode_run(mi_dv_ctx* c, const Row& r, const void* d_frames, int n, void* d_pics) {
  int rc = c->decode_time.begin(c, c->stream);
  if (rc != MI_DV_OK) return rc;
  r.decode(c->stream, (const uint8_t*)d_frames, (unsigned)n, (uint8_t*)d_pics, c->d_tab);
  HIPCHK(c, hipGetLastError());
  return c->decode_time.end(c, c->stream);
}
int decode_batch(mi_dv_ctx* c, const Row& r, const char* who, const void* d_frames, int n, void* d_pics) {
  const BatchCheck k{c, who};
  int rc = k.count(c && d_frames && d_pics, n, "frames");
  if (rc == MI_DV_OK) rc = k.aligned(d_frames, d_pics, nullptr, "4-byte and d_pics 8-byte");
  if (rc != MI_DV_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return decode_run(c, r, d_frames, n, d_pics);
}

// ---- the one-frame paths ----
// their buffers hold a frame and a picture of system r (they only grow; the stream is idle between these calls, so
// nothing is waited for)
int one_frame_buffers(mi_dv_ctx* c, const Row& r) {
  int rc = c->d_frame.grow(c, (uint64_t)r.frame_bytes, nullptr);
  if (rc == MI_DV_OK && (uint64_t)r.pic_bytes > c->h_pic.cap) {  // (the last of the two to grow)
    c->d_pic.release();
    c->h_pic.release();
    rc = c->d_pic.grow(c, (uint64_t)r.pic_bytes, nullptr);
    if (rc == MI_DV_OK) rc = c->h_pic.grow(c, (uint64_t)r.pic_bytes, nullptr);
  }
  return rc;
}
bool has_planes(const uint8_t* const planes[3], const int strides[3]) {
  return planes && strides && planes[0] && planes[1] && planes[2];
}
int check_strides(mi_dv_ctx* c, const Row& r, const int strides[3]) {
  if (strides[0] < r.w[0] || strides[1] < r.w[1] || strides[2] < r.w[2]) return fail(c, MI_DV_ERR_ARG, "strides below the picture's width");
  return MI_DV_OK;
}
// a tightly packed picture of system r and the caller's planes: out of the picture into the planes, or back
void copy_planes(const Row& r, uint8_t* pic, uint8_t* const planes[3], const int strides[3], bool into_planes) {
  for (int pl = 0; pl < 3; pl++) {
    const int w = r.w[pl], h = r.h[pl];
    for (int y = 0; y < h; y++) {
      uint8_t *row = planes[pl] + (size_t)y * strides[pl], *packed = pic + (size_t)y * w;
      memcpy(into_planes ? row : packed, into_planes ? packed : row, (size_t)w);
    }
    pic += (size_t)w * h;
  }
}

// one host frame of system r, checked: arguments, length, announcement, strides, in this order
int check_one(mi_dv_ctx* c, const Row& r, const char* who, const uint8_t* frame, size_t len, uint8_t* const planes[3],
              const int strides[3]) {
  if (!c || !frame || !has_planes(planes, strides)) return fail(c, MI_DV_ERR_ARG, "%s: NULL argument", who);
  if (len < (size_t)r.frame_bytes)
    return fail(c, MI_DV_ERR_FORMAT, "DIF frame of %zu bytes: %s frames have %d", len, r.frames, r.frame_bytes);
  if (classify(frame, len) != r.id) {
    const int dsf = frame[3] >> 7, apt = frame[5] & 7, stype = frame[80 * 5 + 48 + 3] & 0x1f;
    char seen[64];
    if (r.says_apt) snprintf(seen, sizeof seen, "DSF %d, APT %d, stype 0x%02x", dsf, apt, stype);
    else snprintf(seen, sizeof seen, "DSF %d, stype 0x%02x", dsf, stype);
    return fail(c, MI_DV_ERR_FORMAT, "not a %s (%s%s)", r.what, seen, r.expected);
  }
  return check_strides(c, r, strides);
}

// the device picture d_pic of system r through the pinned buffer into the caller's planes; synchronises
int planes_out(mi_dv_ctx* c, const Row& r, const uint8_t* d_pic, uint8_t* const planes[3], const int strides[3]) {
  HIPCHK(c, hipMemcpyAsync(c->h_pic, d_pic, (size_t)r.pic_bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  copy_planes(r, c->h_pic, planes, strides, true);
  return MI_DV_OK;
}

// one host frame of system r, checked, through the kernel into the caller's planes
int decode_one(mi_dv_ctx* c, const Row& r, const char* who, const uint8_t* frame, size_t len, uint8_t* const planes[3],
               const int strides[3]) {
  int rc = check_one(c, r, who, frame, len, planes, strides);
  if (rc != MI_DV_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  rc = one_frame_buffers(c, r);
  if (rc != MI_DV_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(c->d_frame, frame, (size_t)r.frame_bytes, hipMemcpyHostToDevice, c->stream));
  rc = decode_batch(c, r, who, c->d_frame, 1, c->d_pic);
  if (rc != MI_DV_OK) return rc;
  return planes_out(c, r, c->d_pic, planes, strides);
}
}  // namespace
