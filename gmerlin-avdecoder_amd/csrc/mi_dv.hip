// mi_dv.hip — C ABI (include/mi_dv.h) of the MI355X DV decoder and encoder (25 Mbit/s: 525/60 4:1:1, 625/50 4:2:0, 625/50 4:1:1;
// 50 Mbit/s: both line systems in 4:2:2).  No CPU path: without a gfx950 device every call fails with a message.
// The entry points only; what they call: host_base.h (shared with the other device libraries: owned buffers, errors, the
// timer, the bodies of the calls every library has), dv_host_systems.h (the table of systems, the instance, the
// decoder), dv_host_hold.h (the held calls), dv_host_encode.h (the encoder), dv_host_audio.h (the sound),
// dv_host_meta.h (timecode, recording date and time, aspect).
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/mi_dv.h"
#include "dv_host_systems.h"
#include "dv_host_hold.h"
#include "dv_host_encode.h"
#include "dv_host_audio.h"
#include "dv_host_meta.h"

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
static_assert(kSystems[0].id == MI_DV_SYS_525_60, "mi_dv_decode_batch and mi_dv_decode_frame take the table's first row");

static_assert(MI_DV_OK == kOk && MI_DV_ERR_HIP == kErrHip, "header and host base agree");

extern "C" {

int mi_dv_device_count(void) { return device_count(); }

const char* mi_dv_last_error(const mi_dv_ctx* c) { return last_error(c); }

mi_dv_ctx* mi_dv_create(int device) {
  if ((device = usable_device(device, "DV decoder", MI_DV_ERR_ARG)) < 0) return nullptr;
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
  AudioTables at;
  build_audio_tables(&at);
  mi_dv_ctx* c = new mi_dv_ctx();
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream.p, hipStreamNonBlocking) != hipSuccess ||
      c->d_tab.grow(c, 1, nullptr) != MI_DV_OK || hipMemcpy(c->d_tab, &t, sizeof t, hipMemcpyHostToDevice) != hipSuccess ||
      c->d_enc.grow(c, 1, nullptr) != MI_DV_OK || hipMemcpy(c->d_enc, &et, sizeof et, hipMemcpyHostToDevice) != hipSuccess ||
      c->audio.d_tab.grow(c, 1, nullptr) != MI_DV_OK || hipMemcpy(c->audio.d_tab, &at, sizeof at, hipMemcpyHostToDevice) != hipSuccess ||
      c->d_enc_stats.grow(c, kEncStats, nullptr) != MI_DV_OK ||
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
  delete c;  // (buffers and events, then HostCtx's stream)
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
void mi_dv_dev_free(mi_dv_ctx* c, void* d) { dev_free(c, d); }
int mi_dv_h2d(mi_dv_ctx* c, void* d, const void* h, size_t n) {
  if (!c || (!d && n) || (!h && n)) return fail(c, MI_DV_ERR_ARG, "mi_dv_h2d: NULL argument");
  return copy_sync(c, d, h, n, hipMemcpyHostToDevice);
}
int mi_dv_d2h(mi_dv_ctx* c, void* h, const void* d, size_t n) {
  if (!c || (!d && n) || (!h && n)) return fail(c, MI_DV_ERR_ARG, "mi_dv_d2h: NULL argument");
  return copy_sync(c, h, d, n, hipMemcpyDeviceToHost);
}
int mi_dv_sync(mi_dv_ctx* c) { return c ? stream_sync(c) : MI_DV_ERR_ARG; }

#ifdef MIDV_DEBUG
void mi_dv_debug_buffer(void* d) { g_dbg = d; }
#endif

int mi_dv_decode_batch(mi_dv_ctx* c, const void* d_frames, int n, void* d_pics) {
  return decode_batch(c, kSystems[0], "mi_dv_decode_batch", d_frames, n, d_pics);
}

int mi_dv_decode_batch_sys(mi_dv_ctx* c, int system, const void* d_frames, int n, void* d_pics) {
  const Row* r = find(system);
  if (!r) return fail(c, MI_DV_ERR_ARG, "mi_dv_decode_batch_sys: unknown system %d", system);
  return decode_batch(c, *r, "mi_dv_decode_batch_sys", d_frames, n, d_pics);
}

int mi_dv_kernel_times(mi_dv_ctx* c, float* total_ms, int* launches) {
  return times(c, c ? &c->decode_time : nullptr, 1, total_ms, launches, MI_DV_ERR_ARG);
}

size_t mi_dv_copy_tables(void* out, size_t cap) {
  Tables t;
  if (!build_tables(&t)) return 0;
  if (out && cap >= sizeof t) memcpy(out, &t, sizeof t);
  return sizeof t;
}

int mi_dv_decode_frame(mi_dv_ctx* c, const uint8_t* frame, size_t len, uint8_t* const planes[3], const int strides[3]) {
  return decode_one(c, kSystems[0], "mi_dv_decode_frame", frame, len, planes, strides);
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
  return hold_count(c, held);
}

int mi_dv_hold_times(mi_dv_ctx* c, float* total_ms, int* launches) {  // k_dv_hold_mask, k_dv_hold_carry, k_dv_hold_copy
  return times(c, c ? &c->hold.time : nullptr, 3, total_ms, launches, MI_DV_ERR_ARG);
}

int mi_dv_hold_reset(mi_dv_ctx* c) {
  if (!c) return MI_DV_ERR_ARG;
  hold_forget(c);
  return MI_DV_OK;
}

int mi_dv_decode_frame_held(mi_dv_ctx* c, int system, const uint8_t* frame, size_t len, uint8_t* const planes[3],
                            const int strides[3], unsigned sta_mask, int* held) {
  return decode_one_held(c, find(system), system, frame, len, planes, strides, sta_mask, held);
}

// ---- the encoder ----

int mi_dv_encode_batch(mi_dv_ctx* c, int system, const void* d_pics, int n, void* d_frames, int flags) {
  const Row* r = find(system);
  if (!r) return fail(c, MI_DV_ERR_ARG, "mi_dv_encode_batch: unknown system %d", system);
  return encode_batch(c, *r, "mi_dv_encode_batch", d_pics, n, d_frames, flags);
}

int mi_dv_encode_frame(mi_dv_ctx* c, int system, const uint8_t* const planes[3], const int strides[3], uint8_t* frame, size_t cap,
                       int flags) {
  const Row* r = find(system);
  if (!r) return fail(c, MI_DV_ERR_ARG, "mi_dv_encode_frame: unknown system %d", system);
  return encode_one(c, *r, "mi_dv_encode_frame", planes, strides, frame, cap, flags);
}

int mi_dv_encode_times(mi_dv_ctx* c, float* total_ms, int* launches) {
  return times(c, c ? &c->encode_time : nullptr, 1, total_ms, launches, MI_DV_ERR_ARG);
}

int mi_dv_encode_stats(mi_dv_ctx* c, long long qno_hist[16], long long* dropped) {
  if (!c || !qno_hist || !dropped) return MI_DV_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  unsigned long long v[kEncStats];
  HIPCHK(c, hipMemcpyAsync(v, c->d_enc_stats, sizeof v, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < 16; i++) qno_hist[i] = (long long)v[i];
  *dropped = (long long)v[16];
  return MI_DV_OK;
}

// ---- the sound ----

int mi_dv_audio_batch(mi_dv_ctx* c, int system, const void* d_frames, int n, void* d_pcm, int pairs, void* d_info) {
  const Row* r = find(system);
  if (!r) return fail(c, MI_DV_ERR_ARG, "mi_dv_audio_batch: unknown system %d", system);
  return audio_batch(c, *r, "mi_dv_audio_batch", d_frames, n, d_pcm, pairs, d_info);
}

int mi_dv_audio_write_batch(mi_dv_ctx* c, int system, void* d_frames, int n, const void* d_pcm, int pairs, int samplerate,
                            const int* samples) {
  const Row* r = find(system);
  if (!r) return fail(c, MI_DV_ERR_ARG, "mi_dv_audio_write_batch: unknown system %d", system);
  return audio_write_batch(c, *r, "mi_dv_audio_write_batch", d_frames, n, d_pcm, pairs, samplerate, samples);
}

int mi_dv_audio_samples(int system, int samplerate, long long frame) {
  const Row* r = find(system);
  if (!r || audio_freq(samplerate) < 0 || frame < 0 || frame > (1ll << 31))
    return fail(nullptr, MI_DV_ERR_ARG, "mi_dv_audio_samples: system %d, %d Hz, frame %lld out of range", system, samplerate, frame);
  return audio_cadence(*r, samplerate, frame);
}

int mi_dv_audio_times(mi_dv_ctx* c, float* total_ms, int* launches) {  // k_dv_audio_extract, k_dv_audio_write
  return times(c, c ? &c->audio.time : nullptr, 1, total_ms, launches, MI_DV_ERR_ARG);
}

size_t mi_dv_audio_copy_tables(void* out, size_t cap) {
  AudioTables t;
  build_audio_tables(&t);
  if (out && cap >= sizeof t) memcpy(out, &t, sizeof t);
  return sizeof t;
}

// ---- timecode, recording date and time, aspect ----

int mi_dv_meta_batch(mi_dv_ctx* c, int system, const void* d_frames, int n, void* d_meta) {
  const Row* r = find(system);
  if (!r) return fail(c, MI_DV_ERR_ARG, "mi_dv_meta_batch: unknown system %d", system);
  return meta_batch(c, *r, "mi_dv_meta_batch", d_frames, n, d_meta);
}

int mi_dv_meta_write_batch(mi_dv_ctx* c, int system, void* d_frames, int n, long long first_frame, int drop_frame,
                           long long rec_seconds, int wide) {
  const Row* r = find(system);
  if (!r) return fail(c, MI_DV_ERR_ARG, "mi_dv_meta_write_batch: unknown system %d", system);
  return meta_write_batch(c, *r, "mi_dv_meta_write_batch", d_frames, n, first_frame, drop_frame, rec_seconds, wide);
}

int mi_dv_timecode_of(int system, long long frame, int drop_frame, int hmsf[4]) {
  const Row* r = find(system);
  if (!r || !hmsf || frame < 0)
    return fail(nullptr, MI_DV_ERR_ARG, "mi_dv_timecode_of: system %d, frame %lld out of range", system, frame);
  const int rc = meta_check_drop(nullptr, *r, "mi_dv_timecode_of", drop_frame);
  if (rc != MI_DV_OK) return rc;
  uint32_t v[4];
  meta_timecode(r->line ? 25u : 30u, (uint32_t)drop_frame, (unsigned long long)frame, v);
  for (int i = 0; i < 4; i++) hmsf[i] = (int)v[i];
  return MI_DV_OK;
}

int mi_dv_meta_times(mi_dv_ctx* c, float* total_ms, int* launches) {  // k_dv_meta_extract, k_dv_meta_write
  return times(c, c ? &c->meta.time : nullptr, 1, total_ms, launches, MI_DV_ERR_ARG);
}

}  // extern "C"
