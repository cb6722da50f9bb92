// mi_pcm.hip — C ABI (include/mi_pcm.h) of the MI355X decoder of the PCM family of lib/audio_pcm.c.  No CPU path: without
// a gfx950 device every call but the host-only ones fails with a message.  The codec table, the transforms, the G.711
// tables, the float classifiers and init_pcm's arms: pcm_format.h; the kernels: pcm_kernels.h.  Owned memory, errors, the
// event timer and the bodies of the calls every device library has: host_base.h.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/mi_pcm.h"
#include "host_base.h"
#include "pcm_kernels.h"

using namespace mipcm;

static_assert(MI_PCM_OK == kOk && MI_PCM_ERR_HIP == kErrHip, "header and host base agree");
static_assert(MI_PCM_COPY8 == kCopy8 && MI_PCM_COPY16 == kCopy16 && MI_PCM_SWAP16 == kSwap16 && MI_PCM_S24LE == kS24le &&
                  MI_PCM_S24BE == kS24be && MI_PCM_LPCM24 == kLpcm24 && MI_PCM_LPCM24_MONO == kLpcm24Mono &&
                  MI_PCM_LPCM20 == kLpcm20 && MI_PCM_LPCM20_MONO == kLpcm20Mono && MI_PCM_COPY32 == kCopy32 &&
                  MI_PCM_SWAP32 == kSwap32 && MI_PCM_F32LE == kF32le && MI_PCM_F32BE == kF32be && MI_PCM_F64LE == kF64le &&
                  MI_PCM_F64BE == kF64be && MI_PCM_ULAW == kUlaw && MI_PCM_ALAW == kAlaw && MI_PCM_CODECS == kCodecs,
              "header and format table agree on the codecs");
static_assert(MI_PCM_U8 == kU8 && MI_PCM_S8 == kS8 && MI_PCM_U16 == kU16 && MI_PCM_S16 == kS16 && MI_PCM_S32 == kS32 &&
                  MI_PCM_FLOAT == kFloat && MI_PCM_DOUBLE == kDouble && MI_PCM_ENDIANESS_LITTLE == kEndianLittle,
              "header and format table agree on the labels");
static_assert(MI_PCM_TILE_BYTES == kTileBytes && MI_PCM_FRAME_SAMPLES == kFrameSamples && MI_PCM_MAX_CHANNELS == kMaxChannels,
              "header and kernels agree");

namespace {
// What one call brings from the host: offsets, sample_offsets, valid_in, out_bytes and tile_first, in pinned memory and on
// the device.  A call takes a slot whose last call is over (`done`), so it never touches what a queued launch still reads.
struct CallSlot {
  PinnedBuf<uint8_t> h;
  DevBuf<uint8_t> d;
  Event done;
  bool used = false;
};
constexpr size_t kMaxSlots = 64;  // with this many calls in flight a call waits for the oldest
constexpr uint64_t kMaxTiles = 0x7fffffffu;
uint64_t up16(uint64_t x) { return (x + 15u) & ~(uint64_t)15u; }
}  // namespace

// Device, stream and error text are HostCtx's (host_base.h), destroyed after everything here; the timer goes before the
// pool it hands its pairs to.
struct __attribute__((visibility("hidden"))) mi_pcm_ctx : HostCtx {
  EventPool ev_free;
  Timer t_launch{ev_free};     // mi_pcm_times: a pair a launch
  std::deque<CallSlot> slots;  // oldest call first
  // mi_pcm_decode_packet's staging: the packet on the device; samples and count on the device and in pinned memory
  DevBuf<uint8_t> d_in, d_out;
  PinnedBuf<uint8_t> h_out;
};

namespace {
// a slot no launch reads any more, at the back of the queue: the oldest if its call is over (or if kMaxSlots are in
// flight: after waiting for it), else a new one
int free_slot(mi_pcm_ctx* c, CallSlot** out) {
  if (!c->slots.empty()) {
    CallSlot& old = c->slots.front();
    bool over = !old.used;
    if (!over) {
      const hipError_t q = hipEventQuery(old.done);
      if (q == hipSuccess) over = true;
      else if (q != hipErrorNotReady) return fail(c, MI_PCM_ERR_HIP, "hipEventQuery failed: %s", hipGetErrorString(q));
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
      return MI_PCM_OK;
    }
  }
  CallSlot fresh;
  HIPCHK(c, hipEventCreateWithFlags(&fresh.done.p, hipEventDisableTiming));
  c->slots.push_back(std::move(fresh));
  *out = &c->slots.back();
  return MI_PCM_OK;
}

struct Job {
  int codec;
  uint32_t ch;
  const uint8_t* packets;
  const uint64_t* offsets;
  const uint32_t* lens;
  int n;
  uint8_t* samples;
  const uint64_t* sample_offsets;
  uint32_t* outside;
  uint64_t tiles;  // of the call
};

template <class Launch>
int timed(mi_pcm_ctx* c, const char* what, Launch launch) {
  int rc = c->t_launch.begin(c, c->stream);
  if (rc != MI_PCM_OK) return rc;
  launch();
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(c, MI_PCM_ERR_HIP, "the launch of %s failed: %s", what, hipGetErrorString(e));
  return c->t_launch.end(c, c->stream);
}

// the call's arrays into the slot and on their way to the device in one copy, then the launches; the checks are the caller's
int stage_and_launch(mi_pcm_ctx* c, const Job& j, CallSlot& s) {
  const size_t n = (size_t)j.n, o_samples = 8u * n, o_valid = 16u * n, o_bytes = 20u * n, o_first = 24u * n, bytes = 28u * n;
  if (j.outside) {
    const int rc = timed(c, "k_pcm_zero", [&] {
      hipLaunchKernelGGL(k_pcm_zero, dim3(((uint32_t)j.n + 255u) / 256u), dim3(256), 0, c->stream, j.outside, (uint32_t)j.n);
    });
    if (rc != MI_PCM_OK) return rc;
  }
  if (j.tiles == 0) return MI_PCM_OK;
  int rc = s.h.grow(c, bytes, nullptr);  // (no launch uses the slot: nothing is waited for)
  if (rc == MI_PCM_OK) rc = s.d.grow(c, bytes, nullptr);
  if (rc != MI_PCM_OK) return rc;
  uint8_t* h = s.h;
  memcpy(h, j.offsets, 8u * n);
  memcpy(h + o_samples, j.sample_offsets, 8u * n);
  uint32_t *valid = (uint32_t*)(h + o_valid), *out_bytes = (uint32_t*)(h + o_bytes), *first = (uint32_t*)(h + o_first);
  uint64_t tiles = 0;
  for (size_t i = 0; i < n; i++) {
    const Layout l = layout_of(j.codec, j.ch, j.lens[i]);
    valid[i] = (uint32_t)l.valid_in, out_bytes[i] = (uint32_t)l.out_bytes, first[i] = (uint32_t)tiles;
    tiles += (l.out_bytes + kTileBytes - 1u) / kTileBytes;
  }
  HIPCHK(c, hipMemcpyAsync(s.d, h, bytes, hipMemcpyHostToDevice, c->stream));
  Call k;
  k.packets = j.packets, k.samples = j.samples, k.offsets = (const uint64_t*)s.d.p;
  k.sample_offsets = (const uint64_t*)(s.d.p + o_samples), k.valid_in = (const uint32_t*)(s.d.p + o_valid);
  k.out_bytes = (const uint32_t*)(s.d.p + o_bytes), k.tile_first = (const uint32_t*)(s.d.p + o_first);
  k.outside = j.outside, k.n = (uint32_t)j.n;
  return timed(c, "k_pcm_decode", [&] {
    dispatch(j.codec, [&](auto tag) {
      hipLaunchKernelGGL(k_pcm_decode<decltype(tag)::value>, dim3((uint32_t)j.tiles), dim3(kThreads), 0, c->stream, k);
    });
  });
}

int run(mi_pcm_ctx* c, const Job& j) {
  CallSlot* slot = nullptr;
  int rc = free_slot(c, &slot);
  if (rc != MI_PCM_OK) return rc;
  rc = stage_and_launch(c, j, *slot);
  // whatever became of the launch, the copy may be queued: the slot is free when the stream has passed this point
  slot->used = true;
  const hipError_t e = hipEventRecord(slot->done, c->stream);
  if (e != hipSuccess && rc == MI_PCM_OK) return fail(c, MI_PCM_ERR_HIP, "hipEventRecord failed: %s", hipGetErrorString(e));
  return rc;
}

bool takes(int codec, int channels) {
  return codec >= 0 && codec < kCodecs && channels >= 1 && channels <= kMaxChannels && !(kGroups[codec].mono && channels != 1);
}
}  // namespace

extern "C" {

int mi_pcm_device_count(void) { return device_count(); }

const char* mi_pcm_last_error(const mi_pcm_ctx* c) { return last_error(c); }

mi_pcm_ctx* mi_pcm_create(int device) {
  if ((device = usable_device(device, "PCM decoder", MI_PCM_ERR_ARG)) < 0) return nullptr;
  mi_pcm_ctx* c = new mi_pcm_ctx();
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream.p, hipStreamNonBlocking) != hipSuccess) {
    fail(nullptr, MI_PCM_ERR_HIP, "cannot set up device %d: %s", device, hipGetErrorString(hipGetLastError()));
    mi_pcm_destroy(c);
    return nullptr;
  }
  return c;
}

void mi_pcm_destroy(mi_pcm_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  delete c;
}

void* mi_pcm_dev_alloc(mi_pcm_ctx* c, size_t bytes) {
  if (!c) return nullptr;
  void* d = nullptr;
  if (hipSetDevice(c->device) != hipSuccess || hipMalloc(&d, bytes ? bytes : 1) != hipSuccess) {
    fail(c, MI_PCM_ERR_NOMEM, "hipMalloc(%zu) failed", bytes);
    return nullptr;
  }
  return d;
}
void mi_pcm_dev_free(mi_pcm_ctx* c, void* d) { dev_free(c, d); }
int mi_pcm_h2d(mi_pcm_ctx* c, void* d, const void* h, size_t n) {
  if (!c || (!d && n) || (!h && n)) return fail(c, MI_PCM_ERR_ARG, "mi_pcm_h2d: NULL argument");
  return copy_sync(c, d, h, n, hipMemcpyHostToDevice);
}
int mi_pcm_d2h(mi_pcm_ctx* c, void* h, const void* d, size_t n) {
  if (!c || (!d && n) || (!h && n)) return fail(c, MI_PCM_ERR_ARG, "mi_pcm_d2h: NULL argument");
  return copy_sync(c, h, d, n, hipMemcpyDeviceToHost);
}
int mi_pcm_sync(mi_pcm_ctx* c) { return c ? stream_sync(c) : MI_PCM_ERR_ARG; }

int mi_pcm_codec_of(uint32_t fourcc, int bits, int channels, int endianess, const uint8_t* header, int header_len, mi_pcm_format* out) {
  if (!out || channels < 1 || channels > kMaxChannels) return -1;
  Format f;
  if (!codec_of(fourcc, bits, channels, endianess, header, header_len, &f)) return -1;
  out->codec = f.codec, out->label = f.label, out->block_align = f.block_align, out->sample_bytes = f.sample_bytes;
  return 0;
}

int64_t mi_pcm_payload_of(int64_t len, int64_t duration, int block_align) { return payload_of(len, duration, block_align); }

int mi_pcm_layout_of(int codec, int channels, uint64_t len, mi_pcm_layout* out) {
  if (!out || !takes(codec, channels)) return -1;
  const Layout l = layout_of(codec, (uint32_t)channels, len);
  out->frames = l.frames, out->written = l.written, out->consumed = l.consumed, out->out_bytes = l.out_bytes;
  return 0;
}

int mi_pcm_decode_batch(mi_pcm_ctx* c, int codec, int channels, const void* d_packets, const uint64_t* offsets, const uint32_t* lens,
                        int n, void* d_samples, const uint64_t* sample_offsets, uint32_t* d_outside) {
  const char* who = "mi_pcm_decode_batch";
  if (!c || !d_packets || !offsets || !lens || !d_samples || !sample_offsets) return fail(c, MI_PCM_ERR_ARG, "%s: NULL argument", who);
  if (n < 1 || n > MI_PCM_MAX_PACKETS) return fail(c, MI_PCM_ERR_ARG, "%s: %d packets; 1 to %d per call (split the batch)", who, n, (int)MI_PCM_MAX_PACKETS);
  if (codec < 0 || codec >= kCodecs) return fail(c, MI_PCM_ERR_ARG, "%s: codec %d; 0 to %d", who, codec, kCodecs - 1);
  if (!takes(codec, channels)) return fail(c, MI_PCM_ERR_ARG, "%s: %d channels for %s; 1 to %d, and 1 for the mono codecs", who, channels, kGroups[codec].name, kMaxChannels);
  if ((uintptr_t)d_samples & 15u) return fail(c, MI_PCM_ERR_ARG, "%s: d_samples must be 16-byte aligned", who);
  if ((uintptr_t)d_outside & 3u) return fail(c, MI_PCM_ERR_ARG, "%s: d_outside must be 4-byte aligned", who);
  uint64_t tiles = 0;
  for (int i = 0; i < n; i++) {
    if (lens[i] >= 0x80000000u) return fail(c, MI_PCM_ERR_ARG, "%s: packet %d has %u bytes; below 2^31", who, i, lens[i]);
    if (sample_offsets[i] & 15u) return fail(c, MI_PCM_ERR_ARG, "%s: sample_offsets[%d] must be a multiple of 16", who, i);
    tiles += (layout_of(codec, (uint32_t)channels, lens[i]).out_bytes + kTileBytes - 1u) / kTileBytes;
  }
  if (tiles > kMaxTiles) return fail(c, MI_PCM_ERR_ARG, "%s: %llu tiles of %u output bytes; at most %llu a call (split the batch)", who, (unsigned long long)tiles, kTileBytes, (unsigned long long)kMaxTiles);
  HIPCHK(c, hipSetDevice(c->device));
  const Job j = {codec, (uint32_t)channels, (const uint8_t*)d_packets, offsets, lens, n, (uint8_t*)d_samples, sample_offsets, d_outside, tiles};
  return run(c, j);
}

int mi_pcm_decode_packet(mi_pcm_ctx* c, int codec, int channels, const uint8_t* bytes, size_t len, void* samples, uint32_t* outside) {
  const char* who = "mi_pcm_decode_packet";
  if (!c || (!bytes && len)) return fail(c, MI_PCM_ERR_ARG, "%s: NULL argument", who);
  if (!takes(codec, channels)) return fail(c, MI_PCM_ERR_ARG, "%s: codec %d with %d channels", who, codec, channels);
  if (len >= 0x80000000u) return fail(c, MI_PCM_ERR_ARG, "%s: %zu bytes; below 2^31", who, len);
  const Layout l = layout_of(codec, (uint32_t)channels, len);
  if (!samples && l.out_bytes) return fail(c, MI_PCM_ERR_ARG, "%s: NULL argument", who);
  HIPCHK(c, hipSetDevice(c->device));
  // (the stream is idle between these calls: nothing is waited for).  The count lies behind the samples.
  const size_t o_count = (size_t)up16(l.out_bytes), staged = o_count + 16u;
  int rc = c->d_in.grow(c, up16(len ? len : 1), nullptr);
  if (rc == MI_PCM_OK) rc = c->d_out.grow(c, staged, nullptr);
  if (rc == MI_PCM_OK) rc = c->h_out.grow(c, staged, nullptr);
  if (rc != MI_PCM_OK) return rc;
  if (len) HIPCHK(c, hipMemcpyAsync(c->d_in, bytes, len, hipMemcpyHostToDevice, c->stream));
  const uint64_t zero = 0;
  const uint32_t used = (uint32_t)len;
  const Job j = {codec, (uint32_t)channels, c->d_in, &zero, &used, 1, c->d_out, &zero, (uint32_t*)(c->d_out.p + o_count),
                 (l.out_bytes + kTileBytes - 1u) / kTileBytes};
  rc = run(c, j);
  if (rc != MI_PCM_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(c->h_out, c->d_out, staged, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (l.out_bytes) memcpy(samples, c->h_out.p, l.out_bytes);
  if (outside) memcpy(outside, c->h_out.p + o_count, 4);
  return MI_PCM_OK;
}

int mi_pcm_times(mi_pcm_ctx* c, float* ms, int* launches) { return times(c, c ? &c->t_launch : nullptr, 1, ms, launches, MI_PCM_ERR_ARG); }

}  // extern "C"
