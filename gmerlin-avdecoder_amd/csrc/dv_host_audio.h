// dv_host_audio.h — the sound's calls.  Included by mi_dv.hip after dv_host_systems.h; not a
// kernel header.
#pragma once
#include "dv_host_systems.h"

namespace {
static_assert(MI_DV_AUDIO_PAIRS == kAudioPairs && MI_DV_AUDIO_PAIR_BYTES == kAudioPairBytes, "header and kernels agree (sound)");

// 0: 48 kHz, 1: 44.1 kHz, 2: 32 kHz, as the AAUX source pack numbers them; -1: no rate of DV's
int audio_freq(int samplerate) { return samplerate == 48000 ? 0 : samplerate == 44100 ? 1 : samplerate == 32000 ? 2 : -1; }

// the samples of frame k of an unlocked stream: what k + 1 frames hold, less what k frames hold, rounded down both times
int audio_cadence(const Row& r, int samplerate, long long k) {
  const long long per_num = (long long)samplerate * r.rate_den;  // samples a frame: per_num / rate_num
  return (int)((k + 1) * per_num / r.rate_num - k * per_num / r.rate_num);
}

// the sound of n resident frames of system r into d_pcm and d_info, timed: every argument is checked before anything is
// launched
int audio_batch(mi_dv_ctx* c, const Row& r, const char* who, const void* d_frames, int n, void* d_pcm, int pairs, void* d_info) {
  const BatchCheck k{c, who};
  int rc = k.count(c && d_frames && d_pcm && d_info, n, "frames");
  if (rc == MI_DV_OK && (pairs < 1 || pairs > MI_DV_AUDIO_PAIRS))
    rc = fail(c, MI_DV_ERR_ARG, "%s: %d pairs; 1 to %d", who, pairs, (int)MI_DV_AUDIO_PAIRS);
  if (rc == MI_DV_OK) rc = k.on(d_frames, 4, "d_frames");
  if (rc == MI_DV_OK) rc = k.on(d_pcm, 16, "d_pcm");
  if (rc == MI_DV_OK) rc = k.on(d_info, 4, "d_info");
  if (rc != MI_DV_OK) return rc;
  const size_t frame_bytes = (size_t)n * r.frame_bytes, pcm_bytes = (size_t)n * pairs * MI_DV_AUDIO_PAIR_BYTES, info_bytes = (size_t)n * 16;
  rc = k.apart(d_pcm, pcm_bytes, "d_pcm", d_frames, frame_bytes, "d_frames");
  if (rc == MI_DV_OK) rc = k.apart(d_info, info_bytes, "d_info", d_frames, frame_bytes, "d_frames");
  if (rc == MI_DV_OK) rc = k.apart(d_info, info_bytes, "d_info", d_pcm, pcm_bytes, "d_pcm");
  if (rc != MI_DV_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  mi_dv_ctx::Audio& a = c->audio;
  rc = a.time.begin(c, c->stream);
  if (rc != MI_DV_OK) return rc;
  r.audio_extract(c->stream, (const uint8_t*)d_frames, (unsigned)n, (uint8_t*)d_pcm, (uint32_t)pairs, (int32_t*)d_info, a.d_tab);
  HIPCHK(c, hipGetLastError());
  return a.time.end(c, c->stream);
}

// 16-bit sound from d_pcm into the audio blocks of n resident frames of system r, timed: every argument is checked before
// anything is launched.  The sample counts go through a pinned buffer (it only grows), guarded by an event
int audio_write_batch(mi_dv_ctx* c, const Row& r, const char* who, void* d_frames, int n, const void* d_pcm, int pairs,
                      int samplerate, const int* samples) {
  const BatchCheck k{c, who};
  int rc = k.count(c && d_frames && d_pcm && samples, n, "frames");
  if (rc != MI_DV_OK) return rc;
  if (pairs < r.chans || pairs > MI_DV_AUDIO_PAIRS)
    return fail(c, MI_DV_ERR_ARG, "%s: %d pairs; %s frames take %d, at most %d", who, pairs, r.frames, r.chans, (int)MI_DV_AUDIO_PAIRS);
  const int freq = audio_freq(samplerate);
  if (freq < 0) return fail(c, MI_DV_ERR_ARG, "%s: %d Hz; 48000, 44100 or 32000", who, samplerate);
  AudioTables t;
  build_audio_tables(&t);
  const int lo = t.min_samples[r.line][freq], hi = lo + 63;
  for (int i = 0; i < n; i++)
    if (samples[i] < lo || samples[i] > hi)
      return fail(c, MI_DV_ERR_ARG, "%s: frame %d has %d samples; %s frames at %d Hz hold %d to %d", who, i, samples[i], r.frames,
                  samplerate, lo, hi);
  rc = k.on(d_frames, 4, "d_frames");
  if (rc == MI_DV_OK) rc = k.on(d_pcm, 16, "d_pcm");
  if (rc == MI_DV_OK)
    rc = k.apart(d_pcm, (size_t)n * pairs * MI_DV_AUDIO_PAIR_BYTES, "d_pcm", d_frames, (size_t)n * r.frame_bytes, "d_frames");
  if (rc != MI_DV_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  mi_dv_ctx::Audio& a = c->audio;
  if (!a.samples_done) HIPCHK(c, hipEventCreateWithFlags(&a.samples_done.p, hipEventDisableTiming));
  if ((uint64_t)n > a.d_samples.cap) {
    rc = release_together(c, c->stream, a.h_samples, a.d_samples);
    if (rc == MI_DV_OK) rc = a.h_samples.grow(c, (uint64_t)n, nullptr);
    if (rc == MI_DV_OK) rc = a.d_samples.grow(c, (uint64_t)n, nullptr);
    if (rc != MI_DV_OK) return rc;
  }
  HIPCHK(c, hipEventSynchronize(a.samples_done));  // (the last upload has left the pinned buffer; at once if there was none)
  for (int i = 0; i < n; i++) a.h_samples[i] = samples[i];
  HIPCHK(c, hipMemcpyAsync(a.d_samples, a.h_samples, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(a.samples_done, c->stream));
  rc = a.time.begin(c, c->stream);
  if (rc != MI_DV_OK) return rc;
  r.audio_write(c->stream, (uint8_t*)d_frames, (unsigned)n, (const uint8_t*)d_pcm, (uint32_t)pairs, (uint32_t)freq, a.d_samples, a.d_tab);
  HIPCHK(c, hipGetLastError());
  return a.time.end(c, c->stream);
}
}  // namespace
