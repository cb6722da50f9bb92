// dv_host_meta.h — the calls of the timecode, the recording date and time and the aspect flag.
// Included by mi_dv.hip after dv_host_systems.h; not a kernel header.
#pragma once
#include "dv_host_systems.h"

namespace {
static_assert(MI_DV_META_INTS == kMetaInts, "header and kernels agree (timecode, date, aspect)");
constexpr long long kMetaFrameLimit = 1ll << 40;  // first_frame + n stays at or below it

// the rows of n resident frames of system r into d_meta, timed: every argument is checked before anything is launched
int meta_batch(mi_dv_ctx* c, const Row& r, const char* who, const void* d_frames, int n, void* d_meta) {
  const BatchCheck k{c, who};
  int rc = k.count(c && d_frames && d_meta, n, "frames");
  if (rc == MI_DV_OK) rc = k.on(d_frames, 4, "d_frames");
  if (rc == MI_DV_OK) rc = k.on(d_meta, 64, "d_meta");
  if (rc == MI_DV_OK)
    rc = k.apart(d_meta, (size_t)n * kMetaInts * sizeof(int32_t), "d_meta", d_frames, (size_t)n * r.frame_bytes, "d_frames");
  if (rc != MI_DV_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  rc = c->meta.time.begin(c, c->stream);
  if (rc != MI_DV_OK) return rc;
  r.meta_extract(c->stream, (const uint8_t*)d_frames, (unsigned)n, (int32_t*)d_meta);
  HIPCHK(c, hipGetLastError());
  return c->meta.time.end(c, c->stream);
}

// what mi_dv_meta_write_batch and mi_dv_timecode_of refuse of a timecode's arguments
int meta_check_drop(mi_dv_ctx* c, const Row& r, const char* who, int drop_frame) {
  if (drop_frame != 0 && drop_frame != 1) return fail(c, MI_DV_ERR_ARG, "%s: drop_frame %d; 0 or 1", who, drop_frame);
  if (drop_frame && r.line) return fail(c, MI_DV_ERR_ARG, "%s: %s frames have no drop-frame timecode", who, r.frames);
  return MI_DV_OK;
}

// the subcode and VAUX blocks of n resident frames of system r, timed: every argument is checked before anything is
// launched
int meta_write_batch(mi_dv_ctx* c, const Row& r, const char* who, void* d_frames, int n, long long first_frame, int drop_frame,
                     long long rec_seconds, int wide) {
  const BatchCheck k{c, who};
  int rc = k.count(c && d_frames, n, "frames");
  if (rc == MI_DV_OK) rc = k.on(d_frames, 4, "d_frames");
  if (rc == MI_DV_OK) rc = meta_check_drop(c, r, who, drop_frame);
  if (rc != MI_DV_OK) return rc;
  if (first_frame < 0 || first_frame > kMetaFrameLimit - n)
    return fail(c, MI_DV_ERR_ARG, "%s: frames %lld to %lld + %d; 0 to 2^40", who, first_frame, first_frame, n);
  if (rec_seconds >= kMetaLastSecond)
    return fail(c, MI_DV_ERR_ARG, "%s: recording time %lld s; below %lld (2070), or negative for none", who, rec_seconds,
                (long long)kMetaLastSecond);
  if (wide != 0 && wide != 1) return fail(c, MI_DV_ERR_ARG, "%s: wide %d; 0 or 1", who, wide);
  HIPCHK(c, hipSetDevice(c->device));
  rc = c->meta.time.begin(c, c->stream);
  if (rc != MI_DV_OK) return rc;
  r.meta_write(c->stream, (uint8_t*)d_frames, (unsigned)n, (unsigned long long)first_frame, (uint32_t)drop_frame,
               rec_seconds < 0 ? -1ll : rec_seconds, (uint32_t)wide);
  HIPCHK(c, hipGetLastError());
  return c->meta.time.end(c, c->stream);
}
}  // namespace
