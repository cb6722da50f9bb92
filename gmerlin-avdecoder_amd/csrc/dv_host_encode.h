// dv_host_encode.h — the encoder's calls.  Included by mi_dv.hip after dv_host_systems.h; not a
// kernel header.
#pragma once
#include "dv_host_systems.h"

namespace {
int check_flags(mi_dv_ctx* c, const char* who, int flags) {
  if (flags < 0 || flags > 3) return fail(c, MI_DV_ERR_ARG, "%s: flags %d; bit 0: 2-4-8 blocks, bit 1: classes", who, flags);
  return MI_DV_OK;
}

// n resident pictures of system r into n resident frames, timed: every argument is checked before anything is launched
int encode_batch(mi_dv_ctx* c, const Row& r, const char* who, const void* d_pics, int n, void* d_frames, int flags) {
  const BatchCheck k{c, who};
  int rc = k.count(c && d_pics && d_frames, n, "pictures");
  if (rc == MI_DV_OK) rc = check_flags(c, who, flags);
  if (rc == MI_DV_OK) rc = k.aligned(d_frames, d_pics, nullptr, "4-byte and d_pics 8-byte");
  if (rc == MI_DV_OK) rc = k.apart(d_frames, (size_t)n * r.frame_bytes, "d_frames", d_pics, (size_t)n * r.pic_bytes, "d_pics");
  if (rc != MI_DV_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemsetAsync(c->d_enc_stats, 0, kEncStats * sizeof(unsigned long long), c->stream));
  rc = c->encode_time.begin(c, c->stream);
  if (rc != MI_DV_OK) return rc;
  r.encode(c->stream, (const uint8_t*)d_pics, (unsigned)n, (uint8_t*)d_frames, c->d_enc, (uint32_t)flags, c->d_enc_stats);
  HIPCHK(c, hipGetLastError());
  return c->encode_time.end(c, c->stream);
}

// one picture from the caller's planes through the pinned picture and the kernel into `cap` bytes of host memory
int encode_one(mi_dv_ctx* c, const Row& r, const char* who, const uint8_t* const planes[3], const int strides[3], uint8_t* frame,
               size_t cap, int flags) {
  if (!c || !frame || !has_planes(planes, strides)) return fail(c, MI_DV_ERR_ARG, "%s: NULL argument", who);
  if (cap < (size_t)r.frame_bytes)
    return fail(c, MI_DV_ERR_ARG, "%s: room for %zu bytes: %s frames have %d", who, cap, r.frames, r.frame_bytes);
  int rc = check_flags(c, who, flags);
  if (rc == MI_DV_OK) rc = check_strides(c, r, strides);
  if (rc != MI_DV_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  rc = one_frame_buffers(c, r);
  if (rc != MI_DV_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));  // (the pinned picture is free)
  copy_planes(r, c->h_pic, (uint8_t* const*)planes, strides, false);  // (read only)
  HIPCHK(c, hipMemcpyAsync(c->d_pic, c->h_pic, (size_t)r.pic_bytes, hipMemcpyHostToDevice, c->stream));
  rc = encode_batch(c, r, who, c->d_pic, 1, c->d_frame, flags);
  if (rc != MI_DV_OK) return rc;
  HIPCHK(c, hipMemcpyAsync(frame, c->d_frame, (size_t)r.frame_bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return MI_DV_OK;
}
}  // namespace
