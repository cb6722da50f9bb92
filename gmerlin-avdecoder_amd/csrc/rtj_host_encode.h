// rtj_host_encode.h — the entry points beside the decoder: synthetic pictures, the encoder (all formats), the colour
// stage, the copy ceiling and the quantiser tables.  Included by mi_rtjpeg.hip behind the instance's state.
#pragma once

namespace {
// the format's kernel of one pass: m pictures (kInter: one) from `frames` into block slots and lengths
template <bool kInter>
void launch_encode_fmt(int fmt, hipStream_t st, const uint8_t* frames, int w, int h, int m, const QTab* qt, uint8_t* slots,
                       uint8_t* lens, int16_t* old, int lmask, int cmask) {
  const Format& F = kFormats[fmt];
  const dim3 grid(F.parts * F.groups((uint32_t)F.units(w, h)), (unsigned)m);
  if (fmt == MI_RTJ_FMT_YUV420)
    hipLaunchKernelGGL((k_encode_fmt<kFmtYUV420, kInter>), grid, dim3(64), 0, st, frames, w, h, qt, slots, lens, old, lmask, cmask);
  else if (fmt == MI_RTJ_FMT_YUV422)
    hipLaunchKernelGGL((k_encode_fmt<kFmtYUV422, kInter>), grid, dim3(64), 0, st, frames, w, h, qt, slots, lens, old, lmask, cmask);
  else
    hipLaunchKernelGGL((k_encode_fmt<kFmtGrey, kInter>), grid, dim3(64), 0, st, frames, w, h, qt, slots, lens, old, lmask, cmask);
}

// work queued on the stream is waited for when the scope ends (declared behind the buffers that work uses)
struct SyncAtExit {
  hipStream_t s;
  ~SyncAtExit() { (void)hipStreamSynchronize(s); }
};

// shared body of the intra batch encoder and the in-order inter (skip-block) stream encoder, all formats
int encode_impl(mi_rtj_ctx* c, int fmt, int w, int h, int Q, int key_rate, int lmask, int cmask, int n, const void* d_frames,
                void* d_stream, int align, uint64_t* pkt_offset, uint32_t* pkt_len) {
  if (!format_known(fmt))
    return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_encode: unknown format %d (0 = 4:2:0, 1 = 4:2:2, 2 = greyscale)", fmt);
  const Format& F = kFormats[fmt];
  const bool args_ok = c && d_frames && d_stream && pkt_offset && pkt_len && n > 0 && align >= 1 && !(align & (align - 1));
  if (fmt == MI_RTJ_FMT_YUV420) {  // the calls without a format argument have one message for everything
    if (!args_ok || !F.geometry_ok(w, h)) return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_encode: bad argument");
  } else {
    if (!args_ok)
      return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_encode: bad argument (NULL buffer, no pictures, or align not a power of two)");
    if (!F.geometry_ok(w, h)) return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_encode: %dx%d: %s", w, h, F.encode_rule);
  }
  if (Q < 1) Q = 1;
  if (Q > 255) Q = 255;
  // RTjpeg_set_intra's clamps (lib/RTjpeg.c:2459-2468)
  key_rate = key_rate < 0 ? 0 : (key_rate > 255 ? 255 : key_rate);
  lmask = lmask < 0 ? 0 : (lmask > 16 ? 16 : lmask);
  cmask = cmask < 0 ? 0 : (cmask > 16 ? 16 : cmask);
  const bool inter = key_rate > 0;
  HIPCHK(c, hipSetDevice(c->device));
  const uint32_t nblk = (uint32_t)F.blocks(w, h);
  const size_t fsz = F.picture_bytes(w, h);
  // frames per pass: inter frames depend on each other, intra ones do not (256: 0.8 GB of block slots at 1080p)
  const int chunk = inter ? 1 : (int)std::max<size_t>(1, std::min<size_t>(256, ((size_t)1 << 30) / ((size_t)nblk * 64)));
  hipStream_t const s = c->stream;
  DevBuf<uint8_t> slots, lens;
  DevBuf<uint32_t> offs, fbytes, d_alllen;
  DevBuf<uint64_t> d_pktoff, d_alloff;
  DevBuf<int16_t> old;
  const SyncAtExit wait{s};  // (before the buffers above go)
  int rc;
  if ((rc = slots.grow(c, (size_t)chunk * nblk * 64, s)) != MI_RTJ_OK) return rc;
  if ((rc = lens.grow(c, (size_t)chunk * nblk, s)) != MI_RTJ_OK) return rc;
  if ((rc = offs.grow(c, (size_t)chunk * nblk, s)) != MI_RTJ_OK) return rc;
  if ((rc = fbytes.grow(c, (size_t)chunk, s)) != MI_RTJ_OK) return rc;
  if ((rc = d_pktoff.grow(c, (size_t)chunk, s)) != MI_RTJ_OK) return rc;
  if (inter && (rc = old.grow(c, (size_t)nblk * 64, s)) != MI_RTJ_OK) return rc;
  // packet offsets and lengths of ALL frames stay on the device until the end: no host round trip between passes
  if ((rc = d_alloff.grow(c, (size_t)n + 1, s)) != MI_RTJ_OK) return rc;
  if ((rc = d_alllen.grow(c, (size_t)n, s)) != MI_RTJ_OK) return rc;
  uint64_t* const d_cursor = d_alloff + n;
  HIPCHK(c, hipMemsetAsync(d_cursor, 0, 8, s));
  int key_count = 0;
  for (int f0 = 0; f0 < n; f0 += chunk) {
    const int m = n - f0 < chunk ? n - f0 : chunk;
    // RTjpeg_compress: the previous-block store is cleared whenever key_count is 0 (lib/RTjpeg.c:3504-3505)
    if (inter && key_count == 0) HIPCHK(c, hipMemsetAsync(old, 0, (size_t)nblk * 64 * sizeof(int16_t), s));
    const uint8_t* fr = (const uint8_t*)d_frames + (size_t)f0 * fsz;
    if (inter) launch_encode_fmt<true>(fmt, s, fr, w, h, m, c->d_lut + Q, slots, lens, old, lmask, cmask);
    else launch_encode_fmt<false>(fmt, s, fr, w, h, m, c->d_lut + Q, slots, lens, nullptr, 0, 0);
    hipLaunchKernelGGL(k_encode_scan, dim3(m), dim3(256), 0, s, lens, nblk, offs, fbytes);
    hipLaunchKernelGGL(k_encode_place, dim3(1), dim3(256), 0, s, fbytes, m, (uint32_t)align, d_cursor, d_alloff + f0,
                       d_alllen + f0, d_pktoff);
    hipLaunchKernelGGL(k_encode_pack, dim3((nblk + 255) / 256, m), dim3(256), 0, s, slots, lens, offs,
                       d_pktoff, fbytes, nblk, w, h, Q, inter ? key_count : 0, (uint8_t*)d_stream);
    HIPCHK(c, hipGetLastError());
    if (inter && ++key_count > key_rate) key_count = 0;  // lib/RTjpeg.c:3512-3514
  }
  // one copy of every packet's place and size at the end (the kernels of all passes are queued by now)
  HIPCHK(c, hipMemcpyAsync(pkt_offset, d_alloff, (size_t)n * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(pkt_len, d_alllen, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return MI_RTJ_OK;
}
}  // namespace

extern "C" {

int mi_rtj_synth_frames(mi_rtj_ctx* c, int w, int h, int first, int n, uint32_t seed, int amp, void* d_frames) {
  if (!c || !d_frames || w <= 0 || h <= 0 || (w & 15) || (h & 15) || n <= 0 || amp < 0)
    return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_synth_frames: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(k_synth, dim3(1024, n), dim3(256), 0, c->stream, (uint8_t*)d_frames, w, h, first, seed, amp);
  HIPCHK(c, hipGetLastError());
  return MI_RTJ_OK;
}

int mi_rtj_synth_frames_lcg(mi_rtj_ctx* c, int w, int h, int first, int n, uint32_t seed, int amp, void* d_frames) {
  if (!c || !d_frames || w <= 0 || h <= 0 || (w & 15) || (h & 15) || n <= 0 || amp < 0 || first < 0)
    return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_synth_frames_lcg: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(k_synth_lcg, dim3(4096), dim3(256), 0, c->stream, (uint8_t*)d_frames, w, h, first, n, seed, amp);
  HIPCHK(c, hipGetLastError());
  return MI_RTJ_OK;
}

// every block at its longest, 64 bytes; sizes that are no multiple of the macroblock round down, as they always have
size_t mi_rtj_encode_bound_fmt(int fmt, int w, int h, int n, int align) {
  if (!format_known(fmt) || w <= 0 || h <= 0 || n <= 0 || align < 1) return 0;
  const size_t per = MI_RTJ_HEADER_SIZE + (size_t)kFormats[fmt].blocks(w, h) * 64;
  return (size_t)n * ((per + align - 1) / align * align) + align;
}

size_t mi_rtj_encode_bound(int w, int h, int n, int align) { return mi_rtj_encode_bound_fmt(MI_RTJ_FMT_YUV420, w, h, n, align); }

int mi_rtj_encode_frames(mi_rtj_ctx* c, int w, int h, int Q, int n, const void* d_frames, void* d_stream, int align,
                         uint64_t* pkt_offset, uint32_t* pkt_len) {
  return encode_impl(c, MI_RTJ_FMT_YUV420, w, h, Q, 0, 0, 0, n, d_frames, d_stream, align, pkt_offset, pkt_len);
}

int mi_rtj_encode_frames_fmt(mi_rtj_ctx* c, int fmt, int w, int h, int Q, int n, const void* d_frames, void* d_stream,
                             int align, uint64_t* pkt_offset, uint32_t* pkt_len) {
  return encode_impl(c, fmt, w, h, Q, 0, 0, 0, n, d_frames, d_stream, align, pkt_offset, pkt_len);
}

int mi_rtj_encode_stream(mi_rtj_ctx* c, int w, int h, int Q, int key_rate, int lmask, int cmask, int n,
                         const void* d_frames, void* d_stream, int align, uint64_t* pkt_offset, uint32_t* pkt_len) {
  return encode_impl(c, MI_RTJ_FMT_YUV420, w, h, Q, key_rate, lmask, cmask, n, d_frames, d_stream, align, pkt_offset, pkt_len);
}

int mi_rtj_encode_stream_fmt(mi_rtj_ctx* c, int fmt, int w, int h, int Q, int key_rate, int lmask, int cmask, int n,
                             const void* d_frames, void* d_stream, int align, uint64_t* pkt_offset, uint32_t* pkt_len) {
  return encode_impl(c, fmt, w, h, Q, key_rate, lmask, cmask, n, d_frames, d_stream, align, pkt_offset, pkt_len);
}

int mi_rtj_yuv420_to_rgb(mi_rtj_ctx* c, int fmt, int w, int h, int n, const void* d_planes, size_t in_frame_stride,
                         void* d_rgb, size_t row_pitch, size_t out_frame_stride) {
  static const int bpp[5] = {4, 4, 3, 3, 2};
  if (!c || !d_planes || !d_rgb || fmt < 0 || fmt > 4 || w <= 0 || h <= 0 || (w & 15) || (h & 15) || n <= 0)
    return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_yuv420_to_rgb: bad argument");
  if (row_pitch < (size_t)w * bpp[fmt] || (row_pitch & 15) || ((uintptr_t)d_rgb & 15) || (out_frame_stride & 15) ||
      (in_frame_stride & 15) || ((uintptr_t)d_planes & 15))
    return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_yuv420_to_rgb: buffers, row pitch and frame strides must be 16-byte aligned");
  HIPCHK(c, hipSetDevice(c->device));
  const int tiles = (w / 8) * (h / 2);
  const dim3 grid((unsigned)((tiles + 255) / 256 < 2048 ? (tiles + 255) / 256 : 2048), (unsigned)n), block(256);
  const uint8_t* in = (const uint8_t*)d_planes;
  uint8_t* out = (uint8_t*)d_rgb;
  switch (fmt) {
    case kFmtRGB32: hipLaunchKernelGGL(k_yuv420_to_rgb<kFmtRGB32>, grid, block, 0, c->stream, in, in_frame_stride, out, row_pitch, out_frame_stride, w, h); break;
    case kFmtBGR32: hipLaunchKernelGGL(k_yuv420_to_rgb<kFmtBGR32>, grid, block, 0, c->stream, in, in_frame_stride, out, row_pitch, out_frame_stride, w, h); break;
    case kFmtRGB24: hipLaunchKernelGGL(k_yuv420_to_rgb<kFmtRGB24>, grid, block, 0, c->stream, in, in_frame_stride, out, row_pitch, out_frame_stride, w, h); break;
    case kFmtBGR24: hipLaunchKernelGGL(k_yuv420_to_rgb<kFmtBGR24>, grid, block, 0, c->stream, in, in_frame_stride, out, row_pitch, out_frame_stride, w, h); break;
    default:        hipLaunchKernelGGL(k_yuv420_to_rgb<kFmtRGB16>, grid, block, 0, c->stream, in, in_frame_stride, out, row_pitch, out_frame_stride, w, h); break;
  }
  HIPCHK(c, hipGetLastError());
  return MI_RTJ_OK;
}

int mi_rtj_yuv422_to_rgb24(mi_rtj_ctx* c, int w, int h, int n, const void* d_planes, size_t in_frame_stride, void* d_rgb,
                           size_t row_pitch, size_t out_frame_stride) {
  if (!c || !d_planes || !d_rgb || w <= 0 || h <= 0 || (w & 15) || (h & 7) || n <= 0 || n > kMaxPlanFrames)
    return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_yuv422_to_rgb24: bad argument");
  if (row_pitch < (size_t)w * 3 || (row_pitch & 15) || ((uintptr_t)d_rgb & 15) || (out_frame_stride & 15) ||
      (in_frame_stride & 15) || ((uintptr_t)d_planes & 15))
    return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_yuv422_to_rgb24: buffers, row pitch and frame strides must be 16-byte aligned");
  HIPCHK(c, hipSetDevice(c->device));
  const long long tiles = (long long)(w / 8) * h;
  const dim3 grid((unsigned)((tiles + 255) / 256 < 2048 ? (tiles + 255) / 256 : 2048), (unsigned)n), block(256);
  hipLaunchKernelGGL(k_yuv422_rgb24, grid, block, 0, c->stream, (const uint8_t*)d_planes, in_frame_stride, (uint8_t*)d_rgb,
                     row_pitch, out_frame_stride, w, h);
  HIPCHK(c, hipGetLastError());
  return MI_RTJ_OK;
}

int mi_rtj_copy_ceiling(mi_rtj_ctx* c, const void* d_src, void* d_dst, size_t bytes, int reps, double* gbs) {
  if (!c || !d_src || !d_dst || !gbs || bytes < 16 || (bytes & 15) || reps < 1 || ((uintptr_t)d_src & 15) || ((uintptr_t)d_dst & 15))
    return fail(c, MI_RTJ_ERR_ARG, "mi_rtj_copy_ceiling: bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  EventPair e;  // (every return destroys what it holds)
  HIPCHK(c, hipEventCreate(&e.start.p));
  HIPCHK(c, hipEventCreate(&e.stop.p));
  const size_t n16 = bytes / 16;
  const unsigned grid = (unsigned)std::min<size_t>((n16 + 255) / 256, 256u * 32u);
  hipLaunchKernelGGL(k_copy16, dim3(grid), dim3(256), 0, c->stream, (const uint4*)d_src, (uint4*)d_dst, n16);  // warm-up
  HIPCHK(c, hipEventRecord(e.start, c->stream));
  for (int r = 0; r < reps; r++)
    hipLaunchKernelGGL(k_copy16, dim3(grid), dim3(256), 0, c->stream, (const uint4*)d_src, (uint4*)d_dst, n16);
  HIPCHK(c, hipEventRecord(e.stop, c->stream));
  HIPCHK(c, hipEventSynchronize(e.stop));
  float ms = 0;
  HIPCHK(c, hipEventElapsedTime(&ms, e.start, e.stop));
  *gbs = 2.0 * (double)bytes * reps / ((double)ms * 1e6);
  return MI_RTJ_OK;
}

int mi_rtj_get_tables(int Q, int32_t tables[128], int* lb8, int* cb8) {
  if (!tables || Q < 1 || Q > 255) return MI_RTJ_ERR_ARG;
  QTab t;
  build_qtab(Q, &t);
  memcpy(tables, t.liqt, sizeof t.liqt);
  memcpy(tables + 64, t.ciqt, sizeof t.ciqt);
  if (lb8) *lb8 = t.lb8;
  if (cb8) *cb8 = t.cb8;
  return MI_RTJ_OK;
}

}  // extern "C"
