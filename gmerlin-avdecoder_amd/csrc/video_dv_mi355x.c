/*
 * video_dv_mi355x.c — a bgav_video_decoder_t for DV video on an MI355X: at 25 Mbit/s 525/60 (NTSC, 4:1:1), 625/50
 * (PAL) in the IEC 4:2:0 profile and, opted in with MI_DV_625_411=1, 625/50 in the DVCPRO 4:1:1 profile; at 50 Mbit/s
 * (DVCPRO50) both line systems in 4:2:2.
 *
 * In gmerlin-avdecoder DV pixels are libavcodec's: lib/dvframe.c:663-676 hands each 120,000-byte DIF frame on as a
 * video packet, and the "FFmpeg DV decoder" entry of lib/video_ffmpeg.c:1572-1575 decodes it for the fourccs of
 * lib/video.c:122-145 (bgav_dv_fourccs).  This file registers a decoder for the same fourccs that is asked FIRST
 * (first match wins, lib/codecs.c:246-279): its .probe accepts a stream only when a gfx950 device is usable and the
 * stream is 720 x 480, or 720 x 576 with the pixel format GAVL_YUV_420_P or GAVL_YUV_422_P.  The demultiplexer sets
 * the pixel format from the DIF profile (lib/dvframe.c:490-500; lib/parse_dv.c:51 for DV in other containers): a stream
 * of either height with GAVL_YUV_422_P is DVCPRO50 and decodes to 4:2:2 pictures; a 720 x 480 stream with any other or no
 * pixel format is 525/60 4:1:1; a 625/50 stream at 25 Mbit/s is ours in the IEC 4:2:0 profile and, only where the process
 * environment holds MI_DV_625_411=1, in the DVCPRO 4:1:1 profile (720 x 576 with GAVL_YUV_411_P, lib/dvframe.c:149-169):
 * that layout is the least certain of this decoder's (include/mi_dv.h: parity unpinned), so it is opt-in until it is
 * pinned.  Unset, or set to anything else, such a stream is declined as before.  Every other DV flavour (a 720 x 576
 * stream whose pixel format is not known, DVCPRO HD) and every host without the device still go to the FFmpeg decoder.  The pixels come from include/mi_dv.h: mi_dv_decode_frame_sys with the
 * system the stream was opened with.
 *
 * Integration: add this file to lib/Makefile.am, declare
 * bgav_init_video_decoders_dv_mi355x() in include/codecs.h and call it in bgav_codecs_init (lib/codecs.c:160-200) BEFORE
 * bgav_init_video_decoders_ffmpeg().  Host code stays C.
 *
 * Shape: lib/video_rtjpeg.c's own — synchronous, one packet in, one picture out, into the caller's frame with the
 * caller's strides (copy mode; a skipped frame, f == NULL, consumes its packet and decodes nothing).
 *
 * Damage.  A DV stream flags the macroblocks a deck could not correct (STA, the high nibble of byte 3 of a DIF block), and
 * libavcodec keeps the last good pixels there.  With MI_DV_HOLD=1 in the process environment .decode does the same: it
 * calls mi_dv_decode_frame_held with the default mask (MI_DV_STA_ERRORS), the instance keeps the last DECODED picture as
 * the source (a skipped frame decodes nothing and leaves it alone), and .resync forgets it (mi_dv_hold_reset).  Opt-in
 * because which STA values mean "error" is this repository's reading of IEC 61834-2 from memory, unpinned like the decoder
 * itself; unset, or set to anything else, the wrapper calls mi_dv_decode_frame_sys exactly as before.
 *
 * PARITY UNPINNED: see include/mi_dv.h.
 */
#include <stdlib.h>
#include <string.h>

#include <avdec_private.h>
#include <codecs.h>

#include "mi_dv.h"

#define LOG_DOMAIN "video_dv_mi355x"

typedef struct {
  mi_dv_ctx *ctx;
  int system; /* MI_DV_SYS_*, from the stream's format */
} dv_hip_priv_t;

/* the fourccs of lib/video.c:122-145; inside the tree the library's own array is used */
#ifdef MI_COMPAT_LITE
static const uint32_t dv_fourccs[] = {
    BGAV_MK_FOURCC('d', 'v', 's', 'd'), BGAV_MK_FOURCC('D', 'V', 'S', 'D'), BGAV_MK_FOURCC('d', 'v', 'h', 'd'),
    BGAV_MK_FOURCC('d', 'v', 's', 'l'), BGAV_MK_FOURCC('d', 'v', '2', '5'), BGAV_MK_FOURCC('D', 'V', ' ', ' '),
    BGAV_MK_FOURCC('d', 'v', 'c', 'p'), BGAV_MK_FOURCC('d', 'v', 'c', ' '), BGAV_MK_FOURCC('d', 'v', 'p', 'p'),
    BGAV_MK_FOURCC('A', 'V', 'd', 'v'), BGAV_MK_FOURCC('A', 'V', 'd', '1'), 0x00};
#define DV_FOURCCS dv_fourccs
#else
#define DV_FOURCCS bgav_dv_fourccs /* include/avdec_private.h:1435 */
#endif

/* MI_DV_625_411=1 in the process environment: 720 x 576 GAVL_YUV_411_P streams are taken too (read where it is needed, so
 * that .probe and .init of one process agree) */
static int dv_625_411_opted_in(void) {
  const char *e = getenv("MI_DV_625_411");
  return e && !strcmp(e, "1");
}

/* MI_DV_HOLD=1 in the process environment: macroblocks flagged as errors keep the last decoded picture's pixels (read where
 * it is needed, like MI_DV_625_411) */
static int dv_hold_opted_in(void) {
  const char *e = getenv("MI_DV_HOLD");
  return e && !strcmp(e, "1");
}

/* the system of a stream by its format: GAVL_YUV_422_P is the 50 Mbit/s system of the stream's height; otherwise
 * 720 x 480 is 525/60 4:1:1 and 720 x 576 is 625/50 in the 4:2:0 profile, or in the 4:1:1 profile when opted in; -1 else */
static int dv_system(const gavl_video_format_t *fmt) {
  if (!fmt || fmt->image_width != MI_DV_WIDTH) return -1;
  if (fmt->pixelformat == GAVL_YUV_422_P) {
    if (fmt->image_height == MI_DV_HEIGHT) return MI_DV_SYS_525_60_422;
    if (fmt->image_height == MI_DV_625_HEIGHT) return MI_DV_SYS_625_50_422;
    return -1;
  }
  if (fmt->image_height == MI_DV_HEIGHT) return MI_DV_SYS_525_60;
  if (fmt->image_height == MI_DV_625_HEIGHT && fmt->pixelformat == GAVL_YUV_420_P) return MI_DV_SYS_625_50;
  if (fmt->image_height == MI_DV_625_HEIGHT && fmt->pixelformat == GAVL_YUV_411_P && dv_625_411_opted_in())
    return MI_DV_SYS_625_50_411;
  return -1;
}

/* .probe (include/avdec_private.h:95): only what this decoder can do, so that the FFmpeg decoder registered behind it
 * gets everything else */
static int probe_dv_hip(const gavl_dictionary_t *stream) {
  if (mi_dv_device_count() <= 0) return 0;
  return dv_system(gavl_stream_get_video_format(stream)) >= 0;
}

static int init_dv_hip(bgav_stream_t *s) {
  dv_hip_priv_t *priv;
  const int system = dv_system(s->data.video.format);
  if (system < 0) { /* (a caller that skipped .probe) */
    gavl_log(GAVL_LOG_ERROR, LOG_DOMAIN,
             "Only 525/60 4:1:1 (720x480) and 625/50 4:2:0 (720x576) 25 Mbit/s DV, 625/50 4:1:1 (720x576) with MI_DV_625_411=1 "
             "and 4:2:2 50 Mbit/s DV of both sizes are decoded on the MI355X");
    return 0;
  }
  priv = calloc(1, sizeof(*priv));
  if (!priv) return 0;
  priv->ctx = mi_dv_create(-1);
  if (!priv->ctx) {
    gavl_log(GAVL_LOG_ERROR, LOG_DOMAIN, "Cannot open MI355X DV decoder: %s", mi_dv_last_error(NULL));
    free(priv);
    return 0;
  }
  priv->system = system;
  s->decoder_priv = priv;
  s->data.video.format->frame_width = MI_DV_WIDTH;
  if (system == MI_DV_SYS_525_60) {
    s->data.video.format->frame_height = MI_DV_HEIGHT;
    s->data.video.format->pixelformat = GAVL_YUV_411_P; /* lib/dvframe.c:119: the 525/60 profile's pix_fmt */
  } else if (system == MI_DV_SYS_525_60_422) {
    s->data.video.format->frame_height = MI_DV_HEIGHT; /* the pixel format stays GAVL_YUV_422_P (lib/dvframe.c:170-211) */
  } else {
    /* the pixel format stays GAVL_YUV_420_P (lib/dvframe.c:129-148), GAVL_YUV_411_P (:149-169) or GAVL_YUV_422_P */
    s->data.video.format->frame_height = MI_DV_625_HEIGHT;
  }
  gavl_dictionary_set_string(s->m, GAVL_META_FORMAT, "DV");
  return 1;
}

static gavl_source_status_t decode_dv_hip(bgav_stream_t *s, gavl_video_frame_t *f) {
  dv_hip_priv_t *priv = s->decoder_priv;
  bgav_packet_t *p = NULL;
  gavl_source_status_t st;
  if ((st = bgav_stream_get_packet_read(s, &p)) != GAVL_SOURCE_OK) return st;
  if (!f) { /* skip frame: the packet is consumed, nothing is decoded (every DV frame is a key frame) */
    bgav_stream_done_packet_read(s, p);
    return GAVL_SOURCE_OK;
  }
  if ((dv_hold_opted_in() ? mi_dv_decode_frame_held(priv->ctx, priv->system, p->buf.buf, (size_t)p->buf.len,
                                                    (uint8_t *const *)f->planes, f->strides, MI_DV_STA_ERRORS, NULL)
                          : mi_dv_decode_frame_sys(priv->ctx, priv->system, p->buf.buf, (size_t)p->buf.len,
                                                   (uint8_t *const *)f->planes, f->strides)) != MI_DV_OK) {
    gavl_log(GAVL_LOG_ERROR, LOG_DOMAIN, "Decoding failed: %s", mi_dv_last_error(priv->ctx));
    bgav_stream_done_packet_read(s, p);
    return GAVL_SOURCE_EOF; /* never abort: errors are EOF + a log line, as everywhere in the library */
  }
  bgav_set_video_frame_from_packet(p, f);
  bgav_stream_done_packet_read(s, p);
  return GAVL_SOURCE_OK;
}

/* .resync (after a seek): the picture decoded last is not the stream's previous one any more */
static void resync_dv_hip(bgav_stream_t *s) {
  dv_hip_priv_t *priv = s->decoder_priv;
  if (priv && dv_hold_opted_in()) mi_dv_hold_reset(priv->ctx);
}

static void close_dv_hip(bgav_stream_t *s) {
  dv_hip_priv_t *priv = s->decoder_priv;
  if (!priv) return;
  mi_dv_destroy(priv->ctx);
  free(priv);
  s->decoder_priv = NULL;
}

static bgav_video_decoder_t dv_hip_decoder = {
    .name = "DV video decoder (MI355X)",
    .fourccs = DV_FOURCCS,
    .probe = probe_dv_hip,
    .init = init_dv_hip,
    .decode = decode_dv_hip,
    .close = close_dv_hip,
    .resync = resync_dv_hip,
};

void bgav_init_video_decoders_dv_mi355x(void) { bgav_video_decoder_register(&dv_hip_decoder); }
