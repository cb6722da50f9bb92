/*
 * oracle/video_yuv_ref/avdec_private.h — TEST-ONLY stand-in with which oracle/Makefile compiles the reference's
 * lib/video_yuv.c, unchanged and straight from the reference tree, into oracle/_ref/libvideo_yuv_ref.so.  It starts from
 * what csrc/compat_lite/avdec_private.h declares for the plugin wrappers (included, not edited) and adds the few things
 * only video_yuv.c touches.  This repository's own text; the tag values are opaque here, as they are there.  config.h and
 * codecs.h beside this file are empty: video_yuv.c includes them and takes nothing from them.
 */
#ifndef MI_ORACLE_VIDEO_YUV_REF_AVDEC_PRIVATE_H
#define MI_ORACLE_VIDEO_YUV_REF_AVDEC_PRIVATE_H

#include "../../gmerlin-avdecoder_amd/csrc/compat_lite/avdec_private.h"

#define GAVL_YUY2 0x0401
#define GAVL_UYVY 0x0402
#define GAVL_YUVA_32 0x0403
#define GAVL_YUV_444_P 0x0503
#define GAVL_YUV_410_P 0x0506
#define GAVL_YUVJ_422_P 0x0512
#define GAVL_YUV_444_P_16 0x0523
#define GAVL_YUV_422_P_16 0x0522

#define GAVL_PTR_2_32LE(p) \
  ((uint32_t)((const uint8_t *)(p))[0] | (uint32_t)((const uint8_t *)(p))[1] << 8 | (uint32_t)((const uint8_t *)(p))[2] << 16 | \
   (uint32_t)((const uint8_t *)(p))[3] << 24)

/* implemented by video_yuv_ref_glue.c */
void gavl_video_frame_copy(const gavl_video_format_t *format, gavl_video_frame_t *dst, const gavl_video_frame_t *src);
void gavl_video_frame_copy_metadata(gavl_video_frame_t *dst, const gavl_video_frame_t *src);

#endif
