/*
 * oracle/dvframe_ref/avdec_private.h — TEST-ONLY stand-in for what the reference's lib/dvframe.c takes from gavl and from
 * its own avdec_private.h, so that oracle/Makefile can compile that file, unchanged and straight from the reference
 * tree, into oracle/_ref/libdvframe_ref.so.  This repository's own text: it names the reference's identifiers and
 * copies none of its lines.  Only the members dvframe.c reads or writes exist; the values of the tags are this file's
 * choice (the pixel formats are numbered as include/mi_dvframe.h numbers its MI_DV_PIX_* classes).
 */
#ifndef MI_ORACLE_DVFRAME_REF_AVDEC_PRIVATE_H
#define MI_ORACLE_DVFRAME_REF_AVDEC_PRIVATE_H

#include <stdint.h>

typedef enum { GAVL_YUV_411_P = 0, GAVL_YUV_420_P = 1, GAVL_YUV_422_P = 2 } gavl_pixelformat_t;
typedef enum { GAVL_SAMPLE_NONE = 0, GAVL_SAMPLE_S16 = 3 } gavl_sample_format_t;
typedef enum { GAVL_INTERLEAVE_NONE = 0, GAVL_INTERLEAVE_2 = 1, GAVL_INTERLEAVE_ALL = 2 } gavl_interleave_mode_t;

typedef struct {
  int samples_per_frame, samplerate, num_channels;
  gavl_sample_format_t sample_format;
  gavl_interleave_mode_t interleave_mode;
} gavl_audio_format_t;

typedef struct {
  uint32_t frame_width, frame_height, image_width, image_height, pixel_width, pixel_height;
  gavl_pixelformat_t pixelformat;
  int frame_duration, timescale;
} gavl_video_format_t;

#define MI_DVREF_MAX_CHANNELS 8
typedef struct {
  union { uint8_t *u_8[MI_DVREF_MAX_CHANNELS]; int16_t *s_16[MI_DVREF_MAX_CHANNELS]; } channels;
  int valid_samples;
} gavl_audio_frame_t;

typedef uint64_t gavl_timecode_t;
#define GAVL_TIMECODE_DROP_FRAME 1
typedef struct { int int_framerate, flags; } gavl_timecode_format_t;

typedef struct { uint8_t *buf; int len, alloc; } gavl_buffer_t;
typedef struct {
  gavl_buffer_t buf;
  int64_t duration;
  uint32_t flags;
} bgav_packet_t;
#define MI_DVREF_KEYFRAME 0x100
#define PACKET_SET_KEYFRAME(p) ((p)->flags |= MI_DVREF_KEYFRAME)

typedef struct bgav_stream_s {
  uint32_t fourcc;
  struct {
    struct { gavl_audio_format_t *format; } audio;
    struct { gavl_video_format_t *format; } video;
  } data;
} bgav_stream_t;

#define BGAV_MK_FOURCC(a, b, c, d) (((uint32_t)(a) << 24) | ((uint32_t)(b) << 16) | ((uint32_t)(c) << 8) | (uint32_t)(d))

/* the ten gavl functions, implemented by dvframe_ref_glue.c */
gavl_audio_frame_t *gavl_audio_frame_create(const gavl_audio_format_t *format);
void gavl_audio_frame_null(gavl_audio_frame_t *f);
void gavl_audio_frame_destroy(gavl_audio_frame_t *f);
int gavl_audio_frame_from_data(gavl_audio_frame_t *f, const gavl_audio_format_t *format, uint8_t *data, int len);
int gavl_audio_format_buffer_size(const gavl_audio_format_t *format);
void gavl_audio_format_copy(gavl_audio_format_t *dst, const gavl_audio_format_t *src);
void gavl_video_format_copy(gavl_video_format_t *dst, const gavl_video_format_t *src);
void gavl_set_channel_setup(gavl_audio_format_t *format);
void gavl_packet_alloc(bgav_packet_t *p, int len);
void gavl_timecode_from_hmsf(gavl_timecode_t *tc, int hours, int minutes, int seconds, int frames);

#endif
