/*
 * oracle/dvframe_ref/dvframe_ref_glue.c — TEST-ONLY: what the reference's lib/dvframe.c needs from gavl (ten small
 * functions) and flat entry points for ctypes around its bgav_dv_dec_* calls (tests/dvref.py).  Linked with the
 * reference's file into oracle/_ref/libdvframe_ref.so; this repository's own text.
 *
 * An audio buffer is a fixed MI_DVREF_PAIR_BYTES per stereo pair, pair k at k * MI_DVREF_PAIR_BYTES: the largest slot the
 * de-shuffle can reach is 107 + 35 * 108 = 3887, byte 7775.  gavl_packet_alloc hands out zeroed bytes, so what comes back
 * is what the reference writes into a zeroed buffer.
 */
#include <stdlib.h>
#include <string.h>

#include <avdec_private.h>
#include <dvframe.h>

#define MI_DVREF_PAIR_BYTES 8192
#define MI_DVREF_NO_PROFILE (-100) /* dv_frame_profile answered NULL: the other calls would dereference it */
#define MI_DVREF_UNDEFINED (-101)  /* the reference would write through a NULL pair buffer */
#define MI_DVREF_LARGEST_FRAME 576000
#define MI_DVREF_FIRST_SUBCODE_PACK (80 + 3 + 3)
#define MI_DVREF_SOURCE_PACK (80 * 6 + 80 * 16 * 3 + 3)
#define MI_DVREF_CONTROL_PACK (80 * 5 + 48 + 5)

/* ---- gavl ---- */
gavl_audio_frame_t *gavl_audio_frame_create(const gavl_audio_format_t *format) {
  (void)format; /* dvframe.c passes NULL: no sample memory of its own */
  return calloc(1, sizeof(gavl_audio_frame_t));
}

void gavl_audio_frame_null(gavl_audio_frame_t *f) { memset(f, 0, sizeof *f); }

void gavl_audio_frame_destroy(gavl_audio_frame_t *f) { free(f); }

int gavl_audio_format_buffer_size(const gavl_audio_format_t *format) { return (format->num_channels + 1) / 2 * MI_DVREF_PAIR_BYTES; }

int gavl_audio_frame_from_data(gavl_audio_frame_t *f, const gavl_audio_format_t *format, uint8_t *data, int len) {
  memset(f, 0, sizeof *f);
  for (int c = 0; c < format->num_channels && c < MI_DVREF_MAX_CHANNELS; c++) /* both channels of a pair: interleaved in its buffer */
    if ((c / 2 + 1) * MI_DVREF_PAIR_BYTES <= len) f->channels.u_8[c] = data + c / 2 * MI_DVREF_PAIR_BYTES + (c & 1) * 2;
  return 1;
}

void gavl_audio_format_copy(gavl_audio_format_t *dst, const gavl_audio_format_t *src) { *dst = *src; }
void gavl_video_format_copy(gavl_video_format_t *dst, const gavl_video_format_t *src) { *dst = *src; }
void gavl_set_channel_setup(gavl_audio_format_t *format) { (void)format; }

void gavl_packet_alloc(bgav_packet_t *p, int len) {
  if (len > p->buf.alloc) {
    free(p->buf.buf);
    p->buf.buf = malloc((size_t)len);
    p->buf.alloc = len;
  }
  memset(p->buf.buf, 0, (size_t)len);
  p->buf.len = len;
}

/* the encoding of a timecode is this file's: one byte each */
void gavl_timecode_from_hmsf(gavl_timecode_t *tc, int hours, int minutes, int seconds, int frames) {
  *tc = (gavl_timecode_t)(uint32_t)hours << 24 | (gavl_timecode_t)(uint32_t)minutes << 16 | (gavl_timecode_t)(uint32_t)seconds << 8 |
        (gavl_timecode_t)(uint32_t)frames;
}

/* ---- entry points ---- */
static uint8_t g_scratch[MI_DVREF_LARGEST_FRAME];

/* a decoder with the frame's profile, or NULL where the profile is NULL.  Told from outside: with a timecode pack at
 * the first place of the scan, bgav_dv_dec_get_timecode_format writes its argument exactly when the profile is there.
 * The scratch frame has the header block and the VAUX block of `frame` (all the profile is read from) and is left set */
static bgav_dv_dec_t *open_on(const uint8_t *frame) {
  bgav_dv_dec_t *d = bgav_dv_dec_create();
  gavl_timecode_format_t tf = {-1, -1};
  memset(g_scratch, 0, sizeof g_scratch);
  memcpy(g_scratch, frame, 480);
  g_scratch[MI_DVREF_FIRST_SUBCODE_PACK] = 0x13;
  bgav_dv_dec_set_header(d, g_scratch);
  bgav_dv_dec_set_frame(d, g_scratch);
  bgav_dv_dec_get_timecode_format(d, &tf);
  if (tf.int_framerate == -1 && tf.flags == -1) {
    bgav_dv_dec_destroy(d);
    return NULL;
  }
  return d;
}

/* out: frame size, image width, height, pixel format, frame duration, timescale, timecode rate, timecode flags,
 * pixel aspect 4:3 (num, den), 16:9 (num, den); 12 ints.  header: 480 bytes.  Returns 1, or MI_DVREF_NO_PROFILE */
int mi_dvref_profile(const uint8_t *header, int32_t *out) {
  bgav_dv_dec_t *d = open_on(header);
  gavl_timecode_format_t tf = {0, 0};
  gavl_video_format_t fmt;
  uint32_t num, den;
  if (!d) return MI_DVREF_NO_PROFILE;
  memset(&fmt, 0, sizeof fmt);
  g_scratch[MI_DVREF_CONTROL_PACK] = 0; /* no control pack: 4:3 */
  bgav_dv_dec_get_video_format(d, &fmt);
  bgav_dv_dec_get_timecode_format(d, &tf);
  out[0] = bgav_dv_dec_get_frame_size(d);
  out[1] = (int32_t)fmt.image_width, out[2] = (int32_t)fmt.image_height, out[3] = (int32_t)fmt.pixelformat;
  out[4] = fmt.frame_duration, out[5] = fmt.timescale;
  out[6] = tf.int_framerate, out[7] = tf.flags;
  out[8] = (int32_t)fmt.pixel_width, out[9] = (int32_t)fmt.pixel_height;
  g_scratch[MI_DVREF_CONTROL_PACK] = 0x61, g_scratch[MI_DVREF_CONTROL_PACK + 2] = 0x02; /* the control pack says 16:9 */
  bgav_dv_dec_get_pixel_aspect(d, &num, &den);
  out[10] = (int32_t)num, out[11] = (int32_t)den;
  bgav_dv_dec_destroy(d);
  return 1;
}

/* what bgav_dv_dec_init_audio leaves in a zeroed format for this frame: samplerate (0: untouched), channels, sample
 * format, interleave mode, samples per frame, the stream's fourcc; 6 ints.  The caller keeps the rate field at 0..2 */
int mi_dvref_audio_format(const uint8_t *frame, int32_t *out) {
  bgav_dv_dec_t *d = open_on(frame);
  gavl_audio_format_t fmt;
  bgav_stream_t s;
  if (!d) return MI_DVREF_NO_PROFILE;
  memset(&fmt, 0, sizeof fmt);
  memset(&s, 0, sizeof s);
  s.data.audio.format = &fmt;
  bgav_dv_dec_set_frame(d, (uint8_t *)frame);
  bgav_dv_dec_init_audio(d, &s);
  out[0] = fmt.samplerate, out[1] = fmt.num_channels, out[2] = (int32_t)fmt.sample_format, out[3] = (int32_t)fmt.interleave_mode;
  out[4] = fmt.samples_per_frame, out[5] = (int32_t)s.fourcc;
  bgav_dv_dec_destroy(d);
  return 1;
}

/* dv_extract_audio through bgav_dv_dec_get_audio_packet into `pairs` (1, 2 or 4) zeroed pair buffers: pcm takes
 * pairs * MI_DVREF_PAIR_BYTES bytes, *samples the packet's duration (dv_extract_audio's return value).  The pair count
 * is what init_audio makes of the stype of the frame it is shown: a scratch frame with a 16-bit 48 kHz source pack of
 * the stype that gives it; then the frame under test is set.  Returns 1, MI_DVREF_NO_PROFILE or MI_DVREF_UNDEFINED */
int mi_dvref_audio(const uint8_t *frame, int pairs, uint8_t *pcm, int32_t *samples) {
  bgav_dv_dec_t *d;
  gavl_audio_format_t fmt;
  bgav_stream_t s;
  bgav_packet_t p;
  uint32_t w, h;
  if (pairs != 1 && pairs != 2 && pairs != 4) return MI_DVREF_UNDEFINED;
  if (!(d = open_on(frame))) return MI_DVREF_NO_PROFILE;
  bgav_dv_dec_get_image_size(d, &w, &h);
  {
    /* where the reference has no defined answer it is not called (tests/dvref.py keeps the same rules and never gets
     * here): a first half frame of 720p starts at the third pair buffer, which is NULL with fewer than four pairs, and
     * walks past the fourth in 12-bit mode, as every 12-bit 1080 frame does; a rate above 2 indexes past the table */
    const uint8_t *as = frame + MI_DVREF_SOURCE_PACK;
    const int first_half = h == 720 && ((frame[1] >> 2) & 3) == 0, has = as[0] == 0x50, twelve = has && (as[4] & 7) == 1;
    if ((first_half && (pairs < 4 || twelve)) || (h == 1080 && twelve) || (has && (as[4] & 7) <= 1 && ((as[4] >> 3) & 7) > 2)) {
      bgav_dv_dec_destroy(d);
      return MI_DVREF_UNDEFINED;
    }
  }
  memset(&fmt, 0, sizeof fmt);
  memset(&s, 0, sizeof s);
  memset(&p, 0, sizeof p);
  s.data.audio.format = &fmt;
  g_scratch[MI_DVREF_SOURCE_PACK] = 0x50;
  g_scratch[MI_DVREF_SOURCE_PACK + 3] = pairs == 4 ? 3 : pairs == 2 ? 2 : 0;
  g_scratch[MI_DVREF_SOURCE_PACK + 4] = 0;
  bgav_dv_dec_init_audio(d, &s);
  bgav_dv_dec_set_frame(d, (uint8_t *)frame);
  bgav_dv_dec_get_audio_packet(d, &p);
  *samples = (int32_t)p.duration;
  memcpy(pcm, p.buf.buf, (size_t)pairs * MI_DVREF_PAIR_BYTES);
  free(p.buf.buf);
  bgav_dv_dec_destroy(d);
  return fmt.num_channels == 2 * pairs && p.buf.len == pairs * MI_DVREF_PAIR_BYTES && (p.flags & MI_DVREF_KEYFRAME) ? 1 : MI_DVREF_UNDEFINED;
}

/* out: timecode found, hours, minutes, seconds, frames; date found, year, month, day; time found, hour, minute, second;
 * pixel aspect num, den; 15 ints.  What a call that found nothing leaves alone is 0.  Returns 1 or MI_DVREF_NO_PROFILE */
int mi_dvref_meta(const uint8_t *frame, int32_t *out) {
  bgav_dv_dec_t *d = open_on(frame);
  gavl_timecode_t tc = 0;
  int a = 0, b = 0, c = 0;
  uint32_t num, den;
  if (!d) return MI_DVREF_NO_PROFILE;
  memset(out, 0, 15 * sizeof *out);
  bgav_dv_dec_set_frame(d, (uint8_t *)frame);
  out[0] = bgav_dv_dec_get_timecode(d, &tc);
  if (out[0]) out[1] = (int32_t)(tc >> 24 & 0xff), out[2] = (int32_t)(tc >> 16 & 0xff), out[3] = (int32_t)(tc >> 8 & 0xff), out[4] = (int32_t)(tc & 0xff);
  out[5] = bgav_dv_dec_get_date(d, &a, &b, &c);
  if (out[5]) out[6] = a, out[7] = b, out[8] = c;
  a = b = c = 0;
  out[9] = bgav_dv_dec_get_time(d, &a, &b, &c);
  if (out[9]) out[10] = a, out[11] = b, out[12] = c;
  bgav_dv_dec_get_pixel_aspect(d, &num, &den);
  out[13] = (int32_t)num, out[14] = (int32_t)den;
  bgav_dv_dec_destroy(d);
  return 1;
}
