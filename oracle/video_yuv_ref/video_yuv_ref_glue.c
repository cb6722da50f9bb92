/*
 * oracle/video_yuv_ref/video_yuv_ref_glue.c — TEST-ONLY: the little of bgav and gavl that the reference's
 * lib/video_yuv.c calls, and one entry point for ctypes (tests/yuvref.py): fourcc, width, height, packet -> the planes as
 * the decoder left them.  Linked with the reference's file into oracle/_ref/libvideo_yuv_ref.so; this repository's own
 * text.
 */
#include <stdlib.h>
#include <string.h>

#include <avdec_private.h>

void bgav_init_video_decoders_yuv(void);

/* ---- plane geometry of the formats these decoders set: rows and bytes a row ---- */
typedef struct { int planes, row_bytes[GAVL_MAX_PLANES], rows[GAVL_MAX_PLANES]; } geometry_t;

static int geometry_of(int pixelformat, int w, int h, geometry_t *g) {
  int sub_h = 1, sub_v = 1, bytes = 1;
  memset(g, 0, sizeof *g);
  switch (pixelformat) {
    case GAVL_YUY2:
    case GAVL_UYVY: g->planes = 1, g->row_bytes[0] = 2 * w, g->rows[0] = h; return 1;
    case GAVL_YUVA_32: g->planes = 1, g->row_bytes[0] = 4 * w, g->rows[0] = h; return 1;
    case GAVL_YUV_420_P: sub_h = 2, sub_v = 2; break;
    case GAVL_YUV_410_P: sub_h = 4, sub_v = 4; break;
    case GAVL_YUVJ_422_P: sub_h = 2; break;
    case GAVL_YUV_444_P: break;
    case GAVL_YUV_444_P_16: bytes = 2; break;
    case GAVL_YUV_422_P_16: sub_h = 2, bytes = 2; break;
    default: return 0;
  }
  g->planes = 3;
  g->row_bytes[0] = w * bytes, g->rows[0] = h;
  g->row_bytes[1] = g->row_bytes[2] = (w + sub_h - 1) / sub_h * bytes;
  g->rows[1] = g->rows[2] = (h + sub_v - 1) / sub_v;
  return 1;
}

/* ---- bgav ---- */
#define MI_YUVREF_MAX_DECODERS 16
static bgav_video_decoder_t *g_decoders[MI_YUVREF_MAX_DECODERS];
static int g_num_decoders;

void bgav_video_decoder_register(bgav_video_decoder_t *dec) {
  if (g_num_decoders < MI_YUVREF_MAX_DECODERS) g_decoders[g_num_decoders++] = dec;
}

typedef struct { bgav_packet_t *packet; int served, returned; } one_packet_t;

gavl_source_status_t bgav_stream_get_packet_read(bgav_stream_t *s, bgav_packet_t **p) {
  one_packet_t *q = s->harness;
  if (q->served) return GAVL_SOURCE_EOF;
  q->served = 1;
  *p = q->packet;
  return GAVL_SOURCE_OK;
}

void bgav_stream_done_packet_read(bgav_stream_t *s, bgav_packet_t *p) {
  one_packet_t *q = s->harness;
  if (p == q->packet) q->returned = 1;
}

void bgav_set_video_frame_from_packet(const bgav_packet_t *p, gavl_video_frame_t *f) {
  f->timestamp = p->pts, f->duration = p->duration, f->timecode = p->timecode;
  f->dst_x = p->dst_x, f->dst_y = p->dst_y, f->src_rect = p->src_rect;
}

/* ---- gavl ---- */
void gavl_dictionary_set_string(gavl_dictionary_t *d, const char *key, const char *val) {
  if (d && !strcmp(key, GAVL_META_FORMAT)) {
    strncpy(d->format, val, sizeof d->format - 1);
    d->format[sizeof d->format - 1] = 0;
  }
}

gavl_video_frame_t *gavl_video_frame_create(const gavl_video_format_t *format) {
  (void)format; /* video_yuv.c passes NULL: a frame without plane memory */
  return calloc(1, sizeof(gavl_video_frame_t));
}

void gavl_video_frame_null(gavl_video_frame_t *f) { memset(f->planes, 0, sizeof f->planes); }

void gavl_video_frame_destroy(gavl_video_frame_t *f) { free(f); } /* (its planes were never its own) */

void gavl_video_frame_copy(const gavl_video_format_t *format, gavl_video_frame_t *dst, const gavl_video_frame_t *src) {
  geometry_t g;
  if (!geometry_of(format->pixelformat, format->image_width, format->image_height, &g)) abort();
  for (int p = 0; p < g.planes; p++)
    for (int r = 0; r < g.rows[p]; r++)
      memcpy(dst->planes[p] + (size_t)r * dst->strides[p], src->planes[p] + (size_t)r * src->strides[p], (size_t)g.row_bytes[p]);
}

void gavl_video_frame_copy_metadata(gavl_video_frame_t *dst, const gavl_video_frame_t *src) {
  dst->timestamp = src->timestamp, dst->duration = src->duration, dst->timecode = src->timecode;
  dst->dst_x = src->dst_x, dst->dst_y = src->dst_y, dst->src_rect = src->src_rect;
}

/* ---- the entry point ---- */
int mi_yuvref_num_decoders(void) {
  if (!g_num_decoders) bgav_init_video_decoders_yuv();
  return g_num_decoders;
}

/* the first fourcc of decoder i, in the order of registration */
uint32_t mi_yuvref_fourcc(int i) { return i >= 0 && i < mi_yuvref_num_decoders() ? g_decoders[i]->fourccs[0] : 0; }

enum { MI_YUVREF_SLACK = 24, MI_YUVREF_FILL = 0xA5 };

/* One packet through the decoder whose first fourcc this is.  out takes the planes back to back, each as its rows at
 * the format's row width (geometry_of: gavl's, for the pixel format the decoder set); info takes 14 ints: the pixel format,
 * the plane count, then for each of up to 4 planes row bytes, rows and the stride the decoder left (the packet's, where
 * it hands its own frame on in s->vframe; else the output frame's, which this file makes MI_YUVREF_SLACK bytes wider than
 * the row).  Returns the bytes written to out; 0 for a packet of no bytes (skipped); -1 unknown fourcc, -2 init refused,
 * -3 decode did not answer OK, -4 a pixel format this file has no geometry for, -5 out too small, -6 the decoder wrote
 * between the rows of the output frame, -7 the packet did not come back at the next call */
long mi_yuvref_decode(uint32_t fourcc, int w, int h, const uint8_t *packet, int len, uint8_t *out, long out_size, int32_t *info) {
  bgav_video_decoder_t *dec = NULL;
  bgav_stream_t s;
  gavl_video_format_t fmt;
  gavl_dictionary_t meta;
  gavl_compression_info_t ci;
  bgav_packet_t pkt;
  one_packet_t q;
  gavl_video_frame_t own, *got;
  geometry_t g;
  uint8_t *mem = NULL, *copy;
  long ret = 0;
  for (int i = 0; i < mi_yuvref_num_decoders() && !dec; i++)
    if (g_decoders[i]->fourccs[0] == fourcc) dec = g_decoders[i];
  if (!dec) return -1;
  memset(&s, 0, sizeof s), memset(&fmt, 0, sizeof fmt), memset(&meta, 0, sizeof meta), memset(&ci, 0, sizeof ci);
  memset(&pkt, 0, sizeof pkt), memset(&q, 0, sizeof q), memset(&own, 0, sizeof own);
  fmt.image_width = fmt.frame_width = w, fmt.image_height = fmt.frame_height = h;
  ci.flags = GAVL_COMPRESSION_HAS_P_FRAMES;
  s.fourcc = fourcc, s.m = &meta, s.ci = &ci, s.data.video.format = &fmt, s.harness = &q;
  copy = malloc(len > 0 ? (size_t)len : 1); /* exactly the packet: a read past it is a read past an allocation */
  if (len > 0) memcpy(copy, packet, (size_t)len);
  pkt.buf.buf = copy, pkt.buf.len = len;
  q.packet = &pkt;
  if (!dec->init(&s)) {
    free(copy);
    return -2;
  }
  if (!geometry_of(fmt.pixelformat, w, h, &g)) ret = -4;
  if (!ret && !s.vframe) { /* the decoder copies: an output frame with strides wider than the rows */
    size_t total = 0;
    for (int p = 0; p < g.planes; p++) total += (size_t)(g.row_bytes[p] + MI_YUVREF_SLACK) * (size_t)g.rows[p];
    mem = malloc(total ? total : 1);
    memset(mem, MI_YUVREF_FILL, total);
    total = 0;
    for (int p = 0; p < g.planes; p++) {
      own.planes[p] = mem + total, own.strides[p] = g.row_bytes[p] + MI_YUVREF_SLACK;
      total += (size_t)own.strides[p] * (size_t)g.rows[p];
    }
  }
  if (!ret && dec->decode(&s, s.vframe ? NULL : &own) != GAVL_SOURCE_OK) ret = -3;
  got = s.vframe ? s.vframe : &own;
  if (!ret && len > 0) {
    long at = 0;
    info[0] = fmt.pixelformat, info[1] = g.planes;
    for (int p = 0; p < g.planes && ret >= 0; p++) {
      info[2 + 3 * p] = g.row_bytes[p], info[3 + 3 * p] = g.rows[p], info[4 + 3 * p] = got->strides[p];
      if (at + (long)g.row_bytes[p] * g.rows[p] > out_size) {
        ret = -5;
        break;
      }
      for (int r = 0; r < g.rows[p]; r++) {
        const uint8_t *row = got->planes[p] + (size_t)r * got->strides[p];
        memcpy(out + at, row, (size_t)g.row_bytes[p]);
        at += g.row_bytes[p];
        if (!s.vframe)
          for (int k = g.row_bytes[p]; k < got->strides[p]; k++)
            if (row[k] != MI_YUVREF_FILL) ret = -6;
      }
    }
    if (ret >= 0) ret = at;
  }
  if (ret >= 0) { /* the next call gives the packet back and finds the stream at its end */
    if (dec->decode(&s, s.vframe ? NULL : &own) != GAVL_SOURCE_EOF || !q.returned) ret = -7;
  }
  dec->close(&s);
  free(mem);
  free(copy);
  return ret;
}
