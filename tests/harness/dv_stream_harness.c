/*
 * dv_stream_harness.c — drives csrc/video_dv_mi355x.c the way lib/video.c drives a bgav_video_decoder_t
 * (bgav_video_start: lib/video.c:375-463; read_video_copy: :279-312), for DV streams whose pixel format the
 * demultiplexer set (lib/dvframe.c:490-500).  Only the DV decoder is registered.  The decoder takes a 720 x 576
 * GAVL_YUV_411_P stream only when the environment holds MI_DV_625_411=1; this program passes its environment on unchanged
 * and sets nothing itself, so the caller decides.  PARITY UNPINNED: see include/mi_dv.h.
 *
 *   dv_stream_harness <packets.bin> <image_w> <image_h> <411|420|422|none> <out.bin> [skip_every=N] [pad=P]
 *
 *   411 / 420 / 422 / none  the stream's pixel format before a decoder is chosen: GAVL_YUV_411_P, GAVL_YUV_420_P,
 *                     GAVL_YUV_422_P, or unset
 *   skip_every=N      every N-th frame is skipped (decode(s, NULL): the packet is consumed, no picture)
 *   pad=P             the caller's strides are the plane widths + P bytes
 *
 * packets.bin: repeated { u32 le length, bytes }.  out.bin: for every decoded frame the planes Y, Cb, Cr cropped to the
 * format the decoder announced, tightly packed, followed by 8 bytes pts (le).
 * Exit codes: 0 ok (the stream may have ended early: a decode failure is EOF), 3 no decoder accepted the stream,
 * 4 init failed, 1 usage / io.
 */
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <avdec_private.h>
#include <codecs.h>

/* ---- the compat_lite entry points video_dv_mi355x.c calls (lib/codecs.c:201-279, lib/stream.c, gavl) ---- */
static bgav_video_decoder_t *video_decoders = NULL;
void bgav_video_decoder_register(bgav_video_decoder_t *dec) {
  bgav_video_decoder_t **pp = &video_decoders;
  while (*pp) pp = &(*pp)->next;
  *pp = dec;
  dec->next = NULL;
}
static bgav_video_decoder_t *find_video_decoder(uint32_t fourcc, const gavl_dictionary_t *stream) {
  for (bgav_video_decoder_t *cur = video_decoders; cur; cur = cur->next)
    for (int i = 0; cur->fourccs[i]; i++)
      if (cur->fourccs[i] == fourcc && (!cur->probe || cur->probe(stream))) return cur;
  return NULL;
}

typedef struct {
  gavl_packet_t *pkts;
  int n, next;
} queue_t;
gavl_source_status_t bgav_stream_get_packet_read(bgav_stream_t *s, bgav_packet_t **p) {
  queue_t *q = s->harness;
  if (q->next >= q->n) return GAVL_SOURCE_EOF;
  *p = &q->pkts[q->next++];
  return GAVL_SOURCE_OK;
}
void bgav_stream_done_packet_read(bgav_stream_t *s, bgav_packet_t *p) { (void)s; (void)p; }
void bgav_set_video_frame_from_packet(const bgav_packet_t *p, gavl_video_frame_t *f) {
  f->timestamp = p->pts;
  f->duration = p->duration;
}
void gavl_dictionary_set_string(gavl_dictionary_t *d, const char *key, const char *val) {
  if (!strcmp(key, GAVL_META_FORMAT)) snprintf(d->format, sizeof d->format, "%s", val);
}
const gavl_video_format_t *gavl_stream_get_video_format(const gavl_dictionary_t *stream) { return stream ? stream->vfmt : NULL; }
void gavl_log(int level, const char *domain, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  fprintf(stderr, "[%s] %s: ", level == GAVL_LOG_ERROR ? "error" : "info", domain);
  vfprintf(stderr, fmt, ap);
  fputc('\n', stderr);
  va_end(ap);
}

int main(int argc, char **argv) {
  if (argc < 6)
    return fprintf(stderr, "usage: %s packets.bin w h 411|420|422|none out.bin [skip_every=N] [pad=P]\n", argv[0]), 1;
  const int iw = atoi(argv[2]), ih = atoi(argv[3]);
  int pixfmt;
  if (!strcmp(argv[4], "411")) pixfmt = GAVL_YUV_411_P;
  else if (!strcmp(argv[4], "420")) pixfmt = GAVL_YUV_420_P;
  else if (!strcmp(argv[4], "422")) pixfmt = GAVL_YUV_422_P;
  else if (!strcmp(argv[4], "none")) pixfmt = 0;
  else return fprintf(stderr, "pixel format: 411, 420, 422 or none\n"), 1;
  int skip_every = 0, pad = 0;
  for (int i = 6; i < argc; i++) {
    if (sscanf(argv[i], "skip_every=%d", &skip_every) == 1) continue;
    if (sscanf(argv[i], "pad=%d", &pad) == 1) continue;
    return fprintf(stderr, "unknown argument %s\n", argv[i]), 1;
  }
  if (iw <= 0 || ih <= 0 || pad < 0 || skip_every < 0) return fprintf(stderr, "bad size, skip_every or pad\n"), 1;

  queue_t q = {0};
  FILE *fi = fopen(argv[1], "rb");
  if (!fi) return perror(argv[1]), 1;
  for (;;) {
    uint32_t len;
    if (fread(&len, 4, 1, fi) != 1) break;
    q.pkts = realloc(q.pkts, sizeof(gavl_packet_t) * (q.n + 1));
    gavl_packet_t *p = &q.pkts[q.n];
    memset(p, 0, sizeof *p);
    p->buf.buf = calloc(len + 64, 1);
    p->buf.len = (int)len;
    if (fread(p->buf.buf, 1, len, fi) != len) return fprintf(stderr, "short packet file\n"), 1;
    p->pts = 1000 + 40 * (int64_t)q.n;
    p->duration = 40;
    q.n++;
  }
  fclose(fi);

  bgav_init_video_decoders_dv_mi355x();
  gavl_video_format_t fmt = {.image_width = iw, .image_height = ih, .pixelformat = pixfmt};
  gavl_dictionary_t meta, info;
  memset(&meta, 0, sizeof meta);
  memset(&info, 0, sizeof info);
  info.vfmt = &fmt;
  bgav_stream_t s;
  memset(&s, 0, sizeof s);
  s.fourcc = BGAV_MK_FOURCC('d', 'v', 's', 'd');
  s.m = &meta;
  s.info = &info;
  s.data.video.format = &fmt;
  s.harness = &q;

  bgav_video_decoder_t *dec = find_video_decoder(s.fourcc, s.info);
  if (!dec) return fprintf(stderr, "no video decoder accepted the stream\n"), 3;
  if (!dec->init(&s)) return fprintf(stderr, "decoder init failed\n"), 4;

  /* the planes the decoder announced: 4:1:1 (w / 4 x h: 525/60 and, opted in, 625/50), 4:2:0 (625/50) or 4:2:2 (w / 2 x h) */
  const int cw = fmt.pixelformat == GAVL_YUV_411_P ? iw / 4 : fmt.pixelformat == GAVL_YUV_422_P ? iw / 2 : (iw + 1) / 2;
  const int ch = fmt.pixelformat == GAVL_YUV_411_P || fmt.pixelformat == GAVL_YUV_422_P ? ih : (ih + 1) / 2;
  gavl_video_frame_t f;
  memset(&f, 0, sizeof f);
  f.strides[0] = iw + pad;
  f.strides[1] = f.strides[2] = cw + pad;
  f.planes[0] = calloc((size_t)f.strides[0] * ih, 1);
  f.planes[1] = calloc((size_t)f.strides[1] * ch, 1);
  f.planes[2] = calloc((size_t)f.strides[2] * ch, 1);
  FILE *fo = fopen(argv[5], "wb");
  if (!fo) return perror(argv[5]), 1;
  int nframes = 0, k = 0;
  for (;;) { /* read_video_copy (lib/video.c:279-312) */
    const int skip = skip_every && (++k % skip_every) == 0;
    if (dec->decode(&s, skip ? NULL : &f) != GAVL_SOURCE_OK) break;
    if (skip) continue;
    for (int y = 0; y < ih; y++) fwrite(f.planes[0] + (size_t)y * f.strides[0], 1, iw, fo);
    for (int pl = 1; pl < 3; pl++)
      for (int y = 0; y < ch; y++) fwrite(f.planes[pl] + (size_t)y * f.strides[pl], 1, cw, fo);
    fwrite(&f.timestamp, 8, 1, fo);
    nframes++;
  }
  fclose(fo);
  dec->close(&s);
  fprintf(stderr, "decoder: %s, format %s, frame %dx%d image %dx%d chroma %dx%d\n", dec->name, meta.format, fmt.frame_width,
          fmt.frame_height, iw, ih, cw, ch);
  fprintf(stderr, "%d frames\n", nframes);
  for (int i = 0; i < q.n; i++) free(q.pkts[i].buf.buf);
  free(q.pkts);
  free(f.planes[0]);
  free(f.planes[1]);
  free(f.planes[2]);
  return 0;
}
