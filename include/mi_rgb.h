/*
 * mi_rgb.h — C ABI of the MI355X (gfx950) unpacker of the raw RGB family of QuickTime and AVI: what lib/video_qtraw.c
 * ('raw ' at depths 1, 2, 4, 8, 16, 24, 32 and the grey depths 34, 36, 40) and lib/video_aviraw.c ('RGB ', 'RGB3',
 * 'MTV ' at depths 8, 16, 24, 32) decode, n packets resident in device memory -> n tightly packed pictures in one launch.
 * Plain C types only; libmi_rgb.so.
 *
 * PINNED BY STATEMENT, NOT YET BY BUILD: every line of the arithmetic is in the two upstream files and is cited below;
 * the checker is tests/rgbraw.py, which restates the cited lines twice (vectorised, and loop for loop), and the kernels
 * reproduce it byte for byte.  Nothing here is held to a build of the two files yet.
 *
 * A PICTURE is one tightly packed plane, top row first: rows of w * bpp bytes (bpp = bytes per pixel), 16-bit pixels as
 * native uint16_t.  A packet's rows are `stride` bytes apart; "made even" is `if (x & 1) x++` (video_qtraw.c:365-366),
 * "padded to 4" is video_aviraw.c:273-279 over (w * depth + 7) / 8.  A palette entry gives R, G, B = r >> 8, g >> 8,
 * b >> 8 (BGAV_PALETTE_2_RGB24, avdec_private.h:122-125).  video_qtraw.c is Q, video_aviraw.c is A:
 *
 *   codec      lines               packet row stride       bpp  rule
 *   QT1        Q:43-62, :238-254   w / 8, made even        3    pixel i is bit 7 - i % 8 of byte i / 8 (upstream shifts the
 *                                                               byte left in place); it indexes the palette
 *   QT2        Q:64-83 (depth 34:  w / 4, made even        3    two bits a pixel, high bits first
 *              :162-184)
 *   QT4        Q:85-104 (depth 36: w / 2, made even        3    a nibble a pixel, high first
 *              :186-209)
 *   QT8        Q:106-118 (depth    w, made even            3    palette[byte]
 *              40: :211-223)
 *   QT16       Q:120-135           2w                      2    big-endian 16 bits -> native uint16_t
 *   QT24       Q:137-143           3w, made even           3    copy
 *   QT32       Q:145-160           4w                      4    A R G B -> R G B A
 *   AVI8       A:50-60             w, padded to 4          3    palette[byte]; rows bottom-up (A:183-192)
 *   AVI8_GRAY  A:62-72, :231-235   w, padded to 4          1    copy, bottom-up
 *   AVI16      A:76-89             2w, padded to 4         2    copy (little-endian host), bottom-up
 *   MTV16      A:91-104, :247-251  2w, padded to 4         2    bytes swapped, bottom-up
 *   AVI24      A:108-112           3w, padded to 4         3    copy, bottom-up
 *   AVI32      A:114-118           4w                      4    copy, bottom-up
 *
 * Sizes: w and h are positive; w is a multiple of 8 / 4 / 2 for QT1 / QT2 / QT4 (the widths at which upstream's row loop
 * stays inside the row it was given); packets and pictures stay below 2^31 bytes.
 *
 * Palettes: 2^depth entries (QT1 2, QT2 4, QT4 16, QT8 and AVI8 256) of mi_rgb_color; alpha is never read.  A shorter
 * palette is refused: upstream refuses it for QuickTime (Q:242, :259, :292); for AVI it only warns (A:238-241) and would
 * read past the palette, which is undefined there.  The caller brings the palette, as the demultiplexer does upstream:
 * the QuickTime default palettes are not part of this library, and the grey depths 34, 36, 40 are QT2, QT4, QT8 with
 * the caller's grey palette.
 *
 * Two upstream facts that are stated here and not imitated:
 *   - init_qtraw's test for depth 4 is inverted (Q:276): it fails with a palette and dereferences NULL without one, so
 *     upstream never decodes depth 4.  QT4 is scanline_raw_4 as written (Q:85-104), which is byte for byte the function
 *     depth 36 does run (Q:186-209).
 *   - Upstream destroys the packet while it reads sub-byte pixels (`*src <<= n`).  This library never writes a packet.
 */
#ifndef MI_RGB_H
#define MI_RGB_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { MI_RGB_OK = 0, MI_RGB_ERR_ARG = -1, MI_RGB_ERR_HIP = -2, MI_RGB_ERR_NOMEM = -3, MI_RGB_ERR_FORMAT = -4 };
/* the codecs: video_qtraw.c's by depth, then video_aviraw.c's */
enum {
  MI_RGB_QT1 = 0, MI_RGB_QT2 = 1, MI_RGB_QT4 = 2, MI_RGB_QT8 = 3, MI_RGB_QT16 = 4, MI_RGB_QT24 = 5, MI_RGB_QT32 = 6,
  MI_RGB_AVI8 = 7, MI_RGB_AVI8_GRAY = 8, MI_RGB_AVI16 = 9, MI_RGB_MTV16 = 10, MI_RGB_AVI24 = 11, MI_RGB_AVI32 = 12,
  MI_RGB_CODECS = 13
};

/* a palette entry as upstream's gavl_palette_entry_t: 16 bits a component, of which the high byte is used */
typedef struct { uint16_t r, g, b, a; } mi_rgb_color;

/* what a codec makes of a size: packet_bytes = packet_stride * h, picture_bytes = w * bytes_per_pixel * h; palette_entries
 * is 0 where the codec has no palette; bottom_up is 1 where packet row i is picture row h - 1 - i */
typedef struct mi_rgb_layout {
  int64_t packet_bytes, picture_bytes;
  int32_t packet_stride, bytes_per_pixel, palette_entries, bottom_up;
} mi_rgb_layout;

typedef struct mi_rgb_ctx mi_rgb_ctx;

int mi_rgb_device_count(void);                  /* gfx950 devices usable by this process */
mi_rgb_ctx *mi_rgb_create(int device);          /* -1: the process's current device; NULL on failure (mi_rgb_last_error(NULL)) */
void mi_rgb_destroy(mi_rgb_ctx *c);
const char *mi_rgb_last_error(const mi_rgb_ctx *c);

/* device memory of the instance's device (plain device pointers; 256-byte aligned) */
void *mi_rgb_dev_alloc(mi_rgb_ctx *c, size_t bytes);
void mi_rgb_dev_free(mi_rgb_ctx *c, void *d);
int mi_rgb_h2d(mi_rgb_ctx *c, void *d, const void *h, size_t n); /* synchronous */
int mi_rgb_d2h(mi_rgb_ctx *c, void *h, const void *d, size_t n); /* synchronous */
int mi_rgb_sync(mi_rgb_ctx *c);

/* The codec of a stream: its fourcc (BGAV_MK_FOURCC: the first character in bits 24..31), its depth, and whether it has a
 * palette.  -1 for anything upstream's init refuses.  Host only.
 *   'raw ': 1, 2, 4, 8 with a palette -> QT1, QT2, QT4, QT8 (-1 without; depth 4: see above); 34, 36, 40 -> QT2, QT4, QT8
 *           (upstream's init does not look at the palette there, its decode reads it); 16, 24, 32 -> QT16, QT24, QT32.
 *   'RGB ', 'RGB3': 8 -> AVI8 with a palette, AVI8_GRAY without; 16, 24, 32 -> AVI16, AVI24, AVI32.
 *   'MTV ': as 'RGB ' except 16 -> MTV16.
 *   AVI depths 1 and 4 are `#if 0` upstream (A:34-48, :213-228): -1. */
int mi_rgb_codec_of(uint32_t fourcc, int depth, int has_palette);
/* The layout of a codec at a size.  Host only.  MI_RGB_ERR_ARG, with a message that names the rule
 * (mi_rgb_last_error(NULL)), for an unknown codec, a size the table above does not list, and a packet or picture of 2^31
 * bytes or more. */
int mi_rgb_layout_of(int codec, int w, int h, mi_rgb_layout *out);

/* The hot path: packet i at d_packets + i * packet_stride -> picture i at d_pics + i * pic_stride, i < n, in one launch
 * queued on the instance's stream (pair with mi_rgb_sync).  Both bases and both strides are 16-byte aligned; each stride
 * is at least the layout's size; n is 1..65535; the buffers do not overlap.  Bytes of a picture slot past the picture, and
 * everything outside the slots, are not written; no packet is written.
 * Palettised codecs take n_palettes (1..n) palettes in host memory, palette k at palettes + k * palette_entries, and
 * palette_of: n indices, packet i uses palette palette_of[i] (the palette change in mid-stream of A:166-179), or NULL:
 * every packet uses palette 0.  The call has its own copy of both when it returns: the caller may overwrite its arrays
 * at once, and may queue another call with other palettes without a sync in between.  The other codecs take palettes
 * NULL, n_palettes 0 and palette_of NULL.
 * MI_RGB_ERR_ARG, with nothing launched and nothing written, for anything else: an index at or above n_palettes, a
 * missing palette, a palette given to a codec that has none. */
int mi_rgb_unpack_batch(mi_rgb_ctx *c, int codec, int w, int h, const void *d_packets, size_t packet_stride, int n,
                        void *d_pics, size_t pic_stride, const mi_rgb_color *palettes, int n_palettes,
                        const uint16_t *palette_of);
/* One packet from host memory into the caller's plane, top row first, at the caller's stride (in bytes, at least a row).
 * Synchronous.  palette: the codec's palette_entries entries, NULL for a codec without.  A packet of length 0 is skipped
 * as upstream skips it (A:160-161): MI_RGB_OK with nothing written.  MI_RGB_ERR_FORMAT for a packet shorter than the
 * layout's (upstream would read past it); a longer one is taken (AVI chunks carry padding: it is ignored). */
int mi_rgb_unpack_frame(mi_rgb_ctx *c, int codec, int w, int h, const uint8_t *packet, size_t len,
                        const mi_rgb_color *palette, uint8_t *plane, int stride);
/* Device time of the unpack kernels: every launch is bracketed with HIP events on the instance's stream; this sums them
 * over the launches since the last call (synchronises, then forgets them).  Where nobody asks, the newest 4096 launches
 * are kept and older ones forgotten. */
int mi_rgb_times(mi_rgb_ctx *c, float *total_ms, int *launches);

#ifdef __cplusplus
}
#endif
#endif
