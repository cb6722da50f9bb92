/*
 * mi_tga.h — C ABI of the MI355X (gfx950) decoder of Targa packets, fourcc 'tga ': what lib/video_tga.c decodes over
 * lib/targa.c, run-length packets included, n packets resident in device memory -> n tightly packed pictures, headers
 * parsed on the device.  Plain C types only; libmi_tga.so.
 *
 * PINNED BY STATEMENT, PLUS A FEW RECORDED VECTORS, NOT BY BUILD: every rule is in the two upstream files and is cited
 * below; the checker is tests/tgaraw.py, which restates the cited lines twice (loop for loop, and vectorised), and the
 * kernels reproduce it byte for byte.  tests/golden/tga_vectors.json holds seven results recorded from upstream's own
 * lib/targa.c; the statement is held to them.  Nothing here is held to a build of the two files.
 *
 * video_tga.c is V, targa.c is T.
 *
 * HEADER (T:239-329): 18 bytes: id length, colour-map type, image type, map origin and map length (LE16), map depth,
 * x origin, y origin, width, height (LE16), pixel depth, descriptor; then the id bytes, the colour map, the image data.
 * The checks, in upstream's order (the order decides which code a packet that is bad in two ways gets):
 *   T:239-243  the map type is 0 or 1                                             else CMAP_TYPE
 *   T:245-255  the image type is not 0 (NO_IMG), and is one of 1, 2, 3, 9, 10, 11 else IMG_TYPE
 *   T:267-287  a mapped type (1, 9) with map type 0: with map length != 0 the map is read all the same ("OOPs"); with
 *              length 0 and no palette of the caller's CMAP_MISSING; otherwise the caller's palette becomes the map:
 *              origin 0, length = its entries, depth 32
 *   T:289-296  a mapped type has a map length != 0 (CMAP_LENGTH) and a map depth of 16, 24 or 32 (CMAP_DEPTH)
 *   T:303-304  width and height are not 0                                          else ZERO_SIZE
 *   T:306-309  the pixel depth is 8, 16, 24 or 32, and 8 for a mapped type         else PIXEL_DEPTH
 *   T:313-318  the id bytes are skipped
 *   T:320-329  a map in the packet is length * depth / 8 bytes (integer division); an unmapped type with map type 1
 *              carries a map too, skipped without a look at its depth
 *   T:197-216, :224-229  every read that finds fewer bytes than it asks for is EOF
 * IMAGE DATA is plain, width * height * depth / 8 bytes (T:345-346), or run-length (T:385-433): a header byte b gives
 * count = (b & 127) + 1; b & 128 is a run packet: one pixel is read (EOF if it is short) and repeated, RLE once a repeat
 * passes width * height; otherwise a raw packet: RLE if it would pass width * height, checked before its bytes are read
 * (then EOF if they are short).  The loop ends when the picture is full or the stream is empty; bytes after a full
 * picture are ignored.
 * COLOUR UNMAP (T:875-912): a pixel byte i becomes the bytes at map + i * bpp; i >= origin + length is INDEX_RANGE.
 * THE CALLER'S PALETTE (V:92-121): entry k is the bytes r >> 8, g >> 8, b >> 8, a >> 8.
 * OUTPUT FORMAT (V:53-77, V:170-183), by depth, of the map for a mapped type: 8 GRAY_8, 16 RGB_15 (two bytes, copied),
 * 24 BGR_24, 32 RGBA_32.
 * RED/BLUE SWAP (V:211-212, T:1172-1188): for 32-bit output bytes 0 and 2 of every stored pixel are exchanged, EXCEPT
 * THE LAST STORED PIXEL, index width * height - 1: the loop's bound is (width * height - 1) * bpp.  Defined behaviour;
 * imitated.
 * ORIENTATION (V:220-245): descriptor bit 5 set: the stored rows are the picture's rows in order, else reversed; bit 4
 * set: the columns are reversed.
 *
 * Two upstream facts that are stated here and not imitated, because upstream's result is uninitialised memory there:
 *   - a run-length stream that ends exactly at a packet boundary before the picture is full returns TGA_NOERR with the
 *     rest of malloc's buffer (T:398): MI_TGA_ST_SHORT here;
 *   - a map index below the map's origin reads map bytes nobody wrote (T:322-328): MI_TGA_ST_BELOW_ORIGIN here.
 */
#ifndef MI_TGA_H
#define MI_TGA_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { MI_TGA_OK = 0, MI_TGA_ERR_ARG = -1, MI_TGA_ERR_HIP = -2, MI_TGA_ERR_NOMEM = -3, MI_TGA_ERR_FORMAT = -4 };
/* the output formats, by depth / 8 - 1 */
enum { MI_TGA_GRAY8 = 0, MI_TGA_RGB15 = 1, MI_TGA_BGR24 = 2, MI_TGA_RGBA32 = 3, MI_TGA_FORMATS = 4 };
/* the status of a packet: 0, upstream's tga_result where upstream returns one, or one of this library's own */
enum {
  MI_TGA_ST_OK = 0, MI_TGA_ST_EOF = 2, MI_TGA_ST_CMAP_TYPE = 4, MI_TGA_ST_IMG_TYPE = 5, MI_TGA_ST_NO_IMG = 6,
  MI_TGA_ST_CMAP_MISSING = 7, MI_TGA_ST_CMAP_LENGTH = 9, MI_TGA_ST_CMAP_DEPTH = 10, MI_TGA_ST_ZERO_SIZE = 11,
  MI_TGA_ST_PIXEL_DEPTH = 12, MI_TGA_ST_RLE = 15, MI_TGA_ST_INDEX_RANGE = 16,
  MI_TGA_ST_SHORT = 32,        /* a run-length stream that ends early at a packet boundary */
  MI_TGA_ST_BELOW_ORIGIN = 33, /* a map index below the map's origin */
  MI_TGA_ST_MISMATCH = 34      /* width, height or output format differ from the call's */
};

/* a palette entry as upstream's gavl_palette_entry_t: 16 bits a component, of which the high byte is used */
typedef struct { uint16_t r, g, b, a; } mi_tga_color;

/* What the header says (csrc/tga_format.h has the one parser that fills it, on the host and in the scan kernel).  The
 * header fields are as upstream's tga_image holds them after the read: where T:267-287 changes map_type, map_origin,
 * map_length and map_depth, these are the changed values.  A field the parser did not reach before it refused the
 * packet is 0.  format and bytes_per_pixel are the output's; the stored pixel has pixel_depth / 8 bytes.  map_offset is
 * where the packet's own map begins (0 with from_palette), data_offset where the image data begins. */
typedef struct mi_tga_info {
  int32_t status;
  uint32_t data_offset, map_offset;
  uint16_t map_origin, map_length, x_origin, y_origin, width, height;
  uint8_t id_length, map_type, image_type, map_depth, pixel_depth, descriptor;
  uint8_t format, bytes_per_pixel;
  uint8_t rle, mapped, flip_x, flip_y, from_palette; /* flags, 0 or 1; flip_y: stored row i is picture row h - 1 - i */
  uint8_t reserved[3];
} mi_tga_info;

typedef struct mi_tga_ctx mi_tga_ctx;

int mi_tga_device_count(void);                  /* gfx950 devices usable by this process */
mi_tga_ctx *mi_tga_create(int device);          /* -1: the process's current device; NULL on failure (mi_tga_last_error(NULL)) */
void mi_tga_destroy(mi_tga_ctx *c);
const char *mi_tga_last_error(const mi_tga_ctx *c);

/* device memory of the instance's device (plain device pointers; 256-byte aligned) */
void *mi_tga_dev_alloc(mi_tga_ctx *c, size_t bytes);
void mi_tga_dev_free(mi_tga_ctx *c, void *d);
int mi_tga_h2d(mi_tga_ctx *c, void *d, const void *h, size_t n); /* synchronous */
int mi_tga_d2h(mi_tga_ctx *c, void *h, const void *d, size_t n); /* synchronous */
int mi_tga_sync(mi_tga_ctx *c);

/* The header of a packet of len bytes in host memory, up to where the image data begins; palette_entries is the size of
 * the caller's palette (0: none).  Returns the status, which is info->status too: 0, or the code of the first check
 * that fails in upstream's order.  The image data is not looked at.  Host only. */
int mi_tga_parse(const uint8_t *pkt, size_t len, int palette_entries, mi_tga_info *info);
/* The expansion tile T: the index has one checkpoint for every T stored pixels.  Host only. */
int mi_tga_tile_pixels(void);

/* The hot path: packet i is lengths[i] bytes at d_stream + offsets[i], at any byte address; picture i goes to
 * d_pics + i * pic_stride, tightly packed rows of w * bytes-per-pixel bytes, top row first.  offsets and lengths are in
 * host memory; the call has its own copy of them, and of the palettes, when it returns.  d_pics and pic_stride are
 * 16-byte aligned, pic_stride is at least the picture's size, which is below 2^31 bytes; n is 1..65535; w and h are
 * 1..65535; format is one of MI_TGA_GRAY8 .. MI_TGA_RGBA32.  Three launches (scan, index, expand) queued on the
 * instance's stream (pair with mi_tga_sync); the stream's bytes are never read on the host.
 * Palettes: n_palettes (1..n) palettes of palette_entries (1..65535) entries each in host memory (V:98-104 refuses a
 * change of size), palette k at palettes + k * palette_entries, and palette_of: n indices, packet i uses palette
 * palette_of[i], or NULL: every packet uses palette 0.  palettes may be NULL (with palette_entries 0, n_palettes 0 and
 * palette_of NULL): a packet that needs the caller's palette is then CMAP_MISSING.
 * d_status: n int32_t in device memory, written for every packet.  A packet whose status is not 0 leaves its picture
 * slot unwritten, except for INDEX_RANGE and BELOW_ORIGIN, which are found while expanding: the slot's picture bytes are
 * unspecified then (a picture with indices of both kinds is INDEX_RANGE, as upstream).  A packet whose width, height or
 * output format are not the call's is MISMATCH; for a plain packet that is also too short, MISMATCH is the code.
 * Nothing outside the picture bytes of the slots is written; no packet is written.
 * MI_TGA_ERR_ARG, with nothing launched and nothing written, for anything else. */
int mi_tga_decode_batch(mi_tga_ctx *c, const void *d_stream, const uint64_t *offsets, const uint32_t *lengths, int n, int w,
                        int h, int format, void *d_pics, size_t pic_stride, const mi_tga_color *palettes,
                        int palette_entries, int n_palettes, const uint16_t *palette_of, int32_t *d_status);
/* One packet from host memory into the caller's plane, top row first, at the caller's stride (in bytes, at least a row of
 * the packet's own width and format, which info returns).  Synchronous.  palette: palette_entries entries, or NULL and 0.
 * MI_TGA_ERR_FORMAT with info->status set for a bad packet; the plane is not written then. */
int mi_tga_decode_frame(mi_tga_ctx *c, const uint8_t *pkt, size_t len, const mi_tga_color *palette, int palette_entries,
                        uint8_t *plane, int stride, mi_tga_info *info);
/* Device time of the three kernels, ms[0] scan, ms[1] index, ms[2] expand: every launch is bracketed with HIP events on
 * the instance's stream; this sums them over the launches since the last call (synchronises, then forgets them) and
 * counts the launches, three a call.  Where nobody asks, the newest 4096 launches of each kind are kept. */
int mi_tga_times(mi_tga_ctx *c, float *ms, int *launches);

#ifdef __cplusplus
}
#endif
#endif
