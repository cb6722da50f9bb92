/*
 * mi_spu.h — C ABI of the MI355X (gfx950) decoder of DVD subpictures, fourcc 'DVDS': what lib/subovl_dvd.c decodes, n
 * packets resident in device memory -> n full-frame YUVA overlays of the video's size, control sections parsed on the
 * device.  Plain C types only; libmi_spu.so.
 *
 * PINNED BY STATEMENT, PLUS A FEW RECORDED VECTORS, NOT BY BUILD: every rule is in the one upstream file and is cited
 * below; the checker is tests/spuraw.py, which restates the cited lines loop for loop, and the kernels reproduce it byte
 * for byte.  tests/golden/spu_vectors.json holds results recorded from upstream's own lib/subovl_dvd.c; the statement is
 * held to them.  Nothing here is held to a build of that file.
 *
 * subovl_dvd.c is S.
 *
 * OVERLAY (S:66, S:182): a frame of the VIDEO's size W x H, GAVL_YUVA_32: four bytes a pixel, rows of W * 4 bytes.  It is
 * filled with 0 (transparent) first; the subpicture is drawn at the frame's origin, not at x1, y1 (S:311-316 return the
 * rectangle beside the picture).
 * CONTROL SECTION (S:186-256): starts at BE16(pkt + 2), which is ctrl_start.  A sequence is 2 bytes of date (not read),
 * 2 bytes next_ctrl_offset, then commands of one byte:
 *   00, 01, 02  no operands, no effect
 *   03          2 bytes: palette[3], palette[2], palette[1], palette[0], a nibble each
 *   04          2 bytes: alpha[3], alpha[2], alpha[1], alpha[0], a nibble each
 *   05, 85      6 bytes: x1, x2, y1, y2 of 12 bits each
 *   06          4 bytes: offset1, offset2, BE16
 *   ff          ends the sequence
 *   any other   no operands, skipped (S:245-249): the operands of a 07 are read as commands.  Imitated.
 * The loop ends after the sequence whose next_ctrl_offset equals the one before it (the first: ctrl_start).  The read
 * pointer is NOT set from next_ctrl_offset (S:253-255): the next sequence is read from where the last one ended.  Values
 * accumulate over the sequences; the last one wins.  Imitated.
 * LOCAL PALETTE (S:260-266, the little-endian arm): colour c is the four bytes (e >> 16) & 255, (e >> 8) & 255, e & 255,
 * alpha[c] * 17 with e = ifo_palette[palette[c]]; the top byte of e is shifted out.
 * SCANLINE (S:77-130): nibbles, the high one of a byte first.  A code v is 1 nibble if v >= 4, 2 nibbles if v >= 0x10,
 * 3 nibbles if v >= 0x40, else 4 nibbles; a 4-nibble v < 4 fills to the end of the line.  len = v >> 2, colour = v & 3;
 * x + len > width is clamped (S:114-118; the fprintf is not imitated).  The line ends when x >= width; the next line
 * starts at the next whole byte.
 * FIELD (S:132-147, S:294-304): field 1 is at offset1 with length offset2 - offset1 and goes to rows 0, 2, 4, ...; field
 * 2 is at offset2 with length ctrl_start - offset2 and goes to rows 1, 3, 5, ....  width = x2 - x1 + 1.  Lines are
 * decoded while pos < length and fewer than H / 2 lines are done: the count of lines comes from the data, not from
 * y2 - y1 + 1.  pos < length is tested at a line's start only: a last line may read past its field into whatever
 * follows.  A negative length decodes nothing.  Without a 06 command both offsets are 0 and field 2 decodes the packet's
 * own head.  All of this is defined and imitated.  (With H = 1, H / 2 is 0 and no line is decoded here; upstream's loop
 * tests the count after its first line, whose row for field 2 would lie outside the frame.)
 * BESIDE THE PICTURE (S:311-323): src_w = x2 - x1 + 1, src_h = y2 - y1 + 1, dst_x = x1, dst_y = y1; dst_x + src_w > W
 * makes dst_x = W - src_w, dst_y + src_h > H makes dst_y = H - src_h.  Either may go negative.
 *
 * Upstream returns no error at all.  Where its result is undefined the packet is refused here, with this library's own
 * statuses, in this order (the order decides which code a packet that is bad in several ways gets):
 *   SHORT       the packet is under 4 bytes
 *   CTRL_RANGE  the control walk needs a byte at or past the packet's length (every sequence eats at least 5 bytes, so
 *               the walk always ends)
 *   RECT        width < 1 or width > W: upstream writes nothing, or writes across rows
 *   DATA_RANGE  a scanline needs a nibble whose byte is at or past the packet's length; field 1 comes before field 2
 */
#ifndef MI_SPU_H
#define MI_SPU_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { MI_SPU_OK = 0, MI_SPU_ERR_ARG = -1, MI_SPU_ERR_HIP = -2, MI_SPU_ERR_NOMEM = -3, MI_SPU_ERR_FORMAT = -4 };
/* the status of a packet: this library's own, upstream has none */
enum { MI_SPU_ST_OK = 0, MI_SPU_ST_SHORT = 1, MI_SPU_ST_CTRL_RANGE = 2, MI_SPU_ST_RECT = 3, MI_SPU_ST_DATA_RANGE = 4 };

/* What a packet's control section says and what the decoder made of it (csrc/spu_format.h has the one parser that fills
 * it, on the host and in the scan kernel).  The first seven words are what upstream returns beside the picture, and the
 * lines each field decoded, which only the decoder knows: mi_spu_parse leaves them 0.  In the place of a reserved eighth
 * word ride the raw control values, which widens the struct from 32 to 56 bytes: ctrl_start, the offsets, the rectangle,
 * the number of sequences read, the palette and alpha nibbles (index 0 first), and ctrl_end, the offset of the byte after
 * the last one the walk read.  A command the walk could not read whole changes nothing; with SHORT every field is 0,
 * with CTRL_RANGE the raw values are those gathered so far and src_w .. dst_y are 0.  With DATA_RANGE the two line counts
 * are unspecified. */
typedef struct mi_spu_info {
  int32_t status;
  int32_t src_w, src_h, dst_x, dst_y;
  int32_t lines1, lines2;
  uint16_t ctrl_start, offset1, offset2, x1, x2, y1, y2, sequences;
  uint8_t palette[4], alpha[4];
  uint32_t ctrl_end;
} mi_spu_info;

typedef struct mi_spu_ctx mi_spu_ctx;

int mi_spu_device_count(void);                  /* gfx950 devices usable by this process */
mi_spu_ctx *mi_spu_create(int device);          /* -1: the process's current device; NULL on failure (mi_spu_last_error(NULL)) */
void mi_spu_destroy(mi_spu_ctx *c);
const char *mi_spu_last_error(const mi_spu_ctx *c);

/* device memory of the instance's device (plain device pointers; 256-byte aligned) */
void *mi_spu_dev_alloc(mi_spu_ctx *c, size_t bytes);
void mi_spu_dev_free(mi_spu_ctx *c, void *d);
int mi_spu_h2d(mi_spu_ctx *c, void *d, const void *h, size_t n); /* synchronous */
int mi_spu_d2h(mi_spu_ctx *c, void *h, const void *d, size_t n); /* synchronous */
int mi_spu_sync(mi_spu_ctx *c);

/* The control walk and the rectangle of a packet of len bytes in host memory, for a video of w x h (1..4096 each).
 * Returns the status, which is info->status too: 0, SHORT, CTRL_RANGE or RECT.  The fields are not looked at.  Host
 * only. */
int mi_spu_parse(const uint8_t *pkt, size_t len, int w, int h, mi_spu_info *info);

/* The hot path: packet i is lengths[i] bytes at d_stream + offsets[i], at any byte address; picture i is w * h * 4 tight
 * bytes at d_pics + i * pic_stride.  EVERY byte of a good packet's picture is written, the zeros included: the caller
 * does not clear.  offsets and lengths are in host memory; the call has its own copy of them, of the palettes and of
 * palette_of when it returns.  d_pics and pic_stride are 16-byte aligned, pic_stride is at least w * h * 4; n is
 * 1..65535; w and h are 1..4096; a packet stays below 2^31 bytes.  Two launches (scan, decode) queued on the instance's
 * stream (pair with mi_spu_sync); the stream's bytes are never read on the host.
 * palettes: n_palettes (1..n) palettes of 16 uint32_t each in host memory (the disc's, as the IFO file holds them:
 * upstream's ifo_palette), palette k at palettes + 16 k; palette_of: n indices, packet i uses palette palette_of[i], or
 * NULL: every packet uses palette 0.
 * d_info: n structs in device memory, 4-byte aligned, written for every packet.  A packet of status SHORT, CTRL_RANGE or
 * RECT leaves its slot unwritten.  DATA_RANGE is found while decoding: the slot's picture bytes are unspecified then.
 * Nothing else is written: no byte outside the picture bytes of the slots and the infos, and no packet.
 * MI_SPU_ERR_ARG, with nothing launched and nothing written, for anything else. */
int mi_spu_decode_batch(mi_spu_ctx *c, const void *d_stream, const uint64_t *offsets, const uint32_t *lengths, int n, int w,
                        int h, void *d_pics, size_t pic_stride, const uint32_t *palettes, int n_palettes,
                        const uint16_t *palette_of, mi_spu_info *d_info);
/* One packet from host memory into the caller's plane of h rows at the caller's stride (in bytes, at least w * 4).
 * Synchronous.  palette: 16 entries.  Every row's w * 4 bytes are written; the bytes between the rows are not.
 * MI_SPU_ERR_FORMAT with info->status set for a bad packet; the plane is not written then. */
int mi_spu_decode_frame(mi_spu_ctx *c, const uint8_t *pkt, size_t len, int w, int h, const uint32_t *palette, uint8_t *plane,
                        int stride, mi_spu_info *info);
/* Device time of the two kernels, ms[0] scan, ms[1] decode: every launch is bracketed with HIP events on the instance's
 * stream; this sums them over the launches since the last call (synchronises, then forgets them) and counts the
 * launches, two a call.  Where nobody asks, the newest 4096 launches of each kind are kept. */
int mi_spu_times(mi_spu_ctx *c, float *ms, int *launches);

#ifdef __cplusplus
}
#endif
#endif
