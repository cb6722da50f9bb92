/*
 * mi_yuv.h — C ABI of the MI355X (gfx950) unpacker of the uncompressed QuickTime YUV family: the eleven fourccs of
 * lib/video_yuv.c (SURVEY.md layer L2), n packets resident in device memory -> n tightly packed pictures in one launch.
 * Plain C types only; libmi_yuv.so.
 *
 * PINNED BY STATEMENT: every line of the arithmetic is in lib/video_yuv.c and is cited below; the checker is
 * tests/yuvraw.py, a numpy restatement of the cited lines, which tests/test_yuv_reference_cpu.py holds to the file itself
 * (built as it stands into oracle/_ref/libvideo_yuv_ref.so where the reference tree is present), and the kernels
 * reproduce it byte for byte.
 *
 * PAD(x, a) rounds x up to a multiple of a (lib/video_yuv.c:32); words are little-endian (GAVL_PTR_2_32LE).  A PICTURE is
 * tightly packed: its planes back to back in the order below, each plane's rows at the plane's own width; 16-bit samples
 * are native uint16_t.  A size is accepted where the upstream loops cover the whole picture and nothing beyond it.
 *
 *   codec  lines     sizes              packet                                  picture
 *   yuv2   :55-100   w even             rows of 2w: Y0 U Y1 V                   Y w x h, U w/2 x h, V w/2 x h; U, V ^ 0x80
 *   2vuy   :191-214  w even             rows of 2w                              the same 2w x h bytes (UYVY)
 *   VYUY   :221-244  w even             rows of 2w                              the same 2w x h bytes (YUY2)
 *   yv12   :248-278  w, h even          Y w x h, U, V w/2 x h/2                 the same planes, same order
 *   YV12   :280-309  w, h even          Y, then V, then U                       Y, U, V
 *   YVU9   :315-344  w, h % 4 == 0      s = PAD(w, 8): Y at stride s, then V,   Y w x h, U w/4 x h/4, V w/4 x h/4
 *                                       then U at stride s/4, h/4 rows
 *   v308   :349-396  any                rows of 3w: V Y U                       Y, U, V each w x h
 *   v408   :104-182  any                rows of 4w: U Y V A                     packed, 4 bytes a pixel: Y U V alpha(A)
 *   v410   :403-450  any                rows of 4w, one word a pixel            Y, U, V each w x h uint16: U = bits 2..11,
 *                                                                               Y = bits 12..21, V = bits 22..31, each << 6
 *   v210   :457-540  w even             rows at stride PAD(w, 48) * 8 / 3       Y w x h, U w/2 x h, V w/2 x h uint16
 *   yuv4   :549-602  w, h even          h/2 rows of 3w: U V Y00 Y01 Y10 Y11     Y w x h, U, V w/2 x h/2; U, V ^ 0x80
 *
 * v210: four words code six pixels; field k (bits 10k .. 10k + 9) of word j is one sample, written << 6, in the order
 * Cb0 Y0 Cr0 | Y1 Cb1 Y2 | Cr1 Y3 Cb2 | Y4 Cr2 Y5; bits 30..31 are dropped.  The last w % 6 pixels of a row (2 or 4) come
 * from one more group, of which only the first 2 or 4 pixels and their chroma are written (:501-521).
 * v408: alpha(x) = 0 for x < 2, else min(255, ((x - 2) * 255 + 43) / 219) in integers: all 256 entries of the table at
 * :104-138.
 * '2vuy' is the UYVY decoder's: upstream registers it first (:779-781), the VYUY decoder's second fourcc never wins.
 */
#ifndef MI_YUV_H
#define MI_YUV_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { MI_YUV_OK = 0, MI_YUV_ERR_ARG = -1, MI_YUV_ERR_HIP = -2, MI_YUV_ERR_NOMEM = -3, MI_YUV_ERR_FORMAT = -4 };
/* the codecs, in upstream's order of registration */
enum {
  MI_YUV_YUV2 = 0, MI_YUV_2VUY = 1, MI_YUV_YV12_LOWER = 2 /* 'yv12' */, MI_YUV_YV12_UPPER = 3 /* 'YV12' */, MI_YUV_VYUY = 4,
  MI_YUV_YVU9 = 5, MI_YUV_V308 = 6, MI_YUV_V408 = 7, MI_YUV_V410 = 8, MI_YUV_V210 = 9, MI_YUV_YUV4 = 10, MI_YUV_CODECS = 11
};

/* what a codec makes of a size: the packet (its planes, or its one packed plane, at row strides in bytes; 0 for planes the
 * packet does not have), and the picture's planes in picture order: width in samples, height, bytes per sample (packed
 * pictures have one plane: 2vuy and VYUY 2 bytes a sample, v408 4) */
typedef struct mi_yuv_layout {
  int64_t packet_bytes, picture_bytes;
  int32_t packet_strides[3];
  int32_t planes;
  int32_t plane_w[3], plane_h[3], plane_bps[3];
} mi_yuv_layout;

typedef struct mi_yuv_ctx mi_yuv_ctx;

int mi_yuv_device_count(void);                  /* gfx950 devices usable by this process */
mi_yuv_ctx *mi_yuv_create(int device);          /* -1: the process's current device; NULL on failure (mi_yuv_last_error(NULL)) */
void mi_yuv_destroy(mi_yuv_ctx *c);
const char *mi_yuv_last_error(const mi_yuv_ctx *c);

/* device memory of the instance's device (plain device pointers; 256-byte aligned) */
void *mi_yuv_dev_alloc(mi_yuv_ctx *c, size_t bytes);
void mi_yuv_dev_free(mi_yuv_ctx *c, void *d);
int mi_yuv_h2d(mi_yuv_ctx *c, void *d, const void *h, size_t n); /* synchronous */
int mi_yuv_d2h(mi_yuv_ctx *c, void *h, const void *d, size_t n); /* synchronous */
int mi_yuv_sync(mi_yuv_ctx *c);

/* The codec of a fourcc (BGAV_MK_FOURCC: the first character in bits 24..31), -1 for any other.  Host only. */
int mi_yuv_codec_of(uint32_t fourcc);
/* The layout of a codec at a size.  Host only.  MI_YUV_ERR_ARG, with a message that names the rule
 * (mi_yuv_last_error(NULL)), for an unknown codec, a size the table above does not list, and a packet or picture of 2^31
 * bytes or more. */
int mi_yuv_layout_of(int codec, int w, int h, mi_yuv_layout *layout);
/* alpha(x) of v408 for x = 0..255, by the closed form above.  Host only. */
int mi_yuv_alpha_v408(uint8_t out[256]);

/* The hot path: packet i at d_packets + i * packet_stride -> picture i at d_pics + i * pic_stride, i < n, in one launch
 * queued on the instance's stream (pair with mi_yuv_sync).  Both bases and both strides are 16-byte aligned; each stride
 * is at least the layout's size; n is 1..65535; the buffers do not overlap.  Bytes of a picture slot past the picture, and
 * everything outside the slots, are not written.  MI_YUV_ERR_ARG, with nothing launched, for anything else. */
int mi_yuv_unpack_batch(mi_yuv_ctx *c, int codec, int w, int h, const void *d_packets, size_t packet_stride, int n,
                        void *d_pics, size_t pic_stride);
/* One packet from host memory into the caller's planes (the layout's, in picture order; the others are not read) at the
 * caller's strides (in bytes, at least a plane row).  Synchronous.  A packet of length 0 is skipped as upstream skips it
 * (:623-624): MI_YUV_OK with nothing written.  MI_YUV_ERR_FORMAT for a packet shorter than the layout's (upstream would
 * read past it). */
int mi_yuv_unpack_frame(mi_yuv_ctx *c, int codec, int w, int h, const uint8_t *packet, size_t len, uint8_t *const planes[3],
                        const int strides[3]);
/* Device time of the unpack kernels: every launch is bracketed with HIP events on the instance's stream; this sums them
 * over the launches since the last call (synchronises, then forgets them).  Where nobody asks, the newest 4096 launches
 * are kept and older ones forgotten. */
int mi_yuv_times(mi_yuv_ctx *c, float *total_ms, int *launches);

#ifdef __cplusplus
}
#endif
#endif
