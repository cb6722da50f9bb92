/*
 * mi_pcm.h — C ABI of the MI355X (gfx950) decoder of the PCM family: what lib/audio_pcm.c decodes with arithmetic of its
 * own, twenty fourccs and WAV ids behind twenty-two functions, seventeen transforms.  n packets resident in device memory
 * -> their interleaved samples, one call, nothing read on the host.  Plain C types only; libmi_pcm.so.
 *
 * PINNED BY STATEMENT, PLUS RECORDED VECTORS, NOT BY BUILD: every rule is in upstream's file and is cited below; the
 * checker is tests/pcmraw.py, which restates the cited lines loop for loop, the chunk loop included, and the kernel
 * reproduces it byte for byte.  tests/golden/pcm_vectors.json holds results recorded from upstream's own functions, driven
 * as decode_frame_pcm drives them; the statement is held to them.  Nothing here is held to a build of that file.
 *
 * P is lib/audio_pcm.c.
 *
 * A PACKET (P:787-808): get_packet takes len bytes, or duration * block_align where duration > 0 and that is less:
 * mi_pcm_payload_of.  decode_frame_pcm (P:1238-1261) calls the codec's function once per frame of at most FRAME_SAMPLES =
 * 1024 sample frames (P:32) until bytes_in_packet is 0.  Every function computes num_samples from the bytes left, capped
 * at 1024, consumes num_bytes and sets valid_samples = num_samples.  "ch" is num_channels, F the packet's sample frames
 * over all chunks; the output is interleaved, F * ch samples, in native (little-endian) byte order.
 *
 * THE TRANSFORMS (input bytes -> output type of a sample; s is a group's first byte):
 *   COPY8        P:51-69     1 -> 1 byte   copy (U8 and S8 differ only in the label)
 *   COPY16       P:71-91     2 -> int16    copy
 *   SWAP16       P:93-124    2 -> int16    bswap_16
 *   S24LE        P:126-159   3 -> int32    s[0]<<8 | s[1]<<16 | s[2]<<24
 *   S24BE        P:161-193   3 -> int32    s[2]<<8 | s[1]<<16 | s[0]<<24
 *   LPCM24       P:195-227   12 -> 4 int32 sample k: s[2k]<<24 | s[2k+1]<<16 | s[8+k]<<8
 *   LPCM24_MONO  P:229-259   6 -> 2 int32  sample k: s[2k]<<24 | s[2k+1]<<16 | s[4+k]<<8
 *   LPCM20       P:261-294   10 -> 4 int32 s[2k]<<24 | s[2k+1]<<16 | the nibbles of s[8], s[9]: (x&0xf0)<<8, (x&0x0f)<<12
 *   LPCM20_MONO  P:296-326   5 -> 2 int32  the same with s[4]
 *   COPY32       P:329-347   4 -> int32    copy
 *   SWAP32       P:351-383   4 -> int32    bswap_32
 *   F32LE, F32BE P:399-454, 524-584   4 -> float    float32_le_read, float32_be_read
 *   F64LE, F64BE P:456-520, 586-646   8 -> double   double64_le_read, double64_be_read
 *   ULAW         P:650-715   1 -> int16    ulaw_decode[b]
 *   ALAW         P:721-785   1 -> int16    alaw_decode[b]
 * The two tables are G.711's; the library computes all 512 entries at compile time from the closed forms
 * (csrc/pcm_format.h) and holds no copy of them.
 *
 * FRAMES: the plain codecs give F = floor(len / (bytes a sample * ch)) and write every sample.  LPCM24 and LPCM24_MONO give
 * F = floor(len / 3ch) (P:203, 237); LPCM20 and LPCM20_MONO give F = floor(2 len / 5ch) and consume floor(5 F ch / 2) bytes
 * (P:270-275, 304-309).  Their loops run over whole groups only: (num_samples * ch) / 4 turns (P:213, 280), num_samples / 2
 * in the mono forms (P:247, 314).  A full chunk of 1024 frames is a whole number of groups and of group bytes, so the
 * chunks show only in the last one, where upstream reports F * ch samples and writes 4 floor(F ch / 4) of them (mono:
 * 2 floor(F / 2)).  The mono forms are chosen for one channel only (P:969, 976) and take one channel only here.
 *
 * THE FLOAT READERS are libsndfile's portable ones and are no byte swaps.  Both signs of zero read as +0.0 (P:408-409,
 * 469-470).  A float with exponent field 0 and mantissa m != 0 reads as +-(1 + m / 2^23), bits sign | 0x3F800000 | m
 * (`exponent ? exponent - 127 : 0`, P:412, with the hidden bit of P:411).  Where 1 << exponent and 1 << abs(exponent)
 * (P:419-422, 481-484) are defined, |e| <= 30, exponent fields 97..157 of a float and 993..1053 of a double, every step is
 * exact and the result is the IEEE value bit for bit.  Everywhere else the shift is undefined behaviour: every double
 * with exponent field 0 but zero (the double readers have no arm for it), infinities, NaNs, everything below 2^-30.
 *
 * DEPARTURE 1, THE TAIL: bytes behind the last whole sample frame are dropped.  Upstream never consumes them (P:57-67 and
 * alike: num_samples is 0, so is num_bytes) and returns frames of 0 samples for ever (P:1255).
 * DEPARTURE 2, THE LPCM GROUP TAIL: the samples of a last chunk that upstream reports (P:226, 258, 293, 325) but its loop
 * does not write (P:213, 247, 280, 314) are whatever its frame buffer held; here they are written as zeros, so every byte
 * of a result is written.
 * DEPARTURE 3, OUTSIDE THE FLOAT DOMAIN: a float or double for which P:419-422 or P:481-484 is undefined is written as its
 * IEEE value, the plain reordering of its bytes, and is counted for its packet.  Inside the domain the three rules above
 * hold bit for bit.
 */
#ifndef MI_PCM_H
#define MI_PCM_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { MI_PCM_OK = 0, MI_PCM_ERR_ARG = -1, MI_PCM_ERR_HIP = -2, MI_PCM_ERR_NOMEM = -3 };
enum {
  MI_PCM_COPY8 = 0, MI_PCM_COPY16, MI_PCM_SWAP16, MI_PCM_S24LE, MI_PCM_S24BE, MI_PCM_LPCM24, MI_PCM_LPCM24_MONO, MI_PCM_LPCM20,
  MI_PCM_LPCM20_MONO, MI_PCM_COPY32, MI_PCM_SWAP32, MI_PCM_F32LE, MI_PCM_F32BE, MI_PCM_F64LE, MI_PCM_F64BE, MI_PCM_ULAW,
  MI_PCM_ALAW, MI_PCM_CODECS
};
/* upstream's sample_format (GAVL_SAMPLE_*), as a label of this library */
enum { MI_PCM_U8 = 0, MI_PCM_S8, MI_PCM_U16, MI_PCM_S16, MI_PCM_S32, MI_PCM_FLOAT, MI_PCM_DOUBLE };
enum { MI_PCM_FRAME_SAMPLES = 1024, MI_PCM_MAX_PACKETS = 1 << 20, MI_PCM_MAX_CHANNELS = 128 };
/* a tile: the output bytes one workgroup of the kernel makes */
enum { MI_PCM_TILE_BYTES = 16384 };
enum { MI_PCM_ENDIANESS_NONE = 0, MI_PCM_ENDIANESS_BIG = 1, MI_PCM_ENDIANESS_LITTLE = 2 }; /* BGAV_ENDIANESS_* */

typedef struct mi_pcm_ctx mi_pcm_ctx;
typedef struct {
  int32_t codec;        /* MI_PCM_COPY8 .. */
  int32_t label;        /* MI_PCM_U8 .. */
  int32_t block_align;  /* what an arm sets, else ch * ((bits + 7) / 8) (P:1231-1233): 3 ch for 20-bit LPCM */
  int32_t sample_bytes; /* of an output sample */
} mi_pcm_format;
typedef struct {
  uint64_t frames;    /* F */
  uint64_t written;   /* the samples upstream's loops write; F * ch but for an LPCM group tail */
  uint64_t consumed;  /* the bytes upstream consumes */
  uint64_t out_bytes; /* F * ch * sample_bytes: what this library writes */
} mi_pcm_layout;

int mi_pcm_device_count(void);                  /* gfx950 devices usable by this process */
mi_pcm_ctx *mi_pcm_create(int device);          /* -1: the process's current device; NULL on failure (mi_pcm_last_error(NULL)) */
void mi_pcm_destroy(mi_pcm_ctx *c);
const char *mi_pcm_last_error(const mi_pcm_ctx *c);

/* device memory of the instance's device (plain device pointers; 256-byte aligned) */
void *mi_pcm_dev_alloc(mi_pcm_ctx *c, size_t bytes);
void mi_pcm_dev_free(mi_pcm_ctx *c, void *d);
int mi_pcm_h2d(mi_pcm_ctx *c, void *d, const void *h, size_t n); /* synchronous */
int mi_pcm_d2h(mi_pcm_ctx *c, void *h, const void *d, size_t n); /* synchronous */
int mi_pcm_sync(mi_pcm_ctx *c);

/* init_pcm (P:810-1236) arm by arm: which function runs for a stream.  fourcc is BGAV_MK_FOURCC's (the first character in
 * the top byte; a WAV id is its own value), bits is bits_per_sample, endianess is BGAV_ENDIANESS_*, header the codec header
 * of 'lpcm' (formatSpecificFlags in native byte order, P:1107; NULL and 0 elsewhere).  Returns 0 and fills *out, or -1
 * wherever upstream returns 0 (P:857-863, 941-945, 981-985, 1046-1047, 1100-1106, 1218-1221) AND wherever upstream goes on
 * with a NULL decode_func, which it would call: WAV id 0x01 and 'PCM ' above 32 bits (P:866-904 has no else), and the
 * depths the switches of 'lpcm' do not list (P:1120-1153, 1157-1215).  Added here: -1 for channels outside
 * 1..MI_PCM_MAX_CHANNELS and for a NULL out.  Host only. */
int mi_pcm_codec_of(uint32_t fourcc, int bits, int channels, int endianess, const uint8_t *header, int header_len, mi_pcm_format *out);
/* get_packet's clamp (P:800-804): duration * block_align where duration > 0 and that is less than len, else len.  Host only. */
int64_t mi_pcm_payload_of(int64_t len, int64_t duration, int block_align);
/* What the chunk loop makes of len bytes, in closed form (tests/test_pcmraw_cpu.py holds it to the loop).  -1 for a codec
 * or a channel count that mi_pcm_decode_batch refuses, or a NULL out.  Host only. */
int mi_pcm_layout_of(int codec, int channels, uint64_t len, mi_pcm_layout *out);

/* The hot path: packet i is lens[i] bytes at d_packets + offsets[i], at any byte address; its F * ch samples go to
 * d_samples + sample_offsets[i], mi_pcm_layout_of's out_bytes.  One codec and one channel count a call; channels is
 * 1..MI_PCM_MAX_CHANNELS, and 1 for the two mono codecs.  offsets, lens and sample_offsets are in host memory; the call has
 * its own copy of what it needs when it returns.  d_samples and every sample_offsets[i] are 16-byte aligned; n is
 * 1..MI_PCM_MAX_PACKETS; lens[i] is below 2^31; the call's tiles (ceil(out_bytes / MI_PCM_TILE_BYTES) a packet) are
 * below 2^31 in all.  A length of 0, or one under a sample frame, writes nothing for that packet.  The ranges the call
 * names must not overlap one another.
 * d_outside: NULL, or n counts, 4-byte aligned: the samples of packet i outside the float domain (departure 3); written
 * as 0 for the other codecs.
 * LAUNCHES, queued on the instance's stream (pair with mi_pcm_sync): one of k_pcm_decode where any packet has a sample,
 * and before it one of k_pcm_zero where d_outside is given: 0, 1 or 2 a call.
 * No packet byte is read on the host and no packet is written; on the device only 16-byte words that hold a byte of a
 * packet are read.  Nothing but the samples and the counts is written.  MI_PCM_ERR_ARG, with nothing launched and nothing
 * written, for anything else. */
int mi_pcm_decode_batch(mi_pcm_ctx *c, int codec, int channels, const void *d_packets, const uint64_t *offsets, const uint32_t *lens,
                        int n, void *d_samples, const uint64_t *sample_offsets, uint32_t *d_outside);
/* One packet of len bytes (below 2^31) from host memory, through staging buffers the instance owns.  Synchronous.  samples
 * takes mi_pcm_layout_of's out_bytes; outside: NULL or where the count goes. */
int mi_pcm_decode_packet(mi_pcm_ctx *c, int codec, int channels, const uint8_t *bytes, size_t len, void *samples, uint32_t *outside);
/* Device time of the launches: every one is bracketed with HIP events on the instance's stream; this sums them over the
 * launches since the last call (synchronises, then forgets them) and counts them.  Where nobody asks, the newest 4096
 * launches are kept. */
int mi_pcm_times(mi_pcm_ctx *c, float *ms, int *launches);

#ifdef __cplusplus
}
#endif
#endif
