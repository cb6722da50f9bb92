/*
 * mi_dv.h — C ABI of the MI355X (gfx950) DV video decoder (and, at the end, encoder).  Five systems.  At 25 Mbit/s: 525/60 (NTSC), 120,000-byte
 * DIF frames in, 720 x 480 4:1:1 pictures out; 625/50 (PAL) in the IEC 4:2:0 profile, 144,000-byte DIF frames in,
 * 720 x 576 4:2:0 pictures out; and 625/50 in the DVCPRO 4:1:1 profile, 144,000-byte DIF frames in, 720 x 576 4:1:1
 * pictures out.  At 50 Mbit/s ("DVCPRO50", two DIF channels): 525/60, 240,000-byte frames in, 720 x 480
 * 4:2:2 pictures out; and 625/50, 288,000-byte frames in, 720 x 576 4:2:2 pictures out.  Plain C types only; libmi_dv.so.
 *
 * Where it sits in gmerlin-avdecoder.  lib/dvframe.c:663-676 (bgav_dv_dec_get_video_packet) hands every DIF frame on
 * unchanged as a video packet; the pixels are then made by libavcodec's "dvvideo" decoder behind
 * lib/video_ffmpeg.c:556,628 (table entry :1572-1575; the fourccs 'dvc ', 'dvcp', 'dvsd', ... of lib/video.c:122-145).
 * This library replaces that step for the 525/60 25 Mbit/s profile: a decoder
 * registered for those fourccs in front of the FFmpeg one calls mi_dv_decode_frame with
 * gavl_packet_t::buf and the planes / strides of the gavl_video_frame_t (GAVL_YUV_411_P: Y, Cb, Cr).  For the 625/50
 * 4:2:0 profile (lib/dvframe.c:129-148, GAVL_YUV_420_P) it calls mi_dv_decode_frame_sys with MI_DV_SYS_625_50, for the
 * two DVCPRO50 profiles (lib/dvframe.c:170-211, GAVL_YUV_422_P) with MI_DV_SYS_525_60_422 / MI_DV_SYS_625_50_422, for
 * the DVCPRO 625/50 4:1:1 profile (lib/dvframe.c:149-169, GAVL_YUV_411_P) with MI_DV_SYS_625_50_411 — the plugin takes
 * such streams only when the process environment holds MI_DV_625_411=1.  These are all the
 * standard-definition profiles of lib/dvframe.c:106-296; the DVCPRO HD ones are not decoded here.
 *
 * PARITY UNPINNED: the reference holds no DV pixel decoder to compare with and none is reachable from the build
 * container.  The arithmetic is stated in oracle/dv_oracle.c (written from the published format, from memory); the
 * GPU path reproduces THAT bit for bit.  Pictures of a real DV stream will look right only as far as that statement
 * matches the standard's tables.  The 625/50 layout (the number of DIF sequences, the macroblock shuffle, the 4:2:0
 * block placement: DESIGN.md section 9) is written from the published format too and is just as unpinned.  The 4:2:2
 * layout (two channels back to back, areas 1 and 3 of the compressed macroblock without pixels, 16 x 8 macroblocks, the
 * super-block row 2 row + channel: DESIGN.md section 9.3) is this repository's reading of SMPTE 314M, unpinned in the
 * same way.  The 625/50 4:1:1 layout (the 625/50 frame, the 525/60 macroblocks, right-edge column and shuffle with 12
 * sequences as the modulus: DESIGN.md section 9.4) is a reading of SMPTE 314M from memory and the least certain of all,
 * unpinned in the same way.  One checker, tests/dvsys.py, states all four layouts: it moves whole video segments between
 * a system's frames and 525/60 frames around the unchanged oracle.
 */
#ifndef MI_DV_H
#define MI_DV_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { MI_DV_OK = 0, MI_DV_ERR_ARG = -1, MI_DV_ERR_HIP = -2, MI_DV_ERR_NOMEM = -3, MI_DV_ERR_FORMAT = -4 };
enum { MI_DV_FRAME_BYTES = 120000, MI_DV_WIDTH = 720, MI_DV_HEIGHT = 480, MI_DV_CHROMA_WIDTH = 180,
       MI_DV_PICTURE_BYTES = 720 * 480 * 3 / 2 };
/* the systems (the DSF bit of the DIF header), and the 625/50 geometry: Y 720 x 576, Cb 360 x 288, Cr 360 x 288 */
enum { MI_DV_SYS_525_60 = 0, MI_DV_SYS_625_50 = 1 };
/* 625/50 in the DVCPRO 4:1:1 profile (DSF 1, VAUX stype 0, APT != 0): MI_DV_625_FRAME_BYTES in, Y 720 x 576, Cb 180 x 576,
 * Cr 180 x 576 out.  (2 is no system.) */
enum { MI_DV_SYS_625_50_411 = 3 };
enum { MI_DV_625_411_CHROMA_WIDTH = 180, MI_DV_625_411_PICTURE_BYTES = 720 * 576 + 2 * 180 * 576 };
/* the 50 Mbit/s 4:2:2 systems (VAUX stype 0x4 | DSF; 2 is no system, 3 is the one above): Y 720 x 480 / 576, Cb and Cr 360
 * wide and as high as the picture */
enum { MI_DV_SYS_525_60_422 = 4, MI_DV_SYS_625_50_422 = 5 };
enum { MI_DV_525_422_FRAME_BYTES = 240000, MI_DV_525_422_PICTURE_BYTES = 720 * 480 * 2, MI_DV_625_422_FRAME_BYTES = 288000,
       MI_DV_625_422_PICTURE_BYTES = 720 * 576 * 2, MI_DV_422_CHROMA_WIDTH = 360 };
enum { MI_DV_625_FRAME_BYTES = 144000, MI_DV_625_HEIGHT = 576, MI_DV_625_CHROMA_WIDTH = 360, MI_DV_625_CHROMA_HEIGHT = 288,
       MI_DV_625_PICTURE_BYTES = 720 * 576 + 2 * 360 * 288 };

typedef struct mi_dv_ctx mi_dv_ctx;

int mi_dv_device_count(void);                 /* gfx950 devices usable by this process */
mi_dv_ctx *mi_dv_create(int device);          /* -1: the process's current device; NULL on failure (mi_dv_last_error(NULL)) */
void mi_dv_destroy(mi_dv_ctx *c);
const char *mi_dv_last_error(const mi_dv_ctx *c);

/* device memory of the instance's device (plain device pointers; 256-byte aligned) */
void *mi_dv_dev_alloc(mi_dv_ctx *c, size_t bytes);
void mi_dv_dev_free(mi_dv_ctx *c, void *d);
int mi_dv_h2d(mi_dv_ctx *c, void *d, const void *h, size_t n); /* synchronous */
int mi_dv_d2h(mi_dv_ctx *c, void *h, const void *d, size_t n); /* synchronous */
int mi_dv_sync(mi_dv_ctx *c);

/* The hot path: n DIF frames resident in device memory (back to back, MI_DV_FRAME_BYTES each, d_frames 4-byte aligned)
 * -> n pictures (back to back, MI_DV_PICTURE_BYTES each: Y 720 x 480, Cb 180 x 480, Cr 180 x 480, tightly packed;
 * d_pics 8-byte aligned).  Queued on the instance's stream; pair with mi_dv_sync.  Any 120,000 bytes decode to
 * something (damaged frames are not detected, as in the oracle; mi_dv_decode_batch_held and mi_dv_decode_frame_held
 * below read what a stream says about its own damage). */
int mi_dv_decode_batch(mi_dv_ctx *c, const void *d_frames, int n, void *d_pics);
/* Device time of k_dv_decode: every mi_dv_decode_batch brackets its launch with HIP events on the instance's stream;
 * this sums them over the launches since the last call (synchronises, then forgets them).  Where nobody asks, the newest
 * 4096 launches are kept and older ones forgotten; so do mi_dv_hold_times, mi_dv_encode_times, mi_dv_audio_times and
 * mi_dv_meta_times, each with 4096 of its own. */
int mi_dv_kernel_times(mi_dv_ctx *c, float *total_ms, int *launches);

/* One frame from host memory into the caller's planes (Y, Cb, Cr) with the caller's strides — what a
 * bgav_video_decoder_t::decode does with a packet and a gavl_video_frame_t.  Synchronous.  Checks that the frame
 * announces 525/60 (DSF bit clear, lib/dvframe.c:298-316) and returns MI_DV_ERR_FORMAT otherwise. */
int mi_dv_decode_frame(mi_dv_ctx *c, const uint8_t *frame, size_t len, uint8_t *const planes[3], const int strides[3]);

/* The decoder's constant tables exactly as its kernels read them (csrc/dv_common.h, struct Tables: the variable-length
 * code's look-up tables, reconstruction multipliers / areas / coefficient places for both transform modes, quantiser
 * shifts).  Host only — no device needed: the non-GPU tests compare them with what oracle/dv_oracle.c makes of the same
 * format data.  Returns the size in bytes; copies when `out` has room. */
size_t mi_dv_copy_tables(void *out, size_t cap);

/* ---- every system ---- */

/* The 25 Mbit/s system a DIF frame of `len` bytes belongs to, from its header (lib/dvframe.c:298-316): MI_DV_SYS_525_60
 * for DSF 0 with VAUX stype 0, MI_DV_SYS_625_50 for DSF 1 with stype 0 and APT 0; -1 for anything else (DVCPRO 625/50
 * 4:1:1, which is DSF 1 with APT != 0; DVCPRO50; the HD profiles) and for a frame shorter than its system's.  It knows
 * the two 25 Mbit/s systems it names only: mi_dv_profile_of adds the 4:2:2 ones, mi_dv_kind_of answers for all five.
 * Host only. */
int mi_dv_system_of(const uint8_t *frame, size_t len);
/* The same for every profile this library decodes: 0, 1, 4 or 5 (MI_DV_SYS_*; stype 0x4 is DVCPRO50, whose system is
 * stype | DSF); -1 for anything else and for a frame shorter than its system's.  Equal to mi_dv_system_of wherever that
 * is not -1.  Host only. */
int mi_dv_profile_of(const uint8_t *frame, size_t len);
/* The same for every profile this library decodes: 0, 1, 3, 4 or 5.  3 (MI_DV_SYS_625_50_411) is DSF 1 with stype 0, APT
 * != 0 and at least MI_DV_625_FRAME_BYTES; -1 for anything else and for a frame shorter than its system's.  Equal to
 * mi_dv_profile_of wherever that is not -1 (which keeps answering -1 for DVCPRO 625/50 4:1:1, as mi_dv_system_of
 * does).  Host only. */
int mi_dv_kind_of(const uint8_t *frame, size_t len);
/* mi_dv_decode_batch for any system: frames of the system's size in, pictures of the system's size out
 * (MI_DV_625_FRAME_BYTES / MI_DV_625_PICTURE_BYTES for 625/50: Y 720 x 576, Cb 360 x 288, Cr 360 x 288, tightly
 * packed; MI_DV_625_FRAME_BYTES / MI_DV_625_411_PICTURE_BYTES for 625/50 4:1:1: Y 720 x 576, Cb 180 x 576, Cr 180 x 576;
 * MI_DV_525_422_* / MI_DV_625_422_* for the 4:2:2 systems: Y 720 x H, Cb 360 x H, Cr 360 x H).  The same rules
 * on alignment, batch size and kernel times; for MI_DV_SYS_525_60 the same output byte for byte.  MI_DV_ERR_ARG for an
 * unknown system. */
int mi_dv_decode_batch_sys(mi_dv_ctx *c, int system, const void *d_frames, int n, void *d_pics);
/* mi_dv_decode_frame for any system (for MI_DV_SYS_525_60 it is that function).  MI_DV_ERR_FORMAT for a frame that
 * does not announce `system` (for MI_DV_SYS_625_50_411: for which mi_dv_kind_of does not say so) or is shorter than its
 * frames; MI_DV_ERR_ARG for an unknown system.  One instance takes frames of all five systems in any order. */
int mi_dv_decode_frame_sys(mi_dv_ctx *c, int system, const uint8_t *frame, size_t len, uint8_t *const planes[3],
                           const int strides[3]);
/* The kernels' own macroblock placement: macroblock m (0..4) of video segment `slot` (0..26) of DIF sequence `seq`.
 * 525/60: x in 32-pixel columns, y in 8-line rows (a column-22 macroblock is 16 x 16 pixels), as in the oracle;
 * 625/50: x, y in 16 x 16 macroblocks (0..44, 0..35).  625/50 4:1:1: seq 0..11, in the units of 525/60 (x in 32-pixel
 * columns 0..22, y in 8-line rows 0..71).  The 4:2:2 systems: `seq` counts the frame's DIF sequences in
 * byte order, 0..19 / 0..23 (channel seq / 10, seq / 12); x in 16-pixel columns (0..44), y in 8-line rows (0..59 /
 * 0..71).  Host only; MI_DV_ERR_ARG for arguments out of range. */
int mi_dv_mb_place(int system, int seq, int slot, int m, int *x, int *y);

/* ---- macroblocks the stream flags as errors keep the stream's last good pixels ----
 *
 * Byte 3 of every compressed macroblock (DIF block) is STA | QNO.  The calls above drop STA, so to them "damaged frames
 * are not detected"; the calls below read it.  A macroblock is HELD when bit STA (the high nibble, 0..15) is set in a
 * 16-bit mask.  The default, MI_DV_STA_ERRORS, holds STA 0111 and 1111 ("error exists"); 0010, 0100, 0110, 1010, 1100
 * and 1110 say that the SOURCE already concealed the macroblock: its data are valid and are decoded.  UNPINNED like the
 * rest of this decoder: this is the repository's reading of IEC 61834-2 from memory.  The rule is this one mask, so
 * correcting it is one line, and every call takes the caller's own (0: the default).
 * A held macroblock is held as a whole.  Its neighbours in the video segment, which may have lent it bits in the third
 * pass, are decoded as they are.
 * A held macroblock of picture k of a stream is that macroblock of the nearest earlier picture of the stream in which it
 * is good; where there is none it stays what the decoder made of its bytes. */
enum { MI_DV_STA_ERRORS = 0x8080 };
/* The three rectangles {x, y, w, h} macroblock m (0..4) of video segment `slot` (0..26) of DIF sequence `seq` (as
 * mi_dv_mb_place takes it) covers: rect[0] of Y, rect[1] of Cb, rect[2] of Cr, each in its plane's own pixels.  4:1:1:
 * 32 x 8 and 8 x 8, in column 22 16 x 16 and 4 x 16 (the chroma block's halves one above the other); 625/50 4:2:0:
 * 16 x 16 and 8 x 8; 4:2:2: 16 x 8 and 8 x 8.  Macroblock 5 (27 seq + slot) + m of a frame; its DIF block is block
 * 7 + v + v / 15 of its sequence, v = 5 slot + m.  Host only; MI_DV_ERR_ARG for arguments out of range. */
int mi_dv_mb_rects(int system, int seq, int slot, int m, int rect[3][4]);
/* How many macroblocks of a frame (at least the system's frame bytes) the mask holds (0: MI_DV_STA_ERRORS).  Host only;
 * MI_DV_ERR_ARG for an unknown system, a NULL or short frame, a mask above 0xFFFF. */
int mi_dv_held_macroblocks(int system, const uint8_t *frame, size_t len, unsigned sta_mask);
/* mi_dv_decode_batch_sys with held macroblocks.  The n frames are n_runs runs of consecutive frames of one stream each
 * (run_len adds up to n; n_runs 0 or run_len NULL: one run).  d_prev: the picture before each run, n_runs pictures back
 * to back (8-byte aligned, not overlapping d_pics), or NULL; where a macroblock is good in no earlier picture of its run
 * it comes from the run's picture of d_prev.  sta_mask 0: MI_DV_STA_ERRORS.  Queued on the instance's stream like
 * mi_dv_decode_batch_sys; buffers of the instance grow when needed (the call may synchronise then) and never shrink.
 * With no macroblock held the pictures are those of mi_dv_decode_batch_sys byte for byte; a run of one picture without
 * d_prev has no source and costs nothing more.  MI_DV_ERR_ARG, with nothing launched, for an unknown system, n out of
 * range or misaligned buffers (the rules of mi_dv_decode_batch), a run length <= 0, lengths that do not add up to n,
 * d_prev overlapping d_pics, a mask above 0xFFFF. */
int mi_dv_decode_batch_held(mi_dv_ctx *c, int system, const void *d_frames, int n, void *d_pics, int n_runs, const int *run_len,
                            const void *d_prev, unsigned sta_mask);
/* The macroblocks the last held batch took from another picture (held ones without a source do not count).  Synchronises. */
int mi_dv_hold_stats(mi_dv_ctx *c, long long *held);
/* Device time of the hold pass alone (k_dv_hold_mask, k_dv_hold_carry, k_dv_hold_copy: three launches a batch that has a
 * source) since the last call, as mi_dv_kernel_times, which keeps counting k_dv_decode alone. */
int mi_dv_hold_times(mi_dv_ctx *c, float *total_ms, int *launches);
/* mi_dv_decode_frame_sys with held macroblocks: the instance keeps the picture of the last frame this call decoded on
 * the device, and that picture is the next frame's source, as d_prev is a run's: the whole picture, so a macroblock
 * held in two frames running keeps what the kept picture holds.  The checks and messages of mi_dv_decode_frame_sys.  No
 * source, so that held macroblocks stay as decoded: for the first frame, the first after mi_dv_hold_reset, the first of
 * another system than the frame before, and a frame that follows a refused one.  *held (may be NULL): the macroblocks
 * taken from the kept picture. */
int mi_dv_decode_frame_held(mi_dv_ctx *c, int system, const uint8_t *frame, size_t len, uint8_t *const planes[3],
                            const int strides[3], unsigned sta_mask, int *held);
/* Forget the kept picture (a decoder's .resync: after a seek the frame before is not the stream's previous picture). */
int mi_dv_hold_reset(mi_dv_ctx *c);

/* ---- the encoder: pictures on the device -> DIF frames of any of the five systems ----
 *
 * PARITY UNPINNED like the decoder: the frames follow this repository's reading of the format (oracle/dv_oracle.c) and
 * the integer statement tests/dvenc.py, which the kernel reproduces bit for bit; this library decodes them, and so does
 * the oracle.  Nothing here was compared with another DV implementation.  Every frame is complete: the video segments
 * (forward transforms, quantisation by the largest quantisation number at which a segment fits its 2,680 AC bits, the
 * three passes), block ids with the channel bit, DSF, the system's default APT and VAUX stype (mi_dv_kind_of answers the
 * system), zeros everywhere else: no audio until mi_dv_audio_write_batch, no subcode or VAUX content until mi_dv_meta_write_batch.  flags: bit 0 lets a block take the 2-4-8 transform
 * where its two fields differ, bit 1 gives every block a class by its content (clear: class 0). */

/* n pictures of the system's size, resident in device memory and back to back (the layout mi_dv_decode_batch_sys
 * writes), -> n frames of the system's size.  The alignment and batch rules of mi_dv_decode_batch_sys: d_pics 8-byte,
 * d_frames 4-byte aligned, at most 65535 per call.  Queued on the instance's stream; pair with mi_dv_sync.  MI_DV_ERR_ARG,
 * with nothing launched, for an unknown system, n out of range, NULL, misaligned or overlapping buffers, flags above 3. */
int mi_dv_encode_batch(mi_dv_ctx *c, int system, const void *d_pics, int n, void *d_frames, int flags);
/* One picture from the caller's planes (Y, Cb, Cr) with the caller's strides into `cap` bytes of host memory.
 * Synchronous.  MI_DV_ERR_ARG for a cap below the system's frame bytes, strides below the planes' widths, flags above 3,
 * an unknown system. */
int mi_dv_encode_frame(mi_dv_ctx *c, int system, const uint8_t *const planes[3], const int strides[3], uint8_t *frame,
                       size_t cap, int flags);
/* Device time of k_dv_encode since the last call, as mi_dv_kernel_times, which keeps counting k_dv_decode alone. */
int mi_dv_encode_times(mi_dv_ctx *c, float *total_ms, int *launches);
/* Of the last encoded batch: the video segments per chosen quantisation number, and the levels the overflow rule
 * dropped (a segment that does not fit at quantisation number 0 loses last levels of its longest blocks).  Synchronises. */
int mi_dv_encode_stats(mi_dv_ctx *c, long long qno_hist[16], long long *dropped);

/* ---- the sound of resident frames, read and written on the device ----
 *
 * What include/mi_dvframe.h's host reader does with one frame, for a batch: the AAUX source pack of every frame (audio
 * block 3 of sequence 0: samples beyond the rate's minimum, rate, quantisation), then the de-shuffle of its audio blocks
 * into interleaved stereo PCM, byte for byte what that reader writes into zeroed buffers (the statement: tests/dvaudio.py).
 * Reading is pinned like the reader, to lib/dvframe.c where that is defined (include/mi_dvframe.h; the kernel is held to
 * the reference's recorded answers by tests/test_gpu_dv_reference.py).  The other way round only 16-bit sound is written;
 * the AAUX packs it writes are this repository's reading of IEC 61834-4 and UNPINNED (nothing in the reference writes
 * any): this library's readers read them back. */
enum { MI_DV_AUDIO_PAIRS = 4, MI_DV_AUDIO_PAIR_BYTES = 8192 };
/* n resident frames of `system` -> d_pcm[n][pairs][MI_DV_AUDIO_PAIR_BYTES] (interleaved stereo S16LE, 16-byte aligned),
 * d_info[n][4] int32 (4-byte aligned): samples per channel (0: no source pack, -1: unsupported quantisation or rate), and,
 * where that is positive (else 0): the rate in Hz, the pairs the frame's blocks fill (the system's channels, twice as many
 * in 12-bit mode), the bits (16 / 12).  Every byte of d_pcm is written: past 4 * samples, and in pairs the frame does not
 * carry, zero.  pairs 1..4; pairs the frame carries beyond `pairs` are dropped, as the host call drops pairs it has no
 * buffer for.  Queued on the instance's stream; pair with mi_dv_sync.  MI_DV_ERR_ARG, with nothing launched, for an unknown
 * system, n out of 1..65535, NULL or misaligned buffers, pairs out of range, buffers that overlap. */
int mi_dv_audio_batch(mi_dv_ctx *c, int system, const void *d_frames, int n, void *d_pcm, int pairs, void *d_info);
/* PCM into the audio blocks of n resident frames (16-bit): all 9 audio DIF blocks of every sequence are rewritten whole
 * (ids as the encoder writes them, AAUX packs, samples) and no other byte.  d_pcm as above; pair k goes to DIF channel k.
 * samplerate 48000 / 44100 / 32000; samples[i] (host array, read before the call returns) within [min, min + 63] of the
 * system and rate (525/60: min 1580 / 1452 / 1053, 625/50: 1896 / 1742 / 1264); pairs >= the system's channels (1 or 2),
 * the first ones are used.  A sample of -32768 is written as -32767 (0x8000 is the format's "no sample").  Queued on the
 * instance's stream: straight after mi_dv_encode_batch it needs no sync.  MI_DV_ERR_ARG, with nothing launched, as above
 * and for a bad rate or a sample count outside its window. */
int mi_dv_audio_write_batch(mi_dv_ctx *c, int system, void *d_frames, int n, const void *d_pcm, int pairs,
                            int samplerate, const int *samples);
/* The samples of frame `frame` (from 0) of an unlocked stream: floor((k + 1) rate / fps) - floor(k rate / fps) with the
 * system's frame rate (30000/1001 or 25) in 64-bit integers.  Host only; MI_DV_ERR_ARG for an unknown system or rate and
 * a frame below 0 or above 2^31 (the products stay in 64 bits). */
int mi_dv_audio_samples(int system, int samplerate, long long frame);
/* Device time of k_dv_audio_extract and k_dv_audio_write (one launch a batch call) since the last call, as
 * mi_dv_kernel_times, which keeps counting k_dv_decode alone. */
int mi_dv_audio_times(mi_dv_ctx *c, float *total_ms, int *launches);
/* The sound's layout table exactly as both kernels read it (csrc/dv_common.h, struct AudioTables: uint16 shuffle[2][12][9],
 * stride[2], min_samples[2][3]; row 0: 525/60, row 1: 625/50).  Host only, as mi_dv_copy_tables. */
size_t mi_dv_audio_copy_tables(void *out, size_t cap);

/* ---- timecode, recording date and time, aspect of resident frames, read and written on the device ----
 *
 * What include/mi_dvframe.h's mi_dv_timecode, mi_dv_date, mi_dv_time and mi_dv_pixel_aspect answer for one host frame,
 * for a batch (the statement: tests/dvmeta.py); and the writer of the two subcode and three VAUX DIF blocks of every
 * sequence, which the encoder leaves blank.  The readers restate GetSSYBPack and its users (lib/dvframe.c:678-783,
 * :460-471) and are pinned to that file (include/mi_dvframe.h; tests/test_gpu_dv_reference.py for the kernel).  PARITY
 * UNPINNED in the writing direction: the packs written are this repository's reading of IEC 61834-2/-4 from memory
 * (nothing in the reference writes any), and what is checked is that this library's readers, on host and device, read
 * them back. */
enum {
  MI_DV_META_INTS = 16,      /* int32 per frame in d_meta */
  MI_DV_META_FOUND = 0,      /* MI_DV_META_HAS_* */
  MI_DV_META_TC_HOUR = 1, MI_DV_META_TC_MINUTE = 2, MI_DV_META_TC_SECOND = 3, MI_DV_META_TC_FRAME = 4,
  MI_DV_META_TC_DROP = 5,    /* bit 6 of the timecode pack's byte 1 */
  MI_DV_META_YEAR = 6,       /* two digits with the reference's pivot: below 25 -> 20xx, else 19xx */
  MI_DV_META_MONTH = 7, MI_DV_META_DAY = 8,
  MI_DV_META_HOUR = 9, MI_DV_META_MINUTE = 10, MI_DV_META_SECOND = 11,
  MI_DV_META_WIDE = 12,      /* 1: mi_dv_pixel_aspect would answer the 16:9 ratio */
  MI_DV_META_TC_RAW = 13, MI_DV_META_DATE_RAW = 14, MI_DV_META_TIME_RAW = 15 /* bytes 1..4 of the pack, little-endian */
};
enum {
  MI_DV_META_HAS_TIMECODE = 1, /* pack 0x13 in a subcode packet of channel 0 */
  MI_DV_META_HAS_DATE = 2,     /* pack 0x62 */
  MI_DV_META_HAS_TIME = 4,     /* pack 0x63 */
  MI_DV_META_HAS_CONTROL = 8   /* the VAUX source control pack 0x61 at byte 80 * 5 + 48 + 5 */
};
/* n resident frames of `system` (4-byte aligned) -> d_meta[n][MI_DV_META_INTS] int32 (64-byte aligned, not overlapping the
 * frames).  Each pack is the first in the host reader's order: sequence, subcode block, packet, over the sequences of
 * channel 0.  Every field of a pack that was not found is 0.  Queued on the instance's stream; pair with mi_dv_sync.
 * MI_DV_ERR_ARG, with nothing launched, for an unknown system, n out of 1..65535, NULL, misaligned or overlapping buffers. */
int mi_dv_meta_batch(mi_dv_ctx *c, int system, const void *d_frames, int n, void *d_meta);
/* Rewrites the two subcode and the three VAUX DIF blocks of every sequence of every channel of n resident frames, whole,
 * and no other byte: ids as the encoder writes them; in the subcode packets timecode (0x13), recording date (0x62) and
 * recording time (0x63) in turns; in the first and third VAUX block the packs 0x60 (DSF and the system's stype: the
 * frame's kind stays what it was), 0x61 (the aspect: `wide`), 0x62, 0x63; FF elsewhere.  Frame k carries the timecode
 * of frame number first_frame + k (25 or 30 frames a second; drop_frame 1, 525/60 systems only: SMPTE drop-frame) and
 * the recording time rec_seconds + floor(k / frame rate), in seconds from 1970-01-01 00:00:00 with no time zone;
 * rec_seconds below 0: no date and no time (the packs are FF x 5).  A year from 2025 on reads back as 19xx: the readers'
 * pivot.  One call per run of consecutive frames.  Queued on the instance's stream: straight after mi_dv_encode_batch or
 * mi_dv_audio_write_batch it needs no sync.  MI_DV_ERR_ARG, with nothing launched, for an unknown system, n out of
 * 1..65535, a NULL or misaligned d_frames, drop_frame outside {0, 1} or 1 on a 625/50 system, first_frame below 0 or
 * first_frame + n above 2^40, rec_seconds from 3155760000 (the year 2070) on, wide outside {0, 1}. */
int mi_dv_meta_write_batch(mi_dv_ctx *c, int system, void *d_frames, int n, long long first_frame, int drop_frame,
                           long long rec_seconds, int wide);
/* The timecode of frame number `frame` (from 0) as the writer makes it: hours (wrapping at 24), minutes, seconds,
 * frames.  Host only; MI_DV_ERR_ARG for an unknown system, a frame below 0, drop_frame outside {0, 1} or 1 on a 625/50
 * system, a NULL hmsf. */
int mi_dv_timecode_of(int system, long long frame, int drop_frame, int hmsf[4]);
/* Device time of k_dv_meta_extract and k_dv_meta_write (one launch a batch call) since the last call, as
 * mi_dv_kernel_times, which keeps counting k_dv_decode alone. */
int mi_dv_meta_times(mi_dv_ctx *c, float *total_ms, int *launches);

#ifdef __cplusplus
}
#endif
#endif
