/*
 * mi_gsm.h — C ABI of the MI355X (gfx950) decoder of GSM 06.10 full-rate audio: what lib/audio_gsm.c decodes with the
 * vendored lib/GSM610/, fourccs 'agsm' and 'GSM ' (fmt 0) and the Microsoft framing of WAV ids 0x31 and 0x32, "MSGM"
 * (fmt 1).  n streams resident in device memory -> their samples, one call, nothing read on the host.  Plain C types
 * only; libmi_gsm.so.
 *
 * PINNED BY STATEMENT, PLUS RECORDED VECTORS, NOT BY BUILD: every rule is in upstream's files and is cited below; the
 * checker is tests/gsmraw.py, which restates the cited lines loop for loop, and the kernel reproduces it byte for byte.
 * tests/golden/gsm_vectors.json holds results recorded from upstream's own files of lib/GSM610/, driven as lib/audio_gsm.c
 * drives them; the statement is held to them.  Nothing here is held to a build of those files.
 *
 * G is lib/GSM610/, A is lib/audio_gsm.c.
 *
 * PLAIN FRAMING (fmt 0): a frame is 33 bytes, most significant bit first; the high nibble of byte 0 is the magic 0xD
 * (G/gsm_decode.c:276).  The 76 parameters follow in this order (G/gsm_decode.c:278-376): LARc[8] of 6, 6, 5, 5, 4, 4,
 * 3, 3 bits, then for each of the four subframes Nc (7), bc (2), Mc (2), xmaxc (6) and xMc[13] (3 each).  A frame gives
 * 160 samples; a unit is a frame.  A packet holds whole frames, a tail under 33 bytes is dropped (A:118-126).
 * MICROSOFT FRAMING (fmt 1): a block is 65 bytes, least significant bit first, two frames of the same 76 fields, no
 * magic.  The first frame reads 32.5 bytes and leaves a nibble in frame_chain, the second call starts at byte 33
 * (A:130-138, G/gsm_decode.c:40-270): 520 bits in one run.  frame_index is back at 0 after every block: a unit is a
 * block and gives 320 samples.
 * A FRAME (G/decode.c:56-83): four times Gsm_RPE_Decoding (G/rpe.c:244-275, 369-441, 490-506, with gsm_sub, gsm_asl,
 * gsm_asr of G/add.c) and Gsm_Long_Term_Synthesis_Filtering (G/long_term.c:924-967: Nr falls back to nrp outside 40..120,
 * brp = gsm_QLB[bcr], the history moves 40 samples); then Gsm_Short_Term_Synthesis_Filter (G/short_term.c:44-195,
 * 280-318, 402-443: the LARs are decoded, interpolated with the frame before's for k = 0..12, 13..26, 27..39 and
 * 40..159, LARp_to_rp, the lattice over v[9]); then Postprocessing (G/decode.c:40-54).  The integer operations are those
 * of G/gsm610_priv.h:84-191: GSM_MULT_R and GSM_MULT do not saturate, results are narrowed by assignment to `word`.
 * S->fast is never set by A: the integer filter is the one that runs, the float forms are not part of this library.
 * STATE BETWEEN FRAMES: dp0[0..119], v[0..8], msr, nrp and the LARpp of the frame before.  gsm_create zeroes all of it
 * and sets nrp = 40.  Here a state is MI_GSM_STATE_BYTES = 288 bytes, 144 int16: dp[120], v[9], msr, nrp, LARpp[8],
 * then five zeros.
 *
 * DEPARTURE 1, BAD MAGIC: gsm_decode returns -1 before it touches the state, A ignores that and hands on its frame
 * buffer as the last call left it: a result that depends on a buffer this interface does not have.  Here the frame
 * leaves the state untouched, its 160 samples are written as zeros, and the frame is counted for its stream.
 * DEPARTURE 2, THE DEAD LATTICE BRANCH: the lattice's arm for tmp1 == MIN_WORD && tmp2 == MIN_WORD cannot be taken:
 * LARp_to_rp returns -32768 for no LARp in -32768..32767 (tests/test_gsmraw_cpu.py tries them all).  The statement keeps
 * the arm, the kernel has none.
 */
#ifndef MI_GSM_H
#define MI_GSM_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { MI_GSM_OK = 0, MI_GSM_ERR_ARG = -1, MI_GSM_ERR_HIP = -2, MI_GSM_ERR_NOMEM = -3 };
enum { MI_GSM_FRAME_BYTES = 33, MI_GSM_BLOCK_BYTES = 65, MI_GSM_FRAME_SAMPLES = 160, MI_GSM_PARAMS = 76, MI_GSM_STATE_BYTES = 288 };
enum { MI_GSM_MAX_STREAMS = 1 << 20, MI_GSM_MAX_UNITS = 1 << 24 };

typedef struct mi_gsm_ctx mi_gsm_ctx;

int mi_gsm_device_count(void);                  /* gfx950 devices usable by this process */
mi_gsm_ctx *mi_gsm_create(int device);          /* -1: the process's current device; NULL on failure (mi_gsm_last_error(NULL)) */
void mi_gsm_destroy(mi_gsm_ctx *c);
const char *mi_gsm_last_error(const mi_gsm_ctx *c);

/* device memory of the instance's device (plain device pointers; 256-byte aligned) */
void *mi_gsm_dev_alloc(mi_gsm_ctx *c, size_t bytes);
void mi_gsm_dev_free(mi_gsm_ctx *c, void *d);
int mi_gsm_h2d(mi_gsm_ctx *c, void *d, const void *h, size_t n); /* synchronous */
int mi_gsm_d2h(mi_gsm_ctx *c, void *h, const void *d, size_t n); /* synchronous */
int mi_gsm_sync(mi_gsm_ctx *c);

/* n fresh states (gsm_create's) at d_state, 16-byte aligned; n is 1..MI_GSM_MAX_STREAMS.  One launch queued on the
 * instance's stream, which mi_gsm_times does not count. */
int mi_gsm_state_reset(mi_gsm_ctx *c, void *d_state, int n);

/* The parameters of a 33-byte frame (fmt 0: 76) or a 65-byte block (fmt 1: 152, the first frame's first) in host memory,
 * in the order of the bit stream.  Returns 1 with nothing written for a bad magic, else 0; MI_GSM_ERR_ARG for a NULL
 * argument or another fmt.  Host only: the code is the unpacker the kernel runs. */
int mi_gsm_explode(const uint8_t *block, int fmt, int16_t *params);

/* The hot path: stream i is units[i] frames (fmt 0) or blocks (fmt 1) at d_stream + offsets[i], at any byte address; its
 * samples go to d_pcm + pcm_offsets[i] as native int16, 160 (or 320) a unit, the first unit's first; every unit's samples
 * are written.  offsets, units and pcm_offsets are in host memory; the call has its own copy of them when it returns.
 * d_pcm and every pcm_offsets[i] are 16-byte aligned; n is 1..MI_GSM_MAX_STREAMS; units[i] is at most MI_GSM_MAX_UNITS;
 * fmt is 0 or 1.  The ranges the call names must not overlap one another.
 * d_state: NULL (every stream starts fresh and its state is dropped), or n states of MI_GSM_STATE_BYTES, 16-byte aligned,
 * read and written back: a call of 5 units equals calls of 2 and 3 (an nrp outside 40..120, which no decode leaves, is
 * read as 40).  d_bad: NULL, or n counts, 4-byte aligned: the frames
 * of stream i whose magic was bad (fmt 1 has none).  units[i] == 0 writes only that stream's state and count.
 * One launch queued on the instance's stream (pair with mi_gsm_sync); the stream's bytes are never read on the host.
 * Nothing else is written: no byte outside the samples, the states and the counts.  MI_GSM_ERR_ARG, with nothing
 * launched and nothing written, for anything else. */
int mi_gsm_decode_batch(mi_gsm_ctx *c, const void *d_stream, const uint64_t *offsets, const uint32_t *units, int n, int fmt,
                        void *d_pcm, const uint64_t *pcm_offsets, void *d_state, uint32_t *d_bad);
/* One stream of len bytes from host memory, through staging buffers the instance owns.  Synchronous.  floor(len / 33)
 * or floor(len / 65) units, a tail is dropped; pcm takes 160 (or 320) samples a unit.  state_or_null: NULL (fresh, the
 * state is dropped) or MI_GSM_STATE_BYTES in host memory, read and written back.  bad: NULL or where the count goes. */
int mi_gsm_decode_stream(mi_gsm_ctx *c, const uint8_t *bytes, size_t len, int fmt, int16_t *pcm, void *state_or_null,
                         uint32_t *bad);
/* Device time of k_gsm_decode: every launch is bracketed with HIP events on the instance's stream; this sums them over
 * the launches since the last call (synchronises, then forgets them) and counts the launches, one a call.  Where nobody
 * asks, the newest 4096 launches are kept. */
int mi_gsm_times(mi_gsm_ctx *c, float *ms, int *launches);

#ifdef __cplusplus
}
#endif
#endif
