/*
 * dv_float.h — a second statement of the DV25 525/60 block arithmetic, in plain `double`, that the fixed-point
 * statement (dv_oracle.c) and the GPU kernel are compared with.  TEST INFRASTRUCTURE ONLY: nothing in the product loads it.
 *
 * PARITY UNPINNED, like dv_oracle.h.  What this file pins: that the fixed-point arithmetic (14-bit multipliers folded
 * with a scaled transform's factors, a shared 8-bit butterfly, int16 coefficients) realises the closed form the header
 * comment of dv_oracle.c states — weights w(0..7), W(h,v) = w(h) w(v) / 2 (8-8) or w(h) w(2v) / 2 (2-4-8), DC 1/4,
 * orthonormal 8-point and 4-point inverse cosine transforms.  What it does not pin: the closed form to the standard,
 * and the bit layout to anything beyond the repository's parsers (this file's is a third one, written from the same
 * memory of the format).
 *
 * It shares no code with dv_oracle.c.  It restates constant data of the format only (the variable-length code's
 * length / run / amplitude arrays, the two scan orders, the quantiser shift table with class offsets and area limits,
 * the DIF block offsets, the macroblock placement); tests/test_dv_float_cpu.py compares each with the oracle's.  The
 * transforms are matrix products with cos() entries; there are no reconstruction multipliers and no butterfly.
 *
 * Arithmetic of a block with header dc (9-bit signed), mode, cls, quantisation number qno and levels L[k], k = 1..63
 * in scan order, (r, h) the natural position of k:
 *   F(r,h) = L[k] 2^s / W,  s = shift[qno + offset[cls]][area(k)] + (cls == 3),
 *   W = w(h) w(r) / 2 in 8-8 mode, w(h) w(2 (r >> 1)) / 2 in 2-4-8 mode;  F(0,0) = 4 dc
 *   8-8:    pixel = D8' F D8 + 128
 *   2-4-8:  S = even rows of F, D = odd rows; a = D4' S D8, b = D4' D D8; line 2i = (a_i + b_i) / sqrt 2 + 128,
 *           line 2i + 1 = (a_i - b_i) / sqrt 2 + 128
 * Output is the unrounded double; rounding and the 0..255 clip are the comparison's business.
 *
 * RANGE.  A block is "in range" when the fixed-point design cannot narrow: every |F| <= 16383 (the design's
 * coefficient is F times a transform prescale below 2, in int16), every value after the first (column) pass at most
 * 8191 in magnitude (the design carries it times a factor below 4), and every unclipped pixel within -4095 .. 4095
 * (the design holds 8 x pixel in int16 before its last shift).  Outside that range the oracle's int16 narrowing is
 * normative by definition and this model has nothing to say.
 */
#ifndef DV_FLOAT_H
#define DV_FLOAT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { DVF_W = 720, DVF_H = 480, DVF_CW = 180, DVF_FRAME_BYTES = 120000, DVF_PIC_BYTES = 720 * 480 * 3 / 2,
       DVF_SEGMENTS = 270, DVF_MACROBLOCKS = 1350, DVF_BLOCKS = 8100, DVF_SEGMENT_AC_BITS = 2680 };
/* blocks are numbered ((seq * 27 + slot) * 5 + m) * 6 + j everywhere, macroblocks (seq * 27 + slot) * 5 + m */

/* TEST-ONLY: a deliberately wrong decoder model, to show that the recorded bounds have teeth.  0 = the statement;
 * 1: w(4) = 1;  2: w(2) and w(3) swapped;  3: area 1 begins at scan position 7 instead of 6;  4: class 3 not doubled;
 * 5: DC scale halved;  6: 2-4-8 sum and difference rows exchanged.  The encoder and the writer are never perturbed. */
enum { DVF_PERTURBATIONS = 6 };
void dvf_set_perturbation(int which);

/* the restated constant data */
void dvf_scan(int mode, uint8_t out[64]);
int dvf_area(int k);
/* s of the formula above: dvo_shift() returns s + 1 */
int dvf_shift(int qno, int cls, int area);
/* as dvo_vlc_lookup, by walking the code one bit at a time */
int dvf_vlc_lookup(uint32_t bits16, int *len, int *run, int *level);
void dvf_mb_place(int seq, int slot, int m, int *x, int *y);
/* byte offset in the frame of video DIF block v (0..134) of sequence seq, and of block area j (0..5) inside it */
int dvf_block_offset(int seq, int v);
int dvf_area_offset(int j);
/* the closed-form weight W of natural position nat in a mode */
double dvf_weight(int mode, int nat);

/* n blocks: (dc, mode, cls, qno, levels[64] in scan order, levels[0] unused) -> 64 unrounded pixels each, row major;
 * inrange[i] (may be NULL) = 1 when block i is inside the range stated above */
void dvf_blocks(int n, const int16_t *dc, const uint8_t *mode, const uint8_t *cls, const uint8_t *qno, const int16_t (*levels)[64],
                double (*px)[64], uint8_t *inrange);
/* AC bits of a block's levels, end-of-block word included */
int dvf_block_bits(const int16_t levels[64]);

/* one DIF frame -> one unrounded picture (the oracle's plane order); returns the number of blocks outside the range.
 * inrange (DVF_BLOCKS, may be NULL); finished (may be NULL): blocks that ended in pass 1 / 2 / 3, [3] = never */
int dvf_decode_frame(const uint8_t *dif, double *pic, uint8_t *inrange, long finished[4]);
/* the symbols of a frame as the parser read them (any of the outputs may be NULL) */
void dvf_parse_frame(const uint8_t *dif, uint8_t *qno, int16_t *dc, uint8_t *mode, uint8_t *cls, int16_t (*levels)[64]);

/* symbols -> one DIF frame (ids and 525/60 profile bits as dvo_encode_frame writes them).  Returns 0, or -(1 + segment)
 * for the first segment whose AC words need more than DVF_SEGMENT_AC_BITS, or -1000 for a symbol out of its field
 * (dc -256..255, |level| <= 255, qno < 16, cls < 4, mode < 2). */
int dvf_write_frame(const uint8_t *qno, const int16_t *dc, const uint8_t *mode, const uint8_t *cls, const int16_t (*levels)[64],
                    uint8_t *dif);

/* a plain encoder that is no decoder's inverse: forward orthonormal transform, times W, over 2^s, rounded; DC
 * round(F00 / 4).  flags: bit 0 = 2-4-8 where the two fields differ, bit 1 = class by the block's largest coefficient.
 * qno_start (DVF_SEGMENTS entries, may be NULL = 15 everywhere): where each segment's rate control begins. */
void dvf_encode_frame(const uint8_t *pic, uint8_t *dif, int flags, const uint8_t *qno_start);

#ifdef __cplusplus
}
#endif
#endif
