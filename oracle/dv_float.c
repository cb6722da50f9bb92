/*
 * dv_float.c — see dv_float.h.  TEST INFRASTRUCTURE ONLY; PARITY UNPINNED.  A floating-point statement of the DV25
 * block arithmetic with a bit-serial three-pass parser, a plain encoder and a frame writer from symbols.  It shares
 * no code with dv_oracle.c: the tables below are the format's constant data restated (and compared with the oracle's
 * by tests/test_dv_float_cpu.py), the transforms are products with cos() matrices.
 */
#include "dv_float.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

/* ---- constant data of the format ---- */
/* the variable-length code in code order: length without the sign bit, run (255 = end of block), amplitude */
static const uint8_t code_len[89] = {2,  3,  4,  4,  4,  4,  5,  5,  5,  5,  6,  6,  6,  6,  7,  7,  7,  7,  7,  7,  7,  7,  8,
                                     8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  8,  9,  9,  9,  9,  9,  9,  9,  9,
                                     9,  9,  9,  9,  9,  9,  9,  9,  10, 10, 10, 10, 10, 10, 10, 11, 11, 11, 11, 11, 11, 11, 11,
                                     12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12};
static const uint8_t code_run[89] = {0,  0,  255, 1, 0, 0, 2, 1, 0, 0, 3, 4, 0, 0, 5, 6, 2, 1, 1, 0, 0, 0, 7,
                                     8,  9,  10,  3, 4, 2, 1, 1, 1, 0, 0, 0, 0, 0, 0, 11, 12, 13, 14, 5, 6, 3, 4,
                                     2,  2,  1,   0, 0, 0, 0, 0, 5, 3, 3, 2, 1, 1, 1, 0, 1, 6, 4, 3, 1, 1, 1,
                                     2,  3,  4,   5, 7, 8, 9, 10, 7, 8, 4, 3, 2, 2, 2, 2, 2, 1, 1, 1};
static const uint8_t code_amp[89] = {1,  2,  0,  1,  3,  4,  1,  2,  5,  6,  1,  1,  7,  8,  1,  1,  2,  3,  4,  9,  10, 11, 1,
                                     1,  1,  1,  2,  2,  3,  5,  6,  7,  12, 13, 14, 15, 16, 17, 1,  1,  1,  1,  2,  2,  3,  3,
                                     4,  5,  8,  18, 19, 20, 21, 22, 3,  4,  5,  6,  9,  10, 11, 0,  0,  3,  4,  6,  12, 13, 14,
                                     0,  0,  0,  0,  2,  2,  2,  2,  3,  3,  5,  7,  7,  8,  9,  10, 11, 15, 16, 17};
/* after them: 64 words of 13 bits, 1111110 rrrrrr (a run of r zeros and one more), and 256 of 15 bits and a sign,
 * 1111111 aaaaaaaa s */
static const uint8_t scan_88[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
static const uint8_t scan_248[64] = {0,  8,  1,  9,  16, 24, 2,  10, 17, 25, 32, 40, 48, 56, 33, 41, 18, 26, 3,  11, 4,  12,
                                     19, 27, 34, 42, 49, 57, 50, 58, 35, 43, 20, 28, 5,  13, 6,  14, 21, 29, 36, 44, 51, 59,
                                     52, 60, 37, 45, 22, 30, 7,  15, 23, 31, 38, 46, 53, 61, 54, 62, 39, 47, 55, 63};
static const uint8_t shift_tab[22][4] = {{3, 3, 4, 4}, {3, 3, 4, 4}, {2, 3, 3, 4}, {2, 3, 3, 4}, {2, 2, 3, 3}, {2, 2, 3, 3},
                                         {1, 2, 2, 3}, {1, 2, 2, 3}, {1, 1, 2, 2}, {1, 1, 2, 2}, {0, 1, 1, 2}, {0, 1, 1, 2},
                                         {0, 0, 1, 1}, {0, 0, 1, 1}, {0, 0, 0, 1}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0},
                                         {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
static const uint8_t class_offset[4] = {6, 3, 0, 1};
static const uint8_t area_first[4] = {0, 6, 21, 43};        /* first scan position of each area */
static const uint8_t area_byte[6] = {4, 18, 32, 46, 60, 70}; /* the six block areas of a compressed macroblock */
static const uint8_t area_len[6] = {14, 14, 14, 14, 10, 10};

static int perturb;
void dvf_set_perturbation(int which) { perturb = which; }

/* ---- the model ---- */
static double D8[8][8], D4[4][4], wgt[8];
static uint16_t word[89];
static int first_of_len[18]; /* index of the first short word of each length (code order is length order) */
static int ready;

static void init(void) {
  if (ready) return;
  const double pi = acos(-1.0);
  for (int u = 0; u < 8; u++)
    for (int x = 0; x < 8; x++) D8[u][x] = sqrt((u ? 2.0 : 1.0) / 8) * cos((2 * x + 1) * u * pi / 16);
  for (int u = 0; u < 4; u++)
    for (int x = 0; x < 4; x++) D4[u][x] = sqrt((u ? 2.0 : 1.0) / 4) * cos((2 * x + 1) * u * pi / 8);
  double C[8];
  for (int m = 0; m < 8; m++) C[m] = cos(m * pi / 16);
  wgt[0] = 1;
  wgt[1] = C[4] / (4 * C[7] * C[2]);
  wgt[2] = C[4] / (2 * C[6]);
  wgt[3] = 1 / (2 * C[5]);
  wgt[4] = 7.0 / 8;
  wgt[5] = C[4] / C[3];
  wgt[6] = C[4] / C[2];
  wgt[7] = C[4] / C[1];
  /* code words: count upwards, a longer word continues the count shifted left */
  unsigned next = 0;
  for (int i = 0; i < 89; i++) {
    if (i) next = (next + 1) << (code_len[i] - code_len[i - 1]);
    word[i] = (uint16_t)next;
  }
  for (int l = 0; l < 18; l++) first_of_len[l] = 89;
  for (int i = 88; i >= 0; i--) first_of_len[code_len[i]] = i;
  ready = 1;
}

static double weight1(int m) {
  if (perturb == 1 && m == 4) return 1;
  if (perturb == 2 && (m == 2 || m == 3)) return wgt[5 - m];
  return wgt[m];
}
static double weight_of(int mode, int nat, int decoder) {
  const int r = nat >> 3, h = nat & 7, v = mode ? 2 * (r >> 1) : r;
  if (!decoder) return wgt[h] * wgt[v] / 2;
  return weight1(h) * weight1(v) / 2;
}
double dvf_weight(int mode, int nat) {
  init();
  return weight_of(mode, nat, 0);
}
static int area_at(int k, int decoder) {
  int a = 0;
  for (int i = 1; i < 4; i++) a += k >= area_first[i] + (decoder && perturb == 3 && i == 1);
  return a;
}
static int shift_at(int qno, int cls, int area, int decoder) {
  return shift_tab[qno + class_offset[cls]][area] + (cls == 3 && !(decoder && perturb == 4));
}
int dvf_area(int k) { return area_at(k, 0); }
int dvf_shift(int qno, int cls, int area) { return shift_at(qno, cls, area, 0); }
void dvf_scan(int mode, uint8_t out[64]) { memcpy(out, mode ? scan_248 : scan_88, 64); }
int dvf_block_offset(int seq, int v) { return (seq * 150 + 7 + v + v / 15) * 80; }
int dvf_area_offset(int j) { return area_byte[j]; }

void dvf_mb_place(int seq, int slot, int m, int *x, int *y) {
  /* super blocks of 27 macroblocks, 5 columns x 10 rows; a segment takes one macroblock from each of five of them */
  static const uint8_t sb_row[5] = {2, 6, 8, 0, 4}, sb_col[5] = {2, 1, 3, 0, 4};
  static const uint8_t col_first[5] = {0, 4, 9, 13, 18}; /* first 32-pixel column of a super-block column */
  const int row = (seq + sb_row[m]) % 10, col = sb_col[m];
  int k = slot + (col & 1 ? 3 : 0); /* the odd super-block columns begin half way down a column */
  const int c = k / 6, r = k % 6, down = c & 1 ? 5 - r : r;
  *x = col_first[col] + c;
  *y = 6 * row + (*x == 22 ? 2 * down : down); /* column 22 holds 16 x 16 macroblocks, three to a super block */
}

static void block(int dc, int mode, int cls, int qno, const int16_t *L, double *px, uint8_t *inrange) {
  double F[8][8] = {{0}}, T[8][8];
  const uint8_t *scan = mode ? scan_248 : scan_88;
  int ok = 1;
  for (int k = 1; k < 64; k++)
    if (L[k]) {
      const int nat = scan[k];
      const double f = L[k] * ldexp(1.0, shift_at(qno, cls, area_at(k, 1), 1)) / weight_of(mode, nat, 1);
      F[nat >> 3][nat & 7] = f;
      ok = ok && fabs(f) <= 16383;
    }
  F[0][0] = (perturb == 5 ? 2.0 : 4.0) * dc;
  if (mode && perturb == 6)
    for (int v = 0; v < 4; v++)
      for (int h = 0; h < 8; h++) {
        const double t = F[2 * v][h];
        F[2 * v][h] = F[2 * v + 1][h];
        F[2 * v + 1][h] = t;
      }
  /* the vertical pass */
  if (!mode) {
    for (int y = 0; y < 8; y++)
      for (int h = 0; h < 8; h++) {
        double s = 0;
        for (int r = 0; r < 8; r++) s += D8[r][y] * F[r][h];
        T[y][h] = s;
      }
  } else {
    for (int i = 0; i < 4; i++)
      for (int h = 0; h < 8; h++) {
        double a = 0, b = 0;
        for (int v = 0; v < 4; v++) a += D4[v][i] * F[2 * v][h], b += D4[v][i] * F[2 * v + 1][h];
        T[2 * i][h] = (a + b) / sqrt(2.0);
        T[2 * i + 1][h] = (a - b) / sqrt(2.0);
      }
  }
  /* the horizontal pass */
  for (int y = 0; y < 8; y++)
    for (int x = 0; x < 8; x++) {
      double s = 0;
      for (int h = 0; h < 8; h++) s += T[y][h] * D8[h][x];
      px[8 * y + x] = s + 128;
      ok = ok && fabs(T[y][x]) <= 8191 && fabs(s + 128) <= 4095;
    }
  if (inrange) *inrange = (uint8_t)ok;
}

void dvf_blocks(int n, const int16_t *dc, const uint8_t *mode, const uint8_t *cls, const uint8_t *qno, const int16_t (*levels)[64],
                double (*px)[64], uint8_t *inrange) {
  init();
  for (int i = 0; i < n; i++) block(dc[i], mode[i], cls[i], qno[i], levels[i], px[i], inrange ? inrange + i : NULL);
}

/* ---- the variable-length code, one bit at a time ---- */
typedef struct {
  unsigned acc; /* the bits of the word read so far */
  int n;
} wordstate;
/* takes one bit; returns 0 while the word is incomplete, else 1 with run (255: end of block) and the signed level */
static int take_bit(wordstate *w, int bit, int *run, int *level) {
  w->acc = (w->acc << 1) | (unsigned)bit;
  w->n++;
  const int n = w->n;
  /* a short word, or a short word and its sign */
  for (int signbit = 0; signbit < 2; signbit++) {
    const int l = n - signbit;
    if (l < 2 || l > 12) continue;
    const unsigned body = w->acc >> signbit;
    for (int i = first_of_len[l]; i < 89 && code_len[i] == l; i++)
      if (word[i] == body) {
        const int needs_sign = code_run[i] != 255 && code_amp[i] != 0;
        if (needs_sign != signbit) return 0; /* (needs_sign && !signbit): the sign comes next */
        *run = code_run[i];
        *level = signbit && (w->acc & 1) ? -(int)code_amp[i] : code_amp[i];
        w->acc = 0, w->n = 0;
        return 1;
      }
  }
  if (n == 13 && w->acc >> 6 == 0x7E) {
    *run = (int)(w->acc & 63), *level = 0;
    w->acc = 0, w->n = 0;
    return 1;
  }
  if (n == 16 && w->acc >> 9 == 0x7F) {
    *run = 0, *level = (int)((w->acc >> 1) & 255);
    if (w->acc & 1) *level = -*level;
    w->acc = 0, w->n = 0;
    return 1;
  }
  return 0;
}
int dvf_vlc_lookup(uint32_t bits16, int *len, int *run, int *level) {
  init();
  wordstate w = {0, 0};
  for (int i = 15; i >= 0; i--)
    if (take_bit(&w, (bits16 >> i) & 1, run, level)) {
      *len = 16 - i;
      return *run == 255;
    }
  abort(); /* the code is complete: every 16 bits begin with a word */
}

/* ---- the parser: three passes over a video segment, one bit at a time ---- */
typedef struct {
  int dc, mode, cls, pos, done, pass;
  wordstate w;
  int16_t level[64];
} pblock;
/* the block takes bits (positions in the segment's 5 x 80 bytes, listed in `bits` from *at to n) until it ends */
static void feed(pblock *b, const uint8_t *seg[5], const int *bits, int *at, int n, int pass) {
  while (!b->done && *at < n) {
    const int p = bits[(*at)++];
    int run, level;
    if (!take_bit(&b->w, (seg[p / 640][(p % 640) >> 3] >> (7 - (p & 7))) & 1, &run, &level)) continue;
    if (run == 255 || (b->pos += run + 1) > 63) {
      b->done = 1;
      b->pass = pass;
    } else {
      b->level[b->pos] = (int16_t)level;
    }
  }
}
static void parse_segment(const uint8_t *dif, int seq, int slot, pblock blk[30], int qno[5]) {
  const uint8_t *seg[5];
  static int own[112], mbits[5][640], vbits[3200];
  int mn[5], mat[5], vn = 0, vat = 0;
  for (int m = 0; m < 5; m++) {
    seg[m] = dif + dvf_block_offset(seq, 5 * slot + m);
    qno[m] = seg[m][3] & 15;
  }
  for (int m = 0; m < 5; m++) {
    mn[m] = mat[m] = 0;
    for (int j = 0; j < 6; j++) {
      pblock *b = &blk[6 * m + j];
      const uint8_t *a = seg[m] + area_byte[j];
      memset(b, 0, sizeof *b);
      b->dc = ((a[0] << 1) | (a[1] >> 7)) - ((a[0] & 0x80) ? 512 : 0);
      b->mode = (a[1] >> 6) & 1;
      b->cls = (a[1] >> 4) & 3;
      b->pass = 3;
      int n = 0, at = 0;
      for (int i = 12; i < 8 * area_len[j]; i++) own[n++] = 640 * m + 8 * area_byte[j] + i;
      feed(b, seg, own, &at, n, 0);
      while (at < n) mbits[m][mn[m]++] = own[at++];
    }
    for (int j = 0; j < 6; j++) feed(&blk[6 * m + j], seg, mbits[m], &mat[m], mn[m], 1);
    while (mat[m] < mn[m]) vbits[vn++] = mbits[m][mat[m]++];
  }
  for (int i = 0; i < 30; i++) feed(&blk[i], seg, vbits, &vat, vn, 2);
}

/* where pixel (r, c) of block j of the macroblock at (x, y) lives */
static int pixel_at(int x, int y, int j, int r, int c) {
  if (j < 4) {
    if (x < 22) return (8 * y + r) * DVF_W + 32 * x + 8 * j + c;
    return (8 * y + 8 * (j >> 1) + r) * DVF_W + 32 * x + 8 * (j & 1) + c;
  }
  const int plane = DVF_W * DVF_H + (j == 4 ? DVF_CW * DVF_H : 0); /* block 4 is Cr, the third plane */
  if (x < 22) return plane + (8 * y + r) * DVF_CW + 8 * x + c;
  return plane + (8 * y + r + (c < 4 ? 0 : 8)) * DVF_CW + 8 * x + (c & 3); /* right edge: the right half goes below */
}

int dvf_decode_frame(const uint8_t *dif, double *pic, uint8_t *inrange, long finished[4]) {
  init();
  int out = 0;
  if (finished) memset(finished, 0, 4 * sizeof *finished);
  for (int seq = 0; seq < 10; seq++)
    for (int slot = 0; slot < 27; slot++) {
      pblock blk[30];
      int qno[5];
      parse_segment(dif, seq, slot, blk, qno);
      for (int m = 0; m < 5; m++) {
        int x, y;
        dvf_mb_place(seq, slot, m, &x, &y);
        for (int j = 0; j < 6; j++) {
          const pblock *b = &blk[6 * m + j];
          double px[64];
          uint8_t ok;
          block(b->dc, b->mode, b->cls, qno[m], b->level, px, &ok);
          for (int i = 0; i < 64; i++) pic[pixel_at(x, y, j, i >> 3, i & 7)] = px[i];
          if (inrange) inrange[((seq * 27 + slot) * 5 + m) * 6 + j] = ok;
          if (finished) finished[b->pass]++;
          out += !ok;
        }
      }
    }
  return out;
}

void dvf_parse_frame(const uint8_t *dif, uint8_t *qno, int16_t *dc, uint8_t *mode, uint8_t *cls, int16_t (*levels)[64]) {
  init();
  for (int s = 0; s < DVF_SEGMENTS; s++) {
    pblock blk[30];
    int q[5];
    parse_segment(dif, s / 27, s % 27, blk, q);
    for (int i = 0; i < 30; i++) {
      if (qno) qno[5 * s + i / 6] = (uint8_t)q[i / 6];
      if (dc) dc[30 * s + i] = (int16_t)blk[i].dc;
      if (mode) mode[30 * s + i] = (uint8_t)blk[i].mode;
      if (cls) cls[30 * s + i] = (uint8_t)blk[i].cls;
      if (levels) memcpy(levels[30 * s + i], blk[i].level, sizeof blk[i].level);
    }
  }
}

/* ---- the writer ---- */
typedef struct {
  uint8_t bit[64 * 29 + 8];
  int n;
} bits_t;
static void put(bits_t *b, unsigned v, int n) {
  while (n--) b->bit[b->n++] = (v >> n) & 1;
}
static int short_word(int run, int amp) {
  for (int i = 0; i < 89; i++)
    if (code_run[i] == run && code_amp[i] == amp) return i;
  return -1;
}
static void put_zeros(bits_t *b, int run) { /* `run` zeros and one more */
  const int i = short_word(run, 0);
  if (i >= 0) put(b, word[i], code_len[i]);
  else put(b, (0x7Eu << 6) | (unsigned)run, 13);
}
static void put_amplitude(bits_t *b, int level) {
  const int amp = abs(level), i = short_word(0, amp);
  if (i >= 0) put(b, word[i], code_len[i]);
  else put(b, (0x7Fu << 8) | (unsigned)amp, 15);
  put(b, level < 0, 1);
}
static void block_words(const int16_t *L, bits_t *b) {
  b->n = 0;
  int run = 0;
  for (int k = 1; k < 64; k++) {
    if (!L[k]) {
      run++;
      continue;
    }
    const int i = short_word(run, abs(L[k]));
    if (i >= 0) {
      put(b, word[i], code_len[i]);
      put(b, L[k] < 0, 1);
    } else {
      if (run) put_zeros(b, run - 1);
      put_amplitude(b, L[k]);
    }
    run = 0;
  }
  const int e = short_word(255, 0);
  put(b, word[e], code_len[e]);
}
int dvf_block_bits(const int16_t levels[64]) {
  init();
  bits_t b;
  block_words(levels, &b);
  return b.n;
}

static int write_segment(uint8_t *dif, int seq, int slot, const uint8_t *qno, const int16_t *dc, const uint8_t *mode,
                         const uint8_t *cls, const int16_t (*levels)[64]) {
  static bits_t w[30];
  uint8_t *seg[5];
  int sent[30], total = 0;
  for (int i = 0; i < 30; i++) {
    block_words(levels[i], &w[i]);
    total += w[i].n;
    sent[i] = 0;
  }
  if (total > DVF_SEGMENT_AC_BITS) return -1;
  /* free bit positions, segment-wide numbering 640 m + bit in the DIF block */
  static int mfree[5][640], vfree[3200];
  int mn[5], vn = 0, vat = 0;
#define SETBIT(p) (seg[(p) / 640][((p) % 640) >> 3] |= (uint8_t)(0x80 >> ((p) & 7)))
  for (int m = 0; m < 5; m++) {
    seg[m] = dif + dvf_block_offset(seq, 5 * slot + m);
    seg[m][3] = qno[m]; /* STA 0 */
    memset(seg[m] + 4, 0, 76);
    mn[m] = 0;
    for (int j = 0; j < 6; j++) {
      const int i = 6 * m + j, p0 = 640 * m + 8 * area_byte[j];
      uint8_t *a = seg[m] + area_byte[j];
      a[0] = (uint8_t)((dc[i] & 511) >> 1);
      a[1] = (uint8_t)(((dc[i] & 1) << 7) | (mode[i] << 6) | (cls[i] << 4));
      for (int q = 12; q < 8 * area_len[j]; q++) {
        if (sent[i] < w[i].n) {
          if (w[i].bit[sent[i]]) SETBIT(p0 + q);
          sent[i]++;
        } else {
          mfree[m][mn[m]++] = p0 + q;
        }
      }
    }
    int at = 0;
    for (int j = 0; j < 6; j++)
      for (int i = 6 * m + j; sent[i] < w[i].n && at < mn[m]; sent[i]++, at++)
        if (w[i].bit[sent[i]]) SETBIT(mfree[m][at]);
    while (at < mn[m]) vfree[vn++] = mfree[m][at++];
  }
  for (int i = 0; i < 30; i++)
    for (; sent[i] < w[i].n && vat < vn; sent[i]++, vat++)
      if (w[i].bit[sent[i]]) SETBIT(vfree[vat]);
#undef SETBIT
  for (int i = 0; i < 30; i++)
    if (sent[i] < w[i].n) abort(); /* cannot happen: the areas hold DVF_SEGMENT_AC_BITS */
  return 0;
}

static void write_ids(uint8_t *dif) {
  memset(dif, 0, DVF_FRAME_BYTES);
  for (int seq = 0; seq < 10; seq++) {
    for (int b = 0; b < 150; b++) { /* section type, sequence, number within the section */
      uint8_t *id = dif + (seq * 150 + b) * 80;
      int type = b == 0 ? 0 : b < 3 ? 1 : b < 6 ? 2 : (b - 6) % 16 == 0 ? 3 : 4;
      int num = type == 0 ? 0 : type == 1 ? b - 1 : type == 2 ? b - 3 : type == 3 ? (b - 6) / 16 : (b - 6) - (b - 6) / 16 - 1;
      id[0] = (uint8_t)((type << 5) | 0x1F);
      id[1] = (uint8_t)((seq << 4) | 7);
      id[2] = (uint8_t)num;
    }
    dif[seq * 150 * 80 + 3] = 0x3F; /* header block: DSF 0 = 525/60 */
  }
}

int dvf_write_frame(const uint8_t *qno, const int16_t *dc, const uint8_t *mode, const uint8_t *cls, const int16_t (*levels)[64],
                    uint8_t *dif) {
  init();
  for (int i = 0; i < DVF_MACROBLOCKS; i++)
    if (qno[i] > 15) return -1000;
  for (int i = 0; i < DVF_BLOCKS; i++) {
    if (dc[i] < -256 || dc[i] > 255 || mode[i] > 1 || cls[i] > 3) return -1000;
    for (int k = 1; k < 64; k++)
      if (levels[i][k] < -255 || levels[i][k] > 255) return -1000;
  }
  write_ids(dif);
  for (int s = 0; s < DVF_SEGMENTS; s++)
    if (write_segment(dif, s / 27, s % 27, qno + 5 * s, dc + 30 * s, mode + 30 * s, cls + 30 * s, levels + 30 * s)) return -(1 + s);
  return 0;
}

/* ---- the plain encoder ---- */
typedef struct {
  int mode, cls;
  double F[64]; /* natural order */
} eblock;
static void forward(const double *px, int mode, double *F) {
  double T[8][8];
  for (int y = 0; y < 8; y++) /* rows first */
    for (int h = 0; h < 8; h++) {
      double s = 0;
      for (int x = 0; x < 8; x++) s += D8[h][x] * px[8 * y + x];
      T[y][h] = s;
    }
  for (int h = 0; h < 8; h++) {
    if (!mode) {
      for (int r = 0; r < 8; r++) {
        double s = 0;
        for (int y = 0; y < 8; y++) s += D8[r][y] * T[y][h];
        F[8 * r + h] = s;
      }
    } else {
      for (int v = 0; v < 4; v++) {
        double s = 0, d = 0;
        for (int i = 0; i < 4; i++) {
          s += D4[v][i] * (T[2 * i][h] + T[2 * i + 1][h]);
          d += D4[v][i] * (T[2 * i][h] - T[2 * i + 1][h]);
        }
        F[8 * (2 * v) + h] = s / sqrt(2.0);
        F[8 * (2 * v + 1) + h] = d / sqrt(2.0);
      }
    }
  }
}
static int quantise_block(const eblock *b, int qno, int keep, int16_t *L) {
  const uint8_t *scan = b->mode ? scan_248 : scan_88;
  memset(L, 0, 64 * sizeof *L);
  for (int k = 1; k <= keep; k++) {
    const int nat = scan[k];
    double v = floor(fabs(b->F[nat]) * weight_of(b->mode, nat, 0) / ldexp(1.0, shift_at(qno, b->cls, area_at(k, 0), 0)) + 0.5);
    if (v > 255) v = 255;
    L[k] = (int16_t)(b->F[nat] < 0 ? -v : v);
  }
  return dvf_block_bits(L);
}

void dvf_encode_frame(const uint8_t *pic, uint8_t *dif, int flags, const uint8_t *qno_start) {
  init();
  write_ids(dif);
  for (int s = 0; s < DVF_SEGMENTS; s++) {
    const int seq = s / 27, slot = s % 27;
    eblock blk[30];
    int16_t dc[30], L[30][64];
    uint8_t mode[30], cls[30], qnos[5];
    for (int m = 0; m < 5; m++) {
      int x, y;
      dvf_mb_place(seq, slot, m, &x, &y);
      for (int j = 0; j < 6; j++) {
        eblock *b = &blk[6 * m + j];
        double px[64], near = 0, far = 0;
        for (int i = 0; i < 64; i++) px[i] = pic[pixel_at(x, y, j, i >> 3, i & 7)] - 128.0;
        /* the fields differ: neighbouring lines are further apart (squared) than lines of the same field */
        for (int i = 0; i < 48; i++) near += (px[i] - px[i + 8]) * (px[i] - px[i + 8]), far += (px[i] - px[i + 16]) * (px[i] - px[i + 16]);
        b->mode = (flags & 1) && near > 3 * far + 256;
        forward(px, b->mode, b->F);
        double big = 0;
        for (int k = 1; k < 64; k++) {
          const double a = fabs(b->F[k]) * weight_of(b->mode, k, 0);
          if (a > big) big = a;
        }
        b->cls = !(flags & 2) ? 0 : big < 12 ? 0 : big < 36 ? 1 : big < 144 ? 2 : 3;
        const double d = floor(b->F[0] / 4 + 0.5);
        dc[6 * m + j] = (int16_t)(d < -256 ? -256 : d > 255 ? 255 : d);
        mode[6 * m + j] = (uint8_t)b->mode;
        cls[6 * m + j] = (uint8_t)b->cls;
      }
    }
    /* rate control: the finest quantisation number that fits; at the coarsest, give up the highest scan positions */
    int qno = qno_start ? qno_start[s] & 15 : 15, keep = 63;
    for (;;) {
      int total = 0;
      for (int i = 0; i < 30; i++) total += quantise_block(&blk[i], qno, keep, L[i]);
      if (total <= DVF_SEGMENT_AC_BITS) break;
      if (qno > 0) qno--;
      else keep--;
    }
    for (int m = 0; m < 5; m++) qnos[m] = (uint8_t)qno;
    if (write_segment(dif, seq, slot, qnos, dc, mode, cls, (const int16_t(*)[64])L)) abort();
  }
}
