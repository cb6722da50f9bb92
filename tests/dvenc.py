"""Integer statement of the DV encoder (k_dv_encode, csrc/dv_encode_kernels.h).  TEST INFRASTRUCTURE ONLY: the product never
imports it.  PARITY UNPINNED like everything DV here.  The kernel reproduces THIS bit for bit; numpy, integers only.

The unit is a video segment: 30 blocks of 64 pixels and the flags in, five 80-byte DIF blocks out (segment()).  encode525()
is a 525/60 frame of 270 of them with the non-video bytes of dvo_encode_frame; the other four systems are
dvsys.encode(system, pic, flags, encode525=dvenc.encode525).

The format (oracle/dv_oracle.c): 9-bit DC clipped to -256..255, mode, class; 100 AC bits for a luma
area and 68 for a chroma area, 2,680 a segment; levels clipped to +-255; code words spelled as the oracle's put_pair spells
them, a 4-bit end of block behind every block; three passes (own area, the macroblock's free bits in block order, the
segment's in macroblock then block order), a cut-off word continues in the next space, unused bits zero; byte 3 of each
macroblock is the segment's quantisation number with STA 0.

The encoder's own choices:
  transform   pixels - 128, times 8, through a scaled forward butterfly with 12-bit constants, (x c + 2048) >> 12: along the
              lines, then down the columns (8-8), or the 4-point butterfly (the 8-point one's even half) on the sums and on
              the differences of line pairs (2-4-8: rows 2v / 2v + 1 of the result).  Coefficient (r, h) is the orthonormal
              one times a fixed ratio (tools/dv_encode_tables.py).
  DC          (c00 + 128) >> 8, clipped: the orthonormal DC over 4, rounded.
  quantiser   P = |c| MULT[mode][k] (below 2^31), level = min((P + half) >> n, 255) with n = 20 + the quantiser shift of
              (qno, class, area of k), half = 1 << (n - 1); the sign restored.  MULT folds the weight and 2^20 / ratio.
  mode        flags bit 0: 2-4-8 where d1 > 2 d2 + 64, d1 / d2 the summed absolute differences of the pixels of lines r and
              r + 1 / r + 2, r = 0..5 (the oracle's rule, which is integer already).
  class       flags bit 1: by big = max P >> 20 over the block's 63 AC positions: below 12 class 0, below 36 class 1, below
              144 class 2, else 3 (the float statement's thresholds on the same quantity); without the bit class 0.
  rate        the largest qno 0..15 at which the segment's 30 blocks need at most 2,680 bits; if 0 does not fit, the block
              with the most bits (the first such) loses its last non-zero level until it fits.

Four of these rules are module-level callables (mode_rule, clip_level, fits, most_bits) and two are tables (CLASS_LIMITS,
QUANT_SHIFT), so that a test can swap one and see which pictures notice; _mul is looked up by name at every call, so a test
can record its operands.  The pictures built to reach every branch of the rules — named edge segments scattered over the
segments of any system — are tests/dvenc_edges.py.
"""
import numpy as np

import dvlib as D
import dvsys as S

SEGMENTS, SEGMENT_AC_BITS = 270, 2680
FRAC = 20
C707, C383, C541, C1307 = 2896, 1567, 2217, 5352  # cos(pi/4), sin(pi/8), sqrt2 sin(pi/8), sqrt2 cos(pi/8), times 4096
CLASS_LIMITS = (12, 36, 144)
# by natural position (8 r + h), per mode: the multiplier, and the scan position (tools/dv_encode_tables.py)
MULT_NAT = (
    (8192, 5793, 5793, 6270, 7168, 8867, 11585, 21407, 5793, 4096, 4096, 4433, 5069, 6270, 8192, 15137, 5793, 4096, 4096, 4433,
     5069, 6270, 8192, 15137, 6270, 4433, 4433, 4799, 5486, 6786, 8867, 16384, 7168, 5069, 5069, 5486, 6272, 7759, 10137, 18731,
     8867, 6270, 6270, 6786, 7759, 9598, 12540, 23170, 11585, 8192, 8192, 8867, 10137, 12540, 16384, 30274, 21407, 15137, 15137,
     16384, 18731, 23170, 30274, 55938),
    (8192, 5793, 5793, 6270, 7168, 8867, 11585, 21407, 8192, 5793, 5793, 6270, 7168, 8867, 11585, 21407, 5793, 4096, 4096, 4433,
     5069, 6270, 8192, 15137, 5793, 4096, 4096, 4433, 5069, 6270, 8192, 15137, 7168, 5069, 5069, 5486, 6272, 7759, 10137, 18731,
     7168, 5069, 5069, 5486, 6272, 7759, 10137, 18731, 11585, 8192, 8192, 8867, 10137, 12540, 16384, 30274, 11585, 8192, 8192,
     8867, 10137, 12540, 16384, 30274),
)
POS_NAT = (
    (0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53, 10, 19,
     23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63),
    (0, 2, 6, 18, 20, 34, 36, 50, 1, 3, 7, 19, 21, 35, 37, 51, 4, 8, 16, 22, 32, 38, 48, 52, 5, 9, 17, 23, 33, 39, 49, 53, 10, 14,
     24, 30, 40, 46, 54, 60, 11, 15, 25, 31, 41, 47, 55, 61, 12, 26, 28, 42, 44, 56, 58, 62, 13, 27, 29, 43, 45, 57, 59, 63),
)
SCAN = np.argsort(np.array(POS_NAT), axis=1)                                  # [mode][k] -> natural position
MULT = np.take_along_axis(np.array(MULT_NAT, np.int64), SCAN, axis=1)         # [mode][k]; tests may halve an entry
AREA = np.array([0 if k < 6 else 1 if k < 21 else 2 if k < 43 else 3 for k in range(64)])
QUANT_SHIFT = np.array([[3, 3, 4, 4], [3, 3, 4, 4], [2, 3, 3, 4], [2, 3, 3, 4], [2, 2, 3, 3], [2, 2, 3, 3], [1, 2, 2, 3],
                        [1, 2, 2, 3], [1, 1, 2, 2], [1, 1, 2, 2], [0, 1, 1, 2], [0, 1, 1, 2], [0, 0, 1, 1], [0, 0, 1, 1],
                        [0, 0, 0, 1], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0],
                        [0, 0, 0, 0]])
CLASS_OFFSET = np.array([6, 3, 0, 1])
# the variable-length code in code order: lengths without the sign, run (255: end of block), amplitude
VLC_LEN = (2, 3, 4, 4, 4, 4, 5, 5, 5, 5, 6, 6, 6, 6, 7, 7, 7, 7, 7, 7, 7, 7, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 9, 9,
           9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 9, 10, 10, 10, 10, 10, 10, 10, 11, 11, 11, 11, 11, 11, 11, 11, 12, 12, 12, 12,
           12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12, 12)
VLC_RUN = (0, 0, 255, 1, 0, 0, 2, 1, 0, 0, 3, 4, 0, 0, 5, 6, 2, 1, 1, 0, 0, 0, 7, 8, 9, 10, 3, 4, 2, 1, 1, 1, 0, 0, 0, 0, 0, 0, 11,
           12, 13, 14, 5, 6, 3, 4, 2, 2, 1, 0, 0, 0, 0, 0, 5, 3, 3, 2, 1, 1, 1, 0, 1, 6, 4, 3, 1, 1, 1, 2, 3, 4, 5, 7, 8, 9, 10, 7,
           8, 4, 3, 2, 2, 2, 2, 2, 1, 1, 1)
VLC_AMP = (1, 2, 0, 1, 3, 4, 1, 2, 5, 6, 1, 1, 7, 8, 1, 1, 2, 3, 4, 9, 10, 11, 1, 1, 1, 1, 2, 2, 3, 5, 6, 7, 12, 13, 14, 15, 16,
           17, 1, 1, 1, 1, 2, 2, 3, 3, 4, 5, 8, 18, 19, 20, 21, 22, 3, 4, 5, 6, 9, 10, 11, 0, 0, 3, 4, 6, 12, 13, 14, 0, 0, 0, 0,
           2, 2, 2, 2, 3, 3, 5, 7, 7, 8, 9, 10, 11, 15, 16, 17)


def _words(amps=256):
    """PAIR_VAL / PAIR_LEN [run 0..62][amplitude 0..255] of a (run, amplitude) pair without its sign, as put_pair spells it:
    the listed word; else the zeros on their own (listed up to run 5, else 1111110 rrrrrr) and then the amplitude with run 0
    (listed up to 22, else 1111111 aaaaaaaa).  Amplitude 0 is unused.  And the end of block.  amps: a test that removes the
    clip asks for 512, and an amplitude above 255 then runs into the 1111111 in front of it."""
    listed, code, prev, eob = {}, 0, VLC_LEN[0], None
    for ln, run, amp in zip(VLC_LEN, VLC_RUN, VLC_AMP):
        code <<= ln - prev
        prev = ln
        if run == 255:
            eob = (code, ln)
        else:
            listed.setdefault((run, amp), (code, ln))
        code += 1
    val, length = np.zeros((63, amps), np.int64), np.zeros((63, amps), np.int64)
    for run in range(63):
        for amp in range(1, amps):
            if (run, amp) in listed:
                v, n = listed[run, amp]
            else:
                v, n = 0, 0
                if run:
                    v, n = listed[run - 1, 0] if run - 1 <= 5 else ((0x7E << 6) | (run - 1), 13)
                av, an = listed[0, amp] if amp <= 22 else ((0x7F << 8) | amp, 15)
                v, n = (v << an) | av, n + an
            val[run, amp], length[run, amp] = v, n
    return val, length, eob


PAIR_VAL, PAIR_LEN, EOB = _words()


# ---- the rules a test may swap (tests/test_dv_encode_edges_cpu.py does, one at a time, to show that the edge segments of
# tests/dvenc_edges.py notice); as they stand they are the statement ----
def mode_rule(d1, d2):
    """2-4-8 where neighbouring lines differ much more than lines two apart"""
    return d1 > 2 * d2 + 64


def clip_level(lv):
    return np.minimum(lv, 255)


def fits(total):
    """a segment's AC bits at a candidate quantisation number"""
    return total <= SEGMENT_AC_BITS


def most_bits(b):
    """the block of a segment (its 30 bit counts) that the overflow rule takes a level from: the first with the most"""
    return b.index(max(b))


def shift_of(qno, cls):
    """the quantiser shift per scan position: [..., 64] for arrays qno, cls of one shape"""
    return QUANT_SHIFT[np.asarray(qno) + CLASS_OFFSET[np.asarray(cls)]][..., AREA] + (np.asarray(cls) == 3)[..., None]


def _mul(x, c):
    return (x * c + 2048) >> 12


def _fdct8(x):
    """the scaled 8-point forward butterfly along the last axis"""
    t0, t7 = x[..., 0] + x[..., 7], x[..., 0] - x[..., 7]
    t1, t6 = x[..., 1] + x[..., 6], x[..., 1] - x[..., 6]
    t2, t5 = x[..., 2] + x[..., 5], x[..., 2] - x[..., 5]
    t3, t4 = x[..., 3] + x[..., 4], x[..., 3] - x[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    z1 = _mul(t12 + t13, C707)
    o = [None] * 8
    o[0], o[4], o[2], o[6] = t10 + t11, t10 - t11, t13 + z1, t13 - z1
    t10, t11, t12 = t4 + t5, t5 + t6, t6 + t7
    z5 = _mul(t10 - t12, C383)
    z2, z4, z3 = _mul(t10, C541) + z5, _mul(t12, C1307) + z5, _mul(t11, C707)
    z11, z13 = t7 + z3, t7 - z3
    o[5], o[3], o[1], o[7] = z13 + z2, z13 - z2, z11 + z4, z11 - z4
    return np.stack(o, -1)


def _fdct4(x):
    """its even half on four values"""
    t10, t13, t11, t12 = x[..., 0] + x[..., 3], x[..., 0] - x[..., 3], x[..., 1] + x[..., 2], x[..., 1] - x[..., 2]
    z1 = _mul(t12 + t13, C707)
    return np.stack([t10 + t11, t13 + z1, t10 - t11, t13 - z1], -1)


def choose_mode(px, flags):
    """px: [n][64] pixels 0..255 -> the transform mode of each block"""
    p = px.reshape(-1, 8, 8).astype(np.int64)
    d1 = np.abs(p[:, 0:6] - p[:, 1:7]).sum(axis=(1, 2))
    d2 = np.abs(p[:, 0:6] - p[:, 2:8]).sum(axis=(1, 2))
    return (mode_rule(d1, d2) & bool(flags & 1)).astype(np.int64)


def transform(px, mode):
    """[n][64] pixels, [n] modes -> [n][64] coefficients in natural order (row r = vertical frequency; 2-4-8: rows 2v / 2v + 1
    the sums' / the differences' frequency v)"""
    x = (px.reshape(-1, 8, 8).astype(np.int64) - 128) * 8
    t = np.swapaxes(_fdct8(x), 1, 2)  # [n][h][line]
    c88 = _fdct8(t)
    c248 = np.empty_like(t)
    c248[..., 0::2] = _fdct4(t[..., 0::2] + t[..., 1::2])
    c248[..., 1::2] = _fdct4(t[..., 0::2] - t[..., 1::2])
    c = np.where(np.asarray(mode)[:, None, None] != 0, c248, c88)
    return np.swapaxes(c, 1, 2).reshape(-1, 64)


def products(c, mode):
    """P[n][64] in scan order (P[:, 0] unused) and the signs"""
    mode = np.asarray(mode)
    cs = np.take_along_axis(c, SCAN[mode], axis=1)
    P = np.abs(cs) * MULT[mode]
    assert P.max() < (1 << 31) - (1 << 25)
    return P, cs < 0


def choose_class(P, flags):
    big = P[:, 1:].max(axis=1) >> FRAC
    cls = (big >= CLASS_LIMITS[0]).astype(np.int64) + (big >= CLASS_LIMITS[1]) + (big >= CLASS_LIMITS[2])
    return cls if flags & 2 else np.zeros_like(cls)


def quantise(P, neg, cls, qno):
    """signed levels [n][64] (scan order, [:, 0] = 0) at quantisation number qno ([n] or scalar)"""
    n = FRAC + shift_of(np.broadcast_to(qno, np.shape(cls)), cls)
    lv = clip_level((P + (1 << (n - 1))) >> n)
    lv[:, 0] = 0
    return np.where(neg, -lv, lv)


def word_lengths(levels):
    """[n][64]: at every non-zero level the bits of its word or words, sign included; 0 elsewhere"""
    a = np.abs(levels)
    k = np.arange(64)
    prev = np.maximum.accumulate(np.where(a != 0, k, 0), axis=1)
    prev = np.concatenate([np.zeros((a.shape[0], 1), np.int64), prev[:, :-1]], axis=1)  # the last non-zero position before k
    run = np.clip(k - prev - 1, 0, 62)
    return np.where(a != 0, PAIR_LEN[run, a] + 1, 0), run


def block_bits(levels):
    """AC bits of each block, the end of block included"""
    return word_lengths(np.asarray(levels).reshape(-1, 64))[0].sum(axis=1) + EOB[1]


def _bit_arrays(levels):
    """the code words of every block as arrays of bits"""
    n = levels.shape[0]
    ln, run = word_lengths(levels)
    b, k = np.nonzero(levels)
    a = np.abs(levels[b, k])
    val = (PAIR_VAL[run[b, k], a] << 1) | (levels[b, k] < 0)
    wl = ln[b, k]
    # the end of block behind each block's words: order by (block, position), position 64 for the end of block
    blk = np.concatenate([b, np.arange(n)])
    pos = np.concatenate([k, np.full(n, 64)])
    val = np.concatenate([val, np.full(n, EOB[0])])
    wl = np.concatenate([wl, np.full(n, EOB[1])])
    order = np.lexsort((pos, blk))
    blk, val, wl = blk[order], val[order], wl[order]
    w = np.repeat(np.arange(wl.size), wl)
    first = np.repeat(np.cumsum(wl) - wl, wl)
    i = np.arange(w.size) - first                    # bit i of its word, most significant first
    bits = ((val[w] >> (wl[w] - 1 - i)) & 1).astype(np.uint8)
    per_block = np.bincount(blk, weights=wl, minlength=n).astype(np.int64)
    return np.split(bits, np.cumsum(per_block)[:-1])


def encode_blocks(px, flags):
    """[30 s][64] pixels of s video segments -> dict: mode, cls, dc [30 s], qno [s], levels [30 s][64] (scan order),
    dropped [s] (levels the overflow rule took)"""
    px = np.asarray(px).reshape(-1, 64)
    assert px.shape[0] % 30 == 0 and 0 <= flags <= 3
    s = px.shape[0] // 30
    mode = choose_mode(px, flags)
    c = transform(px, mode)
    dc = np.clip((c[:, 0] + 128) >> 8, -256, 255)
    P, neg = products(c, mode)
    cls = choose_class(P, flags)
    qno = np.zeros(s, np.int64)
    undecided = np.ones(s, bool)
    levels = np.zeros((30 * s, 64), np.int64)
    for q in range(15, -1, -1):
        if not undecided.any():
            break
        rows = np.repeat(undecided, 30)
        lv = quantise(P[rows], neg[rows], cls[rows], q)
        fit = fits(block_bits(lv).reshape(-1, 30).sum(axis=1))
        if q == 0:
            fit[:] = True  # what does not fit at 0 goes on to the overflow rule
        idx = np.flatnonzero(undecided)[fit]
        lv = lv.reshape(-1, 30, 64)[fit]
        for i, one in zip(idx, lv):
            levels[30 * i:30 * i + 30] = one
        qno[idx] = q
        undecided[idx] = False
    dropped = np.zeros(s, np.int64)
    bits = block_bits(levels).reshape(s, 30)
    for i in np.flatnonzero(bits.sum(axis=1) > SEGMENT_AC_BITS):
        lv = levels[30 * i:30 * i + 30]
        wl = word_lengths(lv)[0]
        b = [int(x) for x in bits[i]]
        total = sum(b)
        steps = 0
        while total > SEGMENT_AC_BITS:
            assert steps < 30 * 63
            j = most_bits(b)                         # the first block with the most bits
            last = int(np.flatnonzero(lv[j])[-1])
            lv[j, last] = 0
            b[j] -= int(wl[j, last])
            total -= int(wl[j, last])
            steps += 1
        dropped[i] = steps
    return {"mode": mode, "cls": cls, "dc": dc, "qno": qno, "levels": levels, "dropped": dropped}


AREA_OFF = (4, 18, 32, 46, 60, 70)
AREA_BITS = (112, 112, 112, 112, 80, 80)


def pack_segment(dc, mode, cls, qno, bits):
    """30 block headers and bit arrays -> the segment's five DIF blocks [5][80] (bytes 0..2, the ids, are zero)"""
    seg = np.zeros(5 * 640, np.uint8)
    used = [0] * 30
    vfree = []
    for m in range(5):
        free = []
        for j in range(6):
            i, p0 = 6 * m + j, 640 * m + 8 * AREA_OFF[j]
            hd = ((int(dc[i]) & 511) << 3) | (int(mode[i]) << 2) | int(cls[i])
            seg[p0:p0 + 12] = [(hd >> (11 - t)) & 1 for t in range(12)]
            cap = AREA_BITS[j] - 12
            n = min(bits[i].size, cap)
            seg[p0 + 12:p0 + 12 + n] = bits[i][:n]
            used[i] = n
            free.append(np.arange(p0 + 12 + n, p0 + 12 + cap))
        free = np.concatenate(free)
        at = 0
        for i in range(6 * m, 6 * m + 6):  # pass 2
            n = min(bits[i].size - used[i], free.size - at)
            seg[free[at:at + n]] = bits[i][used[i]:used[i] + n]
            used[i] += n
            at += n
        vfree.append(free[at:])
    vfree = np.concatenate(vfree)
    at = 0
    for i in range(30):  # pass 3
        n = min(bits[i].size - used[i], vfree.size - at)
        seg[vfree[at:at + n]] = bits[i][used[i]:used[i] + n]
        used[i] += n
        at += n
    assert all(used[i] == bits[i].size for i in range(30)), "the rate control keeps a segment within its areas"
    out = np.packbits(seg).reshape(5, 80)
    out[:, 3] = qno  # STA 0
    return out


def segment(px, flags):
    """THE UNIT: 30 blocks of 64 pixels (macroblock-major, Y0 Y1 Y2 Y3 Cr Cb) -> five DIF blocks [5][80] without ids"""
    r = encode_blocks(px, flags)
    return pack_segment(r["dc"], r["mode"], r["cls"], int(r["qno"][0]), _bit_arrays(r["levels"]))


_BLOCK_MAP = None


def block_map():
    """picture offsets [8100][64] of the 525/60 blocks, block ((seq 27 + slot) 5 + m) 6 + j"""
    global _BLOCK_MAP
    if _BLOCK_MAP is None:
        idx = np.zeros((SEGMENTS * 30, 64), np.int64)
        for s in range(SEGMENTS):
            for m in range(5):
                x, y = S.mb_place(S.SYS_525_60, s // 27, s % 27, m)
                for j in range(6):
                    idx[(5 * s + m) * 6 + j] = S.block411(x, y, j, D.W, D.H, D.CW)
        _BLOCK_MAP = idx
    return _BLOCK_MAP


def encode525(pic, flags=3, record=None):
    """one 525/60 picture -> one DIF frame; every byte outside the video segments as dvo_encode_frame writes it.  record: a
    dict that receives what the statement chose (encode_blocks' result; qno per segment)"""
    pic = np.ascontiguousarray(pic, np.uint8).reshape(D.PICTURE_BYTES)
    r = encode_blocks(pic[block_map()], flags)
    if record is not None:
        record.update(r)
    bits = _bit_arrays(r["levels"])
    f = np.zeros((10, 150, 80), np.uint8)
    for b in range(150):  # block ids: section type, sequence, number within the section
        if b == 0:
            sct, num = 0, 0
        elif b < 3:
            sct, num = 1, b - 1
        elif b < 6:
            sct, num = 2, b - 3
        elif (b - 6) % 16 == 0:
            sct, num = 3, (b - 6) // 16
        else:
            sct, num = 4, (b - 6) - (b - 6) // 16 - 1
        f[:, b, 0], f[:, b, 1], f[:, b, 2] = (sct << 5) | 0x1F, (np.arange(10) << 4) | 0x07, num
    f[:, 0, 3] = 0x3F  # DSF 0
    frame = f.reshape(-1)
    for s in range(SEGMENTS):
        blk = pack_segment(r["dc"][30 * s:], r["mode"][30 * s:], r["cls"][30 * s:], int(r["qno"][s]), bits[30 * s:30 * s + 30])
        for m in range(5):
            o = D.video_block_offset(s // 27, 5 * (s % 27) + m)
            frame[o + 3:o + 80] = blk[m, 3:]
    return frame


def encode(system, pic, flags=3, record=None):
    """any system's picture -> its frame (dvsys.encode around encode525).  record: a list that receives one encode525 record
    per carrier frame"""
    def one(p, fl):
        rec = {}
        fr = encode525(p, fl, rec)
        if record is not None:
            record.append(rec)
        return fr
    return S.encode(system, pic, flags, encode525=one)


def drop_picture(system):
    """THE DROP-RULE PICTURE of a system: dvsys.synth(system, 0, 1, 8) with uniformly random bytes (seed 7) in every second
    band of 48 lines of Y (lines 0..47, 96..143, ...; in 4:2:2 of Cb and Cr too).  A band is a row of super blocks (two rows in 4:2:2), and the shuffle
    takes all five macroblocks of a segment from rows of one parity: the segments of every second DIF sequence are all
    noise, do not fit at quantisation number 0 and lose levels; the others hold no noise and lose none"""
    g = S.geometry(system)
    pic = S.synth(system, 0, 1, 8).copy()
    y = pic[:g.w * g.h].reshape(g.h, g.w)
    loud = (np.arange(g.h) // 48) % 2 == 0
    rng = np.random.default_rng(7)
    y[loud] = rng.integers(0, 256, (int(loud.sum()), g.w), dtype=np.uint8)
    if g.chans == 2:  # 4:2:2 codes two luma blocks a macroblock: the chroma planes, as high as the picture, take noise too
        c = pic[g.w * g.h:].reshape(2, g.h, g.cw)
        c[:, loud] = rng.integers(0, 256, (2, int(loud.sum()), g.cw), dtype=np.uint8)
    return pic


PICTURES = ("flat", "n8", "n64", "drop")  # what the CPU and the GPU tests encode, in every system


def picture(system, which):
    """dvsys.synth pictures at noise 0, 8 and 64, and the drop-rule picture"""
    if which == "drop":
        return drop_picture(system)
    return S.synth(system, 0, 1, {"flat": 0, "n8": 8, "n64": 64}[which])


_STATED = {}


def stated(system, which, flags):
    """(the statement's frame of picture(system, which), its qno histogram, its dropped levels), made once"""
    key = (system, which, flags)
    if key not in _STATED:
        rec = []
        fr = encode(system, picture(system, which), flags, rec)
        fr.setflags(write=False)
        _STATED[key] = (fr,) + census(system, rec)
    return _STATED[key]


def census(system, records):
    """(qno histogram [16], dropped levels) of a system's frame from its carrier records: the carriers' first segments"""
    n = S.geometry(system).segments
    qno = np.concatenate([r["qno"] for r in records])[:n]
    dropped = np.concatenate([r["dropped"] for r in records])[:n]
    return np.bincount(qno, minlength=16), int(dropped.sum())
