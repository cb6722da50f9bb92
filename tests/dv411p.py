"""Test statement of DVCPRO 625/50 4:1:1 (25 Mbit/s PAL: DSF 1, VAUX stype 0, APT != 0) on top of the unchanged 525/60
oracle (oracle/libdv_oracle.so through dvlib), in the manner of tests/dv625.py.  TEST INFRASTRUCTURE ONLY: the product
never imports it.  PARITY UNPINNED, like the oracle itself: the layout below is this repository's reading of SMPTE 314M,
written from memory, and the least certain of the five.

The codec is the 25 Mbit/s one, and in oracle/dv_oracle.c a video segment's 30 block pictures depend on that segment's
five DIF blocks alone.  So a frame is decoded by moving its 324 segments into the video-segment slots of two 525/60
frames (270 + 54), decoding those with the oracle, and moving every block's 64 pixels from its 525/60 place to its place
here; encoding is the same in reverse, followed by the header.  Both ends are 4:1:1, so a right-edge chroma block, which
is split in halves at either end, maps half to half.

The layout is written here independently of the kernels' statement of it (csrc/dv_common.h, Sys625_411): the 625/50
frame of 12 DIF sequences of 150 blocks; Y 720 x 576, Cb and Cr 180 x 576, tightly packed.  The picture is 12 rows
(48 lines each) x 5 columns of super blocks of 27 macroblocks; macroblock m of segment `slot` of sequence `seq` lies in
super block (row (seq + (2, 6, 8, 0, 4)[m]) mod 12, column (2, 1, 3, 0, 4)[m]).  Macroblocks are 32 x 8 pixels (four luma
blocks side by side, one 8 x 8 block of each chroma plane), six to a 32-pixel column of a super block, walked downwards in
even columns and upwards in odd ones; the super-block columns begin at 32-pixel columns 0, 4 1/2, 9, 13 1/2 and 18 (the
second and the fourth begin half-way down a column), and the last one ends with column 22 (pixels 704..719), where the
macroblocks are 16 x 16 (Y0 Y1 / Y2 Y3), three to the column, and their chroma blocks are split: the left 4 x 8 half in
the upper eight lines, the right half in the eight lines below.  Block 4 is Cr (the third plane), block 5 Cb."""
import numpy as np

import dvlib as D

SYS_625_50_411 = 3
FRAME_BYTES, W, H, CW, CH = 144000, 720, 576, 180, 576
PICTURE_BYTES = W * H + 2 * CW * CH  # 622,080
SEQS = 12
SEGMENTS = SEQS * 27  # 324
MACROBLOCKS = SEGMENTS * 5  # 1,620
HOSTS = 2             # 525/60 frames that carry one frame's segments (270 + 54)
APT = 1               # what encode() announces (any value but 0 marks the profile)


def mb_place(seq, slot, m):
    """(x, y) of a macroblock: x in 32-pixel columns (0..22), y in 8-line rows (0..71); a column-22 macroblock is 16 x 16"""
    col = (2, 1, 3, 0, 4)[m]
    row = (seq + (2, 6, 8, 0, 4)[m]) % SEQS
    k = slot + (3 if col in (1, 3) else 0)  # these super-block columns begin in the middle of a 32-pixel column
    c, r = divmod(k, 6)
    if c % 2:
        r = 5 - r
    x = (0, 4, 9, 13, 18)[col] + c
    return x, 6 * row + (2 * r if x == 22 else r)


def _block(x, y, j, w, h, cw):
    """picture offsets of the 64 pixels (row major) of block j of the macroblock at (x, y) in a 4:1:1 picture of luma
    width w, height h and chroma width cw (32-pixel columns, 8-line rows; column 22 holds 16 x 16 macroblocks whose chroma
    blocks are split: left half in rows 0-7, right half in the eight rows below)"""
    rr, cc = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    if j < 4:
        if x < 22:
            return ((8 * y + rr) * w + 32 * x + 8 * j + cc).ravel()
        return ((8 * y + 8 * (j >> 1) + rr) * w + 32 * x + 8 * (j & 1) + cc).ravel()
    base = w * h + (cw * h if j == 4 else 0)  # block 4 is Cr (third plane), block 5 Cb
    if x < 22:
        return (base + (8 * y + rr) * cw + 8 * x + cc).ravel()
    return (base + (8 * y + rr + 8 * (cc >= 4)) * cw + 8 * x + (cc & 3)).ravel()


def _maps():
    import ctypes as C
    L = D.lib()
    src, dst, blocks_here, blocks525 = [], [], [], []
    for S in range(SEGMENTS):
        seq, slot = divmod(S, 27)
        host, s5 = divmod(S, 270)
        seq5, slot5 = divmod(s5, 27)
        for m in range(5):
            v, v5 = 5 * slot + m, 5 * slot5 + m
            blocks_here.append(D.video_block_offset(seq, v))
            blocks525.append(host * D.FRAME_BYTES + D.video_block_offset(seq5, v5))
            x, y = mb_place(seq, slot, m)
            x5, y5 = C.c_int(), C.c_int()
            L.dvo_mb_place(seq5, slot5, m, C.byref(x5), C.byref(y5))
            # a 16 x 16 macroblock moves to a 16 x 16 place and a 32 x 8 one to a 32 x 8 place only if the two shuffles
            # put the same macroblocks into column 22; they do (the column is a function of slot and m alone)
            assert (x == 22) == (x5.value == 22), (seq, slot, m)
            for j in range(6):
                dst.append(_block(x, y, j, W, H, CW))
                src.append(host * D.PICTURE_BYTES + _block(x5.value, y5.value, j, D.W, D.H, D.CW))
    src, dst = np.concatenate(src), np.concatenate(dst)
    here = (np.array(blocks_here)[:, None] + np.arange(80)).ravel()
    b525 = (np.array(blocks525)[:, None] + np.arange(80)).ravel()
    return src, dst, here, b525


_MAPS = None


def maps():
    """(pixel offsets in two 525/60 pictures, the same pixels' offsets in the 625/50 4:1:1 picture, DIF-block bytes of the
    frame's video segments, the same bytes in two 525/60 frames)"""
    global _MAPS
    if _MAPS is None:
        m = _maps()
        src, dst, here, b525 = m
        assert np.array_equal(np.sort(dst), np.arange(PICTURE_BYTES)), "the blocks must tile the 622,080 bytes exactly once"
        assert np.unique(src).size == src.size
        assert np.unique(here).size == here.size and here.max() < FRAME_BYTES
        _MAPS = m
    return _MAPS


def decode(frame, decode525=None):
    """one DIF frame (any 144,000 bytes) -> one picture (Y 720 x 576, Cb 180 x 576, Cr 180 x 576).  decode525: the 525/60
    frame decoder the segments go through (default: the oracle's; the float statement's can be passed, whose pictures are
    doubles)"""
    decode525 = decode525 or D.decode
    src, dst, here, b525 = maps()
    frame = np.ascontiguousarray(frame, np.uint8).reshape(FRAME_BYTES)
    hosts = np.zeros(HOSTS * D.FRAME_BYTES, np.uint8)
    hosts[b525] = frame[here]
    pics = np.concatenate([decode525(hosts[i * D.FRAME_BYTES:(i + 1) * D.FRAME_BYTES]) for i in range(HOSTS)])
    pic = np.empty(PICTURE_BYTES, pics.dtype)
    pic[dst] = pics[src]
    return pic


def header(frame, apt=APT):
    """block ids of the 12 sequences and the header block's profile bits (DSF 1, APT `apt`, VAUX stype 0), in place"""
    assert 1 <= apt <= 7
    f = frame.reshape(SEQS, 150, 80)
    for seq in range(SEQS):
        for b in range(150):
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
            f[seq, b, :3] = ((sct << 5) | 0x1F, (seq << 4) | 0x07, num)
        f[seq, 0, 3] = 0xBF  # DSF = 1 (625/50)
        f[seq, 0, 5] = (f[seq, 0, 5] & 0xF8) | apt
    f[0, 5, 48 + 3] &= 0xE0  # VAUX source pack: stype 0
    return frame


def pack(hosts, apt=APT):
    """two 525/60 DIF frames (240,000 bytes) -> the 625/50 4:1:1 frame that carries their first 324 video segments"""
    _, _, here, b525 = maps()
    frame = np.zeros(FRAME_BYTES, np.uint8)
    frame[here] = np.ascontiguousarray(hosts, np.uint8).reshape(HOSTS * D.FRAME_BYTES)[b525]
    return header(frame, apt)


def encode(pic, flags=3, encode525=None, apt=APT):
    """one picture -> one DIF frame (the oracle's encoder on every segment, flags as dvo_encode_frame's), announcing
    DSF 1, APT 1, stype 0.  encode525: another 525/60 encoder (picture, flags) -> frame whose rate control is per segment
    too"""
    encode525 = encode525 or D.encode
    src, dst, _, _ = maps()
    pic = np.ascontiguousarray(pic, np.uint8).reshape(PICTURE_BYTES)
    pics = np.full(HOSTS * D.PICTURE_BYTES, 128, np.uint8)
    pics[src] = pic[dst]
    return pack(np.concatenate([encode525(pics[i * D.PICTURE_BYTES:(i + 1) * D.PICTURE_BYTES], flags) for i in range(HOSTS)]), apt)


def synth(n, seed=1, amp=8, region="all"):
    """picture n of a seeded sequence: a smooth gradient, noise of amplitude amp, a few hard edges and combed bands (the
    odd field moved) so that both transform modes and every class occur.  The detail reaches where this layout differs
    from 525/60: lines 480..575 (a second combed band, edges and noise down to the last line) and columns 704..719 (the
    16 x 16 macroblocks with split chroma), in the chroma planes too.  region: 'all'; 'bottom' keeps the detail of lines
    480..575 only and 'right' that of columns 704..719 only — everything else is flat (Y 128, Cb and Cr 128)"""
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    h = (x * 0x9E3779B1) ^ (y * 0x85EBCA77) ^ (n * 0xC2B2AE3D) ^ (seed * 0x27D4EB2F) ^ (SYS_625_50_411 * 0x165667B1)
    h &= 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & 0xFFFFFFFF
    h ^= h >> 12
    h = (h * 0x297A2D39) & 0xFFFFFFFF
    h ^= h >> 15
    combed = (((y >= 200) & (y < 280)) | ((y >= 500) & (y < 560))) & (y % 2 == 1)
    xs = np.where(combed, x + 12, x)
    v = 16 + ((xs + y + 7 * n) % 1300) * 219 // 1300
    v = np.where(((xs // 48) + (y // 40)) % 5 == 0, 235 - v // 2, v)
    v = np.where((x >= 704) & ((x + y // 4 + n) % 6 < 2), 250 - v // 3, v)  # edges inside the right-edge column
    if amp:
        v = v + (h % (2 * amp + 1)).astype(np.int64) - amp
    Y = np.clip(v, 0, 255).astype(np.uint8)
    cy, cx = np.mgrid[0:CH, 0:CW].astype(np.int64)
    hc = h[:, 0:W:4]
    nz = ((hc >> 16) % (amp + 1)).astype(np.int64) - amp // 2 if amp else 0
    comb = np.where(combed[:, 0:W:4], 9, 0)  # the chroma planes have both fields too
    edge = np.where((cx >= 176) & ((cx + cy // 8) % 3 == 0), 24, 0)  # ... and the split halves differ
    cb = np.clip(128 + (cx - 90) * 2 // 3 + comb + edge + nz // 2, 0, 255).astype(np.uint8)
    cr = np.clip(128 - (cy - H // 2) // 4 - comb - edge + nz // 2, 0, 255).astype(np.uint8)
    if region != "all":
        assert region in ("bottom", "right"), region
        keep_y = (y >= 480) if region == "bottom" else (x >= 704)
        keep_c = (cy >= 480) if region == "bottom" else (cx >= 176)
        Y, cb, cr = np.where(keep_y, Y, 128).astype(np.uint8), np.where(keep_c, cb, 128).astype(np.uint8), \
            np.where(keep_c, cr, 128).astype(np.uint8)
    return np.concatenate([Y.ravel(), cb.ravel(), cr.ravel()])
