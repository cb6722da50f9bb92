"""Test statement of the two 50 Mbit/s 4:2:2 DV systems ("DVCPRO50": 525/60 and 625/50) on top of the unchanged 525/60
oracle (oracle/libdv_oracle.so through dvlib), in the manner of tests/dv625.py.  TEST INFRASTRUCTURE ONLY: the product
never imports it.  PARITY UNPINNED, like the oracle itself: the layout below is this repository's reading of SMPTE 314M.

The codec is the 25 Mbit/s one: the same 80-byte compressed macroblock of six areas, the same three passes, and in
oracle/dv_oracle.c a video segment's 30 block pictures depend on that segment's five DIF blocks alone.  So a 4:2:2 frame
is decoded by copying its 540 / 648 video segments into the segment slots of two / three 525/60 frames, decoding those
with the oracle, and moving the 64 pixels of areas 0, 2, 4 and 5 of every macroblock from their 525/60 place to their
4:2:2 place; the pixels of areas 1 and 3, which carry none in these systems, are dropped (their bits took part in all
three passes inside the oracle like any block's).  Encoding is the reverse with areas 1 and 3 of the carrier pictures
flat 128 — which the oracle's encoder writes as DC 0 and an end-of-block — followed by the header.

The layout is written here independently of the kernels' statement of it (csrc/dv_common.h, Sys422): two DIF channels
back to back, each of SEQS sequences (10 / 12) of 150 blocks; macroblocks of 16 x 8 pixels, 45 x 60 / 45 x 72 of them, in
5 columns x 2 SEQS rows of super blocks of 9 x 3; macroblock m of segment `slot` of sequence `seq` of channel `chan` in
super block (row 2 ((seq + (2, 6, 8, 0, 4)[m]) mod SEQS) + chan, column (2, 1, 3, 0, 4)[m]), inside it at column
slot // 3 and row slot % 3 (2 - slot % 3 in odd columns); area 0 the left luma block, area 2 the right one, area 4 Cr,
area 5 Cb, the chroma planes 360 wide and as high as the picture."""
import numpy as np

import dvlib as D

SYS_525_60_422, SYS_625_50_422 = 4, 5  # VAUX stype 4 | DSF
SYSTEMS = (SYS_525_60_422, SYS_625_50_422)
W, CW = 720, 360
SHOWN = (0, 2, 4, 5)  # the areas of a compressed macroblock that carry pixels


class Geometry:
    def __init__(self, system):
        assert system in SYSTEMS, system
        self.system = system
        self.dsf = system & 1
        self.seqs = 12 if self.dsf else 10           # per channel
        self.frame_seqs = 2 * self.seqs              # of the frame, in byte order
        self.frame_bytes = self.frame_seqs * 150 * 80
        self.segments = self.frame_seqs * 27
        self.h = 576 if self.dsf else 480
        self.picture_bytes = W * self.h + 2 * CW * self.h
        self.hosts = -(-self.segments // 270)        # 525/60 frames that carry the segments: 2 (540) / 3 (648)


_GEO = {s: Geometry(s) for s in SYSTEMS}


def geometry(system):
    return _GEO[system]


def mb_place(system, seq, slot, m):
    """(x, y) of a macroblock in 16-pixel columns and 8-line rows; seq counts the frame's sequences, 0 .. 2 SEQS - 1"""
    g = _GEO[system]
    chan, s = divmod(seq, g.seqs)
    col = (2, 1, 3, 0, 4)[m]
    row = (s + (2, 6, 8, 0, 4)[m]) % g.seqs
    c, r = divmod(slot, 3)
    return 9 * col + c, 3 * (2 * row + chan) + (2 - r if c % 2 else r)


def _block_422(g, x, y, j):
    """picture offsets of the 64 pixels (row major) of area j (0, 2, 4 or 5) of the macroblock at (x, y)"""
    rr, cc = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    if j < 4:
        return ((8 * y + rr) * W + 16 * x + 8 * (j // 2) + cc).ravel()
    base = W * g.h + (CW * g.h if j == 4 else 0)  # area 4 is Cr (third plane), area 5 Cb
    return (base + (8 * y + rr) * CW + 8 * x + cc).ravel()


def _block_525(x, y, j):
    """the same for block j of a 525/60 macroblock at (x, y) of dvo_mb_place (32-pixel columns, 8-line rows; column 22
    holds 16 x 16 macroblocks whose chroma blocks are split: left half in rows 0-7, right half in the eight rows below)"""
    rr, cc = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    if j < 4:
        if x < 22:
            return ((8 * y + rr) * D.W + 32 * x + 8 * j + cc).ravel()
        return ((8 * y + 8 * (j >> 1) + rr) * D.W + 32 * x + 8 * (j & 1) + cc).ravel()
    base = D.W * D.H + (D.CW * D.H if j == 4 else 0)
    if x < 22:
        return (base + (8 * y + rr) * D.CW + 8 * x + cc).ravel()
    return (base + (8 * y + rr + 8 * (cc >= 4)) * D.CW + 8 * x + (cc & 3)).ravel()


def _maps(g):
    import ctypes as C
    L = D.lib()
    src, dst, blocks422, blocks525 = [], [], [], []
    for S in range(g.segments):
        seq, slot = divmod(S, 27)
        host, s5 = divmod(S, 270)
        seq5, slot5 = divmod(s5, 27)
        for m in range(5):
            v, v5 = 5 * slot + m, 5 * slot5 + m
            blocks422.append(D.video_block_offset(seq, v))
            blocks525.append(host * D.FRAME_BYTES + D.video_block_offset(seq5, v5))
            x, y = mb_place(g.system, seq, slot, m)
            x5, y5 = C.c_int(), C.c_int()
            L.dvo_mb_place(seq5, slot5, m, C.byref(x5), C.byref(y5))
            for j in SHOWN:
                dst.append(_block_422(g, x, y, j))
                src.append(host * D.PICTURE_BYTES + _block_525(x5.value, y5.value, j))
    src, dst = np.concatenate(src), np.concatenate(dst)
    b422 = (np.array(blocks422)[:, None] + np.arange(80)).ravel()
    b525 = (np.array(blocks525)[:, None] + np.arange(80)).ravel()
    return src, dst, b422, b525


_MAPS = {}


def maps(system):
    """(pixel offsets in the carrier 525/60 pictures, the same pixels' offsets in the 4:2:2 picture, DIF-block bytes of
    the 4:2:2 frame's video segments, the same bytes in the carrier 525/60 frames)"""
    if system not in _MAPS:
        g = _GEO[system]
        m = _maps(g)
        src, dst, b422, b525 = m
        assert np.array_equal(np.sort(dst), np.arange(g.picture_bytes)), "4:2:2 blocks must tile the picture exactly once"
        assert np.unique(src).size == src.size
        assert np.unique(b422).size == b422.size and b422.max() < g.frame_bytes
        _MAPS[system] = m
    return _MAPS[system]


def decode(system, frame, decode525=None):
    """one 4:2:2 DIF frame (any 240,000 / 288,000 bytes) -> one picture (Y 720 x H, Cb 360 x H, Cr 360 x H).
    decode525: the 525/60 frame decoder the segments go through (default: the oracle's)"""
    decode525 = decode525 or D.decode
    g = _GEO[system]
    src, dst, b422, b525 = maps(system)
    frame = np.ascontiguousarray(frame, np.uint8).reshape(g.frame_bytes)
    hosts = np.zeros(g.hosts * D.FRAME_BYTES, np.uint8)
    hosts[b525] = frame[b422]
    pics = np.concatenate([decode525(hosts[i * D.FRAME_BYTES:(i + 1) * D.FRAME_BYTES]) for i in range(g.hosts)])
    pic = np.empty(g.picture_bytes, pics.dtype)
    pic[dst] = pics[src]
    return pic


def header(system, frame):
    """block ids of both channels' sequences (with the channel bit) and the header block's profile bits (the system's
    DSF, VAUX stype 4), in place"""
    g = _GEO[system]
    f = frame.reshape(g.frame_seqs, 150, 80)
    for fs in range(g.frame_seqs):
        chan, seq = divmod(fs, g.seqs)
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
            f[fs, b, :3] = ((sct << 5) | 0x1F, (seq << 4) | (chan << 3) | 0x07, num)
        f[fs, 0, 3] = 0xBF if g.dsf else 0x3F  # DSF
        f[fs, 0, 5] = (f[fs, 0, 5] & 0xF8) | 1  # APT 1
        f[fs, 5, 48 + 3] = (f[fs, 5, 48 + 3] & 0xE0) | 0x04  # VAUX source pack: stype 4 (the first one is what is read)
    return frame


def pack(system, hosts):
    """the carrier 525/60 DIF frames -> the 4:2:2 frame that holds their first 540 / 648 video segments"""
    g = _GEO[system]
    _, _, b422, b525 = maps(system)
    frame = np.zeros(g.frame_bytes, np.uint8)
    frame[b422] = np.ascontiguousarray(hosts, np.uint8).reshape(g.hosts * D.FRAME_BYTES)[b525]
    return header(system, frame)


def encode(system, pic, flags=3, encode525=None):
    """one 4:2:2 picture -> one DIF frame (the oracle's encoder on every segment, flags as dvo_encode_frame's; areas 1
    and 3 of every carrier macroblock are flat 128).  encode525: another 525/60 encoder (picture, flags) -> frame whose
    rate control is per segment too"""
    encode525 = encode525 or D.encode
    g = _GEO[system]
    src, dst, _, _ = maps(system)
    pic = np.ascontiguousarray(pic, np.uint8).reshape(g.picture_bytes)
    pics = np.full(g.hosts * D.PICTURE_BYTES, 128, np.uint8)
    pics[src] = pic[dst]
    return pack(system, np.concatenate([encode525(pics[i * D.PICTURE_BYTES:(i + 1) * D.PICTURE_BYTES], flags)
                                        for i in range(g.hosts)]))


def synth422(system, n, seed=1, amp=8):
    """picture n of a seeded sequence: a smooth gradient, noise of amplitude amp, a few hard edges and a combed band
    (the odd field moved) so that both transform modes and every class occur"""
    g = _GEO[system]
    H = g.h
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    h = (x * 0x9E3779B1) ^ (y * 0x85EBCA77) ^ (n * 0xC2B2AE3D) ^ (seed * 0x27D4EB2F) ^ (system * 0x165667B1)
    h &= 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & 0xFFFFFFFF
    h ^= h >> 12
    h = (h * 0x297A2D39) & 0xFFFFFFFF
    h ^= h >> 15
    xs = np.where((y >= 200) & (y < 280) & (y % 2 == 1), x + 12, x)
    v = 16 + ((xs + y + 7 * n) % 1300) * 219 // 1300
    v = np.where(((xs // 48) + (y // 40)) % 5 == 0, 235 - v // 2, v)
    if amp:
        v = v + (h % (2 * amp + 1)).astype(np.int64) - amp
    Y = np.clip(v, 0, 255).astype(np.uint8)
    cy, cx = np.mgrid[0:H, 0:CW].astype(np.int64)
    hc = h[:, 0:W:2]
    nz = ((hc >> 16) % (amp + 1)).astype(np.int64) - amp // 2 if amp else 0
    comb = np.where((cy >= 200) & (cy < 280) & (cy % 2 == 1), 9, 0)  # the chroma planes have both fields too
    cb = np.clip(128 + (cx - 180) // 3 + comb + nz // 2, 0, 255).astype(np.uint8)
    cr = np.clip(128 - (cy - H // 2) // 4 - comb + nz // 2, 0, 255).astype(np.uint8)
    return np.concatenate([Y.ravel(), cb.ravel(), cr.ravel()])
