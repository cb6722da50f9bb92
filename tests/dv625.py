"""Test statement of DV25 625/50 (IEC 4:2:0) on top of the unchanged 525/60 oracle (oracle/libdv_oracle.so through
dvlib).  TEST INFRASTRUCTURE ONLY: the product never imports it.  PARITY UNPINNED, like the oracle itself.

In oracle/dv_oracle.c a video segment's 30 block pictures depend on that segment's five DIF blocks alone, and the
encoder's rate control is per segment too.  So a 625/50 frame is decoded by moving its 324 segments into the
video-segment slots of two 525/60 frames (270 + 54), decoding those with the oracle, and moving every block's 64 pixels
from its 525/60 place to its 625/50 place; encoding is the same in reverse.

The 625/50 layout is written here from the published format, independently of the kernels' statement of it
(csrc/dv_common.h, Sys625): 12 DIF sequences; 45 x 36 macroblocks of 16 x 16 in 5 x 12 super blocks of 9 x 3;
macroblock m of segment `slot` of sequence `seq` in super block (row (seq + (2, 6, 8, 0, 4)[m]) mod 12,
column (2, 1, 3, 0, 4)[m]), inside it at column slot // 3 and row slot % 3 (2 - slot % 3 in odd columns); blocks
Y0 Y1 / Y2 Y3, then Cr (block 4) and Cb (block 5) as plain 8 x 8 blocks of the 360 x 288 chroma planes."""
import numpy as np

import dvlib as D

FRAME_BYTES, W, H, CW, CH = 144000, 720, 576, 360, 288
PICTURE_BYTES = W * H + 2 * CW * CH
SEQS = 12
SEGMENTS = SEQS * 27  # 324
HOSTS = 2             # 525/60 frames that carry one 625/50 frame's segments (270 + 54)


def mb_place(seq, slot, m):
    """(x, y) of a 625/50 macroblock in 16 x 16 units"""
    col = (2, 1, 3, 0, 4)[m]
    row = (seq + (2, 6, 8, 0, 4)[m]) % 12
    c, r = divmod(slot, 3)
    return 9 * col + c, 3 * row + (2 - r if c % 2 else r)


def _block_625(x, y, j):
    """picture offsets of the 64 pixels (row major) of block j of the macroblock at (x, y)"""
    rr, cc = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    if j < 4:
        return ((16 * y + 8 * (j >> 1) + rr) * W + 16 * x + 8 * (j & 1) + cc).ravel()
    base = W * H + (CW * CH if j == 4 else 0)  # block 4 is Cr (third plane), block 5 Cb
    return (base + (8 * y + rr) * CW + 8 * x + cc).ravel()


def _block_525(x, y, j):
    """the same for a 525/60 macroblock at (x, y) of dvo_mb_place (32-pixel columns, 8-line rows; column 22 holds
    16 x 16 macroblocks whose chroma blocks are split: left half in rows 0-7, right half in the eight rows below)"""
    rr, cc = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    if j < 4:
        if x < 22:
            return ((8 * y + rr) * D.W + 32 * x + 8 * j + cc).ravel()
        return ((8 * y + 8 * (j >> 1) + rr) * D.W + 32 * x + 8 * (j & 1) + cc).ravel()
    base = D.W * D.H + (D.CW * D.H if j == 4 else 0)
    if x < 22:
        return (base + (8 * y + rr) * D.CW + 8 * x + cc).ravel()
    return (base + (8 * y + rr + 8 * (cc >= 4)) * D.CW + 8 * x + (cc & 3)).ravel()


def _maps():
    import ctypes as C
    L = D.lib()
    src, dst = [], []
    blocks625, blocks525 = [], []
    for S in range(SEGMENTS):
        seq, slot = divmod(S, 27)
        host, s5 = divmod(S, 270)
        seq5, slot5 = divmod(s5, 27)
        for m in range(5):
            v, v5 = 5 * slot + m, 5 * slot5 + m
            blocks625.append(D.video_block_offset(seq, v))
            blocks525.append(host * D.FRAME_BYTES + D.video_block_offset(seq5, v5))
            x, y = mb_place(seq, slot, m)
            x5, y5 = C.c_int(), C.c_int()
            L.dvo_mb_place(seq5, slot5, m, C.byref(x5), C.byref(y5))
            for j in range(6):
                dst.append(_block_625(x, y, j))
                src.append(host * D.PICTURE_BYTES + _block_525(x5.value, y5.value, j))
    src, dst = np.concatenate(src), np.concatenate(dst)
    b625 = (np.array(blocks625)[:, None] + np.arange(80)).ravel()
    b525 = (np.array(blocks525)[:, None] + np.arange(80)).ravel()
    return src, dst, b625, b525


_MAPS = None


def maps():
    """(pixel offsets in two 525/60 pictures, the same pixels' offsets in the 625/50 picture, DIF-block bytes of the
    625/50 frame's video segments, the same bytes in two 525/60 frames)"""
    global _MAPS
    if _MAPS is None:
        _MAPS = _maps()
        src, dst = _MAPS[0], _MAPS[1]
        assert np.array_equal(np.sort(dst), np.arange(PICTURE_BYTES)), "625/50 blocks must tile the picture"
        assert np.unique(src).size == src.size
    return _MAPS


def decode(frame, decode525=None):
    """one 625/50 DIF frame (any 144,000 bytes) -> one picture (Y 720x576, Cb 360x288, Cr 360x288).  decode525: the
    525/60 frame decoder the segments go through (default: the oracle's; tests/dvfloat.py passes the float statement's,
    whose pictures are doubles)"""
    decode525 = decode525 or D.decode
    src, dst, b625, b525 = maps()
    frame = np.ascontiguousarray(frame, np.uint8).reshape(FRAME_BYTES)
    hosts = np.zeros(HOSTS * D.FRAME_BYTES, np.uint8)
    hosts[b525] = frame[b625]
    pics = np.concatenate([decode525(hosts[i * D.FRAME_BYTES:(i + 1) * D.FRAME_BYTES]) for i in range(HOSTS)])
    pic = np.empty(PICTURE_BYTES, pics.dtype)
    pic[dst] = pics[src]
    return pic


def header(frame):
    """block ids of the 12 sequences and the header block's profile bits (DSF 1, APT 0, VAUX stype 0), in place"""
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
        f[seq, 0, 5] &= 0xF8  # APT = 0
    f[0, 5, 48 + 3] &= 0xE0  # VAUX source pack: stype 0
    return frame


def pack(hosts):
    """two 525/60 DIF frames (240,000 bytes) -> the 625/50 frame that carries their first 324 video segments"""
    _, _, b625, b525 = maps()
    frame = np.zeros(FRAME_BYTES, np.uint8)
    frame[b625] = np.ascontiguousarray(hosts, np.uint8).reshape(HOSTS * D.FRAME_BYTES)[b525]
    return header(frame)


def encode(pic, flags=3, encode525=None):
    """one 625/50 picture -> one DIF frame (the oracle's encoder on every segment, flags as dvo_encode_frame's).
    encode525: another 525/60 encoder (picture, flags) -> frame whose rate control is per segment too"""
    encode525 = encode525 or D.encode
    src, dst, b625, b525 = maps()
    pic = np.ascontiguousarray(pic, np.uint8).reshape(PICTURE_BYTES)
    pics = np.full(HOSTS * D.PICTURE_BYTES, 128, np.uint8)
    pics[src] = pic[dst]
    return pack(np.concatenate([encode525(pics[i * D.PICTURE_BYTES:(i + 1) * D.PICTURE_BYTES], flags) for i in range(HOSTS)]))


def synth625(n, seed=1, amp=8):
    """picture n of a seeded sequence: a smooth gradient, noise of amplitude amp, a few hard edges and a combed band
    (the odd field moved) so that both transform modes and every class occur"""
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    h = (x * 0x9E3779B1) ^ (y * 0x85EBCA77) ^ (n * 0xC2B2AE3D) ^ (seed * 0x27D4EB2F)
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
    cy, cx = np.mgrid[0:CH, 0:CW].astype(np.int64)
    hc = h[0:H:2, 0:W:2]
    nz = ((hc >> 16) % (amp + 1)).astype(np.int64) - amp // 2 if amp else 0
    cb = np.clip(128 + (cx - 180) // 3 + nz // 2, 0, 255).astype(np.uint8)
    cr = np.clip(128 - (cy - 144) // 4 + nz // 2, 0, 255).astype(np.uint8)
    return np.concatenate([Y.ravel(), cb.ravel(), cr.ravel()])
