"""Checker of the 4:2:2 and greyscale RTjpeg encoders (include/mi_rtjpeg.h, mi_rtj_encode_frames_fmt / _stream_fmt).

A block's coding (forward transform, quantiser, RTjpeg_b2s, RTjpeg_bcomp) does not depend on the picture format, so the
pinned oracle's 4:2:0 encoder restates the other two: the blocks of a 4:2:2 or greyscale picture are placed into a 4:2:0
picture of rtjfmt.source_size() such that rtjfmt.repack() of its packet is the format's packet.  The placement is
repack's rule read backwards:
    4:2:2 macroblock m   luma block k (0, 1) -> luma block 2m + k of the 4:2:0 picture, Cb -> U and Cr -> V of macroblock m
    greyscale block b    -> luma block b
where luma block i of a 4:2:0 picture is quadrant i % 4 (0 top left, 1 top right, 2 bottom left, 3 bottom right) of
macroblock i // 4.  Unused blocks are zero and never reach the output.  One OracleEncoder per stream carries the
previous-block store of inter streams.

tests/test_rtjfmt_encode_cpu.py holds this restatement to golden packets made by the reference and, where oracle/_ref
was built, to the reference's own encoder.  Greyscale: the encoder under test codes the picture it is given (block row r
is lines 8r .. 8r+7), the reference's greyscale arms read other lines (lib/RTjpeg.c:2626, 2630, 3004: a line stride of
8 w); ref_grey_planes() lays a picture out so that the reference reads the same pixels, where such a layout exists.

Only tests/ and tools/bench_formats.py import this."""
import numpy as np

import rtjfmt as F
import rtjlib as R

# noise amplitudes of the golden's cases (tests/golden/make_rtjfmt_golden.py, CASES): the npz does not record them
GOLDEN_AMP = {0: 64, 1: 8, 2: 8, 3: 8, 4: 0, 5: 64, 6: 8, 7: 8, 8: 0}


def arrange(fmt, w, h, pic):
    """The 4:2:0 picture (contiguous planes, source_size()) whose coded blocks, repacked, are those of `pic`."""
    assert fmt in (F.FMT_422, F.FMT_GREY) and F.geometry_ok(fmt, w, h)
    pic = np.ascontiguousarray(pic, dtype=np.uint8)
    assert pic.size == F.plane_bytes(fmt, w, h)
    W, H = F.source_size(fmt, w, h)
    mbw = W // 16
    Y = np.zeros((H, W), np.uint8)
    U = np.zeros((H // 2, W // 2), np.uint8)
    V = np.zeros((H // 2, W // 2), np.uint8)

    def put_luma(i, blk):
        mb, q = divmod(i, 4)
        my, mx = divmod(mb, mbw)
        y0, x0 = 16 * my + 8 * (q >> 1), 16 * mx + 8 * (q & 1)
        Y[y0:y0 + 8, x0:x0 + 8] = blk

    y, cb, cr = F.split(fmt, pic, w, h)
    y = y.reshape(h, w)
    if fmt == F.FMT_422:
        cb, cr = cb.reshape(h, w // 2), cr.reshape(h, w // 2)
        per_row = w // 16
        for m in range(per_row * (h // 8)):
            i, j = divmod(m, per_row)
            put_luma(2 * m, y[8 * i:8 * i + 8, 16 * j:16 * j + 8])
            put_luma(2 * m + 1, y[8 * i:8 * i + 8, 16 * j + 8:16 * j + 16])
            my, mx = divmod(m, mbw)
            U[8 * my:8 * my + 8, 8 * mx:8 * mx + 8] = cb[8 * i:8 * i + 8, 8 * j:8 * j + 8]
            V[8 * my:8 * my + 8, 8 * mx:8 * mx + 8] = cr[8 * i:8 * i + 8, 8 * j:8 * j + 8]
    else:
        per_row = w // 8
        for b in range(per_row * (h // 8)):
            i, j = divmod(b, per_row)
            put_luma(b, y[8 * i:8 * i + 8, 8 * j:8 * j + 8])
    return np.concatenate([Y.reshape(-1), U.reshape(-1), V.reshape(-1)])


class RestatedEncoder:
    """One encoder instance in format `fmt` (one stream, if key_rate > 0): RTjpeg_compress after RTjpeg_set_format,
    RTjpeg_set_size, RTjpeg_set_quality and, with key_rate > 0, RTjpeg_set_intra."""

    def __init__(self, fmt, w, h, Q, key_rate=0, lmask=0, cmask=0):
        self.fmt, self.w, self.h = fmt, w, h
        self.enc = R.OracleEncoder(*F.source_size(fmt, w, h), Q, key_rate, lmask, cmask)

    def encode(self, pic):
        return F.repack(self.fmt, self.w, self.h, self.enc.encode(arrange(self.fmt, self.w, self.h, pic)))


def encode_all(fmt, w, h, Q, pics, key_rate=0, lmask=0, cmask=0):
    """packets of `pics`: independent pictures (key_rate 0) or one stream in order"""
    enc = RestatedEncoder(fmt, w, h, Q, key_rate, lmask, cmask)
    return [enc.encode(p) for p in pics]


def block_offsets(fmt, pkt):
    """block starts of a packet relative to its first data byte, nblocks + 1 entries"""
    w, h, _ = F.header_of(pkt)
    used, offs = F.Restated(fmt).decode(pkt, np.zeros(F.plane_bytes(fmt, w, h), np.uint8))
    assert used == pkt.size
    return offs.astype(np.int64)


def block_kinds(fmt, pkt):
    """(unchanged blocks, coded blocks) of a packet.  An unchanged block is one byte, 0xFF; a coded block never starts
    with 0xFF (its DC byte is clamped to 254) and has at least two bytes."""
    offs = block_offsets(fmt, pkt)
    first = pkt[F.HEADER + offs[:-1]]
    length = np.diff(offs)
    unchanged = (first == 0xFF)
    assert np.all(length[unchanged] == 1) and np.all(length[~unchanged] >= 2)
    return int(np.count_nonzero(unchanged)), int(np.count_nonzero(~unchanged))


def make_stream(fmt, w, h, n, seed=1, amp=8):
    """rtjfmt.make_stream with a change no quantiser of Q >= 64 rounds away: the new top third of every odd picture is
    inverted (255 - v), so that two consecutive pictures differ there by an inversion and are equal below it.  (With
    rtjfmt.make_stream's gradient step alone a coarse quantiser can keep a whole packet within masks of 2.)"""
    pics = F.make_stream(fmt, w, h, n, seed, amp)
    k = pics[0].size // 3
    for i in range(1, n, 2):
        pics[i][:k] = 255 - pics[i][:k]
    return pics


def all_blocks_forced_unchanged(Q, lmask, cmask):
    """True for the inter settings at which the reference's own packets hold no coded block at all, the first packet of
    a stream included: quality 1 with both masks at 2 or more.  Quality 1 quantises every coefficient of an 8-bit picture
    to -2 .. 2 (the coarsest tables: a DC of 255 * 64 gives 2), which is within such a mask of the cleared, all-zero
    previous-block store — so nothing is ever stored and every block of every picture is the byte 0xFF.  A test that
    exempts these settings from "some blocks coded" asserts "no block coded" instead."""
    return Q == 1 and min(lmask, cmask) >= 2


EXTREMES = ("zeros", "full", "stripes", "binary", "uniform")


def extreme_picture(fmt, w, h, kind, seed=1):
    """all 0, all 255, alternating 0 / 255, random 0 / 255, uniform random bytes"""
    n = F.plane_bytes(fmt, w, h)
    rng = np.random.default_rng([seed, fmt, w, h, EXTREMES.index(kind)])
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    if kind == "full":
        return np.full(n, 255, np.uint8)
    if kind == "stripes":
        return ((np.arange(n) & 1) * 255).astype(np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, n) * 255).astype(np.uint8)
    return rng.integers(0, 256, n, dtype=np.uint8)


def golden_422():
    """[(case, w, h, Q, key_rate, [pictures], [packets])] of the golden's 4:2:2 cases: the packets the reference made, and
    the pictures make_rtjfmt_golden.py gave it (make_stream(fmt, w, h, n, seed=10 + case, amp))."""
    g = F.load_golden()
    out = []
    for row in g["cases"]:
        ci, fmt, w, h, Q, key, n = [int(x) for x in row]
        if fmt != F.FMT_422:
            continue
        pics = F.make_stream(fmt, w, h, n, seed=10 + ci, amp=GOLDEN_AMP[ci])
        out.append((ci, w, h, Q, key, pics, [g[f"c{ci}_pkt{i}"] for i in range(n)]))
    return out


def ref_grey_planes(pic, w, h, inter):
    """A zero-padded buffer in which the reference's greyscale encoder reads the pixels of `pic`'s blocks, or None where
    there is none.  Its block (row r, line k) is line r + 8k of the buffer in the intra arm (lib/RTjpeg.c:2626, 2630: one
    to one for h <= 64, above that two block rows claim the same line) and line 8r + 8k in the inter arm (:3004, 3012:
    one to one only for h = 8)."""
    if (inter and h != 8) or h > 64:
        return None
    src = np.ascontiguousarray(pic, dtype=np.uint8).reshape(h, w)
    pad = np.zeros((h // 8 + 57, w), np.uint8)
    for r in range(h // 8):
        for k in range(8):
            pad[(8 * r if inter else r) + 8 * k] = src[8 * r + k]
    return pad.reshape(-1)
