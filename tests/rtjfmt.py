"""Checker of the 4:2:2 and greyscale RTjpeg decoders (include/mi_rtjpeg.h, mi_rtj_set_format).

The two loops of the reference that RTjpeg_decompress dispatches to next to the 4:2:0 one — RTjpeg_decompressYUV422
(lib/RTjpeg.c:2639-2686) and RTjpeg_decompress8 (:2751-2772) — restated over the pinned oracle's block helpers
(rtjo_make_tables, rtjo_s2b, rtjo_idct: oracle/rtj_oracle.h).  tests/test_rtjfmt_cpu.py holds this restatement to the
reference's own code (oracle/_ref, where it was built) and to golden vectors made by it; the GPU tests are then held
to the restatement.  Also: a numpy RTjpeg_yuv422rgb24 (:3077-3121), ctypes bindings of the reference library with
RTjpeg_set_format, a seeded picture maker, and packets of both formats made without the reference (make_packets).

Only tests/ and tools/bench_formats.py import this."""
import ctypes as C
import os

import numpy as np

import rtjlib as R

FMT_420, FMT_422, FMT_GREY = 0, 1, 2  # RTJ_YUV420 / RTJ_YUV422 / RTJ_RGB8 (include/RTjpeg.h:111-113)
HEADER = 12
GOLDEN_NPZ = os.path.join(R.GOLDEN, "rtjfmt_golden.npz")

i32p = C.POINTER(C.c_int32)


def geometry_ok(fmt, w, h):
    """Where the reference's loop ends and stays inside the planes (lib/RTjpeg.c:2651-2653, 2761-2763)."""
    if w <= 0 or h <= 0:
        return False
    if fmt == FMT_422:
        return w % 16 == 0 and h % 8 == 0
    if fmt == FMT_GREY:
        return w % 8 == 0 and h % 8 == 0
    return w % 16 == 0 and h % 16 == 0


def nblocks(fmt, w, h):
    if fmt == FMT_422:
        return (w // 16) * (h // 8) * 4
    if fmt == FMT_GREY:
        return (w // 8) * (h // 8)
    return (w // 16) * (h // 16) * 6


def plane_bytes(fmt, w, h):
    return {FMT_420: w * h * 3 // 2, FMT_422: 2 * w * h, FMT_GREY: w * h}[fmt]


def split(fmt, buf, w, h):
    """(y, cb, cr) views of contiguous planes; greyscale: (y, None, None)."""
    ys = w * h
    if fmt == FMT_GREY:
        return buf[:ys], None, None
    cs = ys // 2 if fmt == FMT_422 else ys // 4
    return buf[:ys], buf[ys:ys + cs], buf[ys + cs:ys + 2 * cs]


def header_of(pkt):
    hdr = np.zeros(HEADER, np.uint8)
    m = min(HEADER, pkt.size)
    hdr[:m] = pkt[:m]
    return int(hdr[6]) | (int(hdr[7]) << 8), int(hdr[8]) | (int(hdr[9]) << 8), int(hdr[10])


class Restated:
    """One decoder instance in format `fmt`: RTjpeg_decompress's header logic (lib/RTjpeg.c:3568-3579) and the
    format's block loop.  A fresh instance has the all-zero tables of RTjpeg_init's bzero, lb8 = cb8 = 0."""

    def __init__(self, fmt):
        assert fmt in (FMT_422, FMT_GREY)
        self.fmt = fmt
        self.L = R.oracle()
        self.w = self.h = self.Q = 0
        self.t = R.RtjoTables()  # zeroed

    def decode(self, pkt, planes):
        """pkt: uint8 array (whole packet).  planes: uint8 array of plane_bytes(), updated in place (a 0xFF block
        leaves its 8x8 destination as it was).  Returns (bytes consumed with the header, block offsets relative to
        the first data byte: nblocks + 1 entries), or None where the reference's loop would not end."""
        pkt = np.ascontiguousarray(pkt, dtype=np.uint8)
        w, h, q = header_of(pkt)
        if not geometry_ok(self.fmt, w, h):
            return None
        self.w, self.h = w, h
        if q != self.Q:
            self.Q = max(q, 1)
            self.L.rtjo_make_tables(self.Q, C.byref(self.t))
        nb = nblocks(self.fmt, w, h)
        # bytes at or past the packet's end read as 0: a block made of them is 64 bytes long
        pad = np.zeros(max(pkt.size, HEADER) + 64 * nb + 64, np.uint8)
        pad[:pkt.size] = pkt
        base = pad.ctypes.data
        y, cb, cr = split(self.fmt, planes, w, h)
        coef = (C.c_int16 * 64)()
        liqt = C.cast(self.t.liqt, i32p)
        ciqt = C.cast(self.t.ciqt, i32p)
        offs = np.zeros(nb + 1, np.uint32)
        sp = HEADER
        k = 0

        def block(luma, dst, dst_off, stride):
            nonlocal sp, k
            offs[k] = sp - HEADER
            k += 1
            if pad[sp] == 0xFF:
                sp += 1
                return
            sp += self.L.rtjo_s2b(C.cast(base + sp, R.u8p), pad.size - sp, self.t.lb8 if luma else self.t.cb8,
                                  liqt if luma else ciqt, coef)
            self.L.rtjo_idct(coef, C.cast(dst.ctypes.data + dst_off, R.u8p), stride)

        if self.fmt == FMT_422:
            cw = w // 2
            for i in range(h // 8):
                for j in range(w // 16):
                    block(True, y, 8 * i * w + 16 * j, w)
                    block(True, y, 8 * i * w + 16 * j + 8, w)
                    block(False, cb, 8 * i * cw + 8 * j, cw)
                    block(False, cr, 8 * i * cw + 8 * j, cw)
        else:
            for i in range(h // 8):
                for j in range(w // 8):
                    block(True, y, 8 * i * w + 8 * j, w)
        offs[k] = sp - HEADER
        return sp, offs


def yuv422_to_rgb24(w, h, planes, dst, pitch):
    """RTjpeg_yuv422rgb24 (lib/RTjpeg.c:3077-3121): dst is a uint8 array of h * pitch bytes, updated in place; the
    bytes of a row past its 3 w are left alone."""
    y, cb, cr = split(FMT_422, planes, w, h)
    yy = (y.reshape(h, w).astype(np.int64) - 16) * 76284
    u = np.repeat(cb.reshape(h, w // 2).astype(np.int64) - 128, 2, axis=1)
    v = np.repeat(cr.reshape(h, w // 2).astype(np.int64) - 128, 2, axis=1)
    r = np.clip((yy + v * 76284) >> 16, 0, 255)
    g = np.clip((yy - v * 53281 - u * 25625) >> 16, 0, 255)
    b = np.clip((yy + u * 132252) >> 16, 0, 255)
    rows = dst.reshape(h, pitch)
    rows[:, :3 * w] = np.stack([r, g, b], axis=2).reshape(h, 3 * w).astype(np.uint8)


def make_picture(fmt, w, h, n, seed=1, amp=8):
    """Contiguous planes of a seeded picture: a moving diagonal gradient plus uniform noise of +-amp on luma and
    +-amp/2 on chroma."""
    rng = np.random.default_rng([seed, fmt, w, h, n])
    xs = np.arange(w, dtype=np.int64)[None, :]
    ys = np.arange(h, dtype=np.int64)[:, None]
    base = 16 + ((xs + ys + 7 * n) % (w + h)) * 219 // (w + h)
    y = np.clip(base + rng.integers(-amp, amp + 1, (h, w)), 0, 255).astype(np.uint8).reshape(-1)
    if fmt == FMT_GREY:
        return y
    cs = plane_bytes(fmt, w, h) - w * h
    c = np.clip(128 + rng.integers(-(amp // 2), amp // 2 + 1, cs), 0, 255).astype(np.uint8)
    return np.concatenate([y, c])


def make_stream(fmt, w, h, n, seed=1, amp=8):
    """n consecutive pictures of one stream: picture 0, then pictures whose first third (the top of the luma plane) is
    new and whose rest stays — so that an encoder with RTjpeg_set_intra codes some blocks and marks the others unchanged."""
    first = make_picture(fmt, w, h, 0, seed, amp)
    pics = [first]
    for i in range(1, n):
        p = first.copy()
        k = p.size // 3
        p[:k] = make_picture(fmt, w, h, i, seed, max(amp, 8))[:k]
        pics.append(p)
    return pics


# ---------------------------------------------------------------------------
# packets without the reference encoder (the GPU tests run where oracle/_ref may be absent)
#
# A block's coding (RTjpeg_b2s, lib/RTjpeg.c:109-155) does not depend on the picture format: a 4:2:2 stream is luma,
# luma, chroma, chroma blocks macroblock after macroblock, a greyscale stream luma blocks alone.  The pinned oracle's
# 4:2:0 encoder makes coded blocks (0xFF "unchanged" ones included, with key_rate > 0); put in the other format's
# order they are a well-formed stream of that format.  What the picture shows is of no interest to a decoder test: the
# decoders are compared with the restatement above, which the CPU tests hold to the reference.
# ---------------------------------------------------------------------------
def _up16(x):
    return (x + 15) // 16 * 16


def source_size(fmt, w, h):
    """size of the 4:2:0 picture whose blocks fill a w x h picture of `fmt`"""
    return (w, _up16(2 * h)) if fmt == FMT_422 else (_up16(w), _up16(h))


def repack(fmt, w, h, pkt420):
    """The coded blocks of a 4:2:0 packet (of source_size()) as a packet of `fmt`, w x h."""
    offs = R.OracleDecoder().block_offsets(pkt420).astype(np.int64)
    blocks = [pkt420[offs[k]:offs[k + 1]] for k in range(offs.size - 1)]
    luma = [b for k, b in enumerate(blocks) if k % 6 < 4]
    chroma = [b for k, b in enumerate(blocks) if k % 6 >= 4]
    seq = []
    if fmt == FMT_422:
        for mb in range((w // 16) * (h // 8)):
            seq += [luma[2 * mb], luma[2 * mb + 1], chroma[2 * mb], chroma[2 * mb + 1]]
    else:
        seq = luma[:nblocks(fmt, w, h)]
    assert len(seq) == nblocks(fmt, w, h)
    body = np.concatenate(seq)
    hdr = pkt420[:HEADER].copy()
    hdr[0:4] = np.frombuffer(np.uint32(HEADER + body.size).tobytes(), np.uint8)
    hdr[6], hdr[7], hdr[8], hdr[9] = w & 255, w >> 8, h & 255, h >> 8
    return np.concatenate([hdr, body])


def make_packets(fmt, w, h, Q, n=1, seed=1, amp=8, key_rate=0, lmask=2, cmask=2):
    """n packets of `fmt`, w x h, quality Q: intra (key_rate 0, independent pictures) or one stream with unchanged blocks."""
    W, H = source_size(fmt, w, h)
    enc = R.OracleEncoder(W, H, Q, key_rate, lmask, cmask)
    if key_rate:
        first = R.synth_frame(W, H, 0, seed=seed, amp=amp)
        frames = [first]
        for i in range(1, n):
            f = first.copy()
            f[:f.size // 3] = R.synth_frame(W, H, i, seed=seed, amp=max(amp, 8))[:f.size // 3]
            frames.append(f)
    else:
        frames = [R.synth_frame(W, H, i, seed=seed, amp=amp) for i in range(n)]
    return [repack(fmt, w, h, enc.encode(f)) for f in frames]


def planes_arg(fmt, buf, w, h):
    y, cb, cr = split(fmt, buf, w, h)
    if fmt == FMT_GREY:
        return (R.u8p * 3)(R._ptr(y), None, None)
    return (R.u8p * 3)(R._ptr(y), R._ptr(cb), R._ptr(cr))


class RefFmt:
    """The reference's own RTjpeg_t (oracle/_ref/librtjpeg_ref.so) with RTjpeg_set_format."""

    def __init__(self, fmt):
        self.fmt = fmt
        self.L = R.reference()
        self.L.RTjpeg_set_format.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        self.h = self.L.RTjpeg_init()
        f = C.c_int(fmt)
        self.L.RTjpeg_set_format(self.h, C.byref(f))

    def __del__(self):
        if getattr(self, "h", None):
            self.L.RTjpeg_close(self.h)
            self.h = None

    def setup_encoder(self, w, h, Q, key_rate=0, lmask=0, cmask=0):
        self.w, self.h_ = w, h
        cw, ch, cq = C.c_int(w), C.c_int(h), C.c_int(Q)
        self.L.RTjpeg_set_size(self.h, C.byref(cw), C.byref(ch))
        self.L.RTjpeg_set_quality(self.h, C.byref(cq))
        if key_rate > 0:
            k, l, c = C.c_int(key_rate), C.c_int(lmask), C.c_int(cmask)
            self.L.RTjpeg_set_intra(self.h, C.byref(k), C.byref(l), C.byref(c))
        self.buf = np.zeros(64 + nblocks(self.fmt, w, h) * 64, dtype=np.uint8)

    def encode(self, planes):
        planes = np.ascontiguousarray(planes, dtype=np.uint8)
        n = self.L.RTjpeg_compress(self.h, R._ptr(self.buf), planes_arg(self.fmt, planes, self.w, self.h_))
        return self.buf[:n].copy()

    def decode(self, pkt, out):
        """out: plane_bytes() bytes, updated in place.  The packet is zero-padded: the reference has no bound."""
        w, h, _ = header_of(pkt)
        pad = np.zeros(pkt.size + 64 * nblocks(self.fmt, w, h) + 64, dtype=np.uint8)
        pad[:pkt.size] = pkt
        self.L.RTjpeg_decompress(self.h, R._ptr(pad), planes_arg(self.fmt, out, w, h))

    def to_rgb24(self, w, h, planes, dst, pitch):
        """RTjpeg_yuv422rgb24 on contiguous 4:2:2 planes; it takes an array of row pointers."""
        cw, ch = C.c_int(w), C.c_int(h)
        self.L.RTjpeg_set_size(self.h, C.byref(cw), C.byref(ch))
        rows = (R.u8p * h)(*[C.cast(dst.ctypes.data + r * pitch, R.u8p) for r in range(h)])
        fn = self.L.RTjpeg_yuv422rgb24
        fn.argtypes = [C.c_void_p, C.POINTER(R.u8p), C.POINTER(R.u8p)]
        fn.restype = None
        fn(self.h, planes_arg(FMT_422, planes, w, h), rows)


def load_golden():
    """{name: array} of tests/golden/rtjfmt_golden.npz (made by tests/golden/make_rtjfmt_golden.py with the reference)."""
    with np.load(GOLDEN_NPZ) as z:
        return {k: z[k] for k in z.files}


def golden_cases(g):
    """[(fmt, w, h, Q, key_rate, [packets], [planes after each packet of a decoder whose planes started as 77])]"""
    out = []
    for row in g["cases"]:
        ci, fmt, w, h, Q, key, n = [int(x) for x in row]
        pk = [g[f"c{ci}_pkt{i}"] for i in range(n)]
        pl = [g[f"c{ci}_out{i}"] for i in range(n)]
        out.append((fmt, w, h, Q, key, pk, pl))
    return out
