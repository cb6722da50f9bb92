"""ctypes view of oracle/libdv_float.so (oracle/dv_float.h): a floating-point statement of the DV25 block arithmetic, a
bit-serial parser, a plain encoder and a frame writer from symbols — and the seeded inputs on which the oracle and the
GPU kernel are compared with it.  TEST INFRASTRUCTURE ONLY; PARITY UNPINNED (it pins the fixed-point arithmetic to the
closed form in dv_oracle.c's header comment, not the closed form to the standard).

The inputs are built here, once, so that tests/golden/make_dv_float_bounds.py measures its bounds on exactly what
tests/test_dv_float_cpu.py and tests/test_gpu_dv_float.py run."""
import contextlib
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np

import dvlib as D
import dvsys as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(os.environ.get("MI_SAN_LIBDIR") or os.path.join(ROOT, "oracle"), "libdv_float.so")
if not os.path.exists(LIB):  # a sanitizer build without this library: the plain one
    LIB = os.path.join(ROOT, "oracle", "libdv_float.so")
BOUNDS = os.path.join(ROOT, "tests", "golden", "dv_float_bounds.json")
SEGMENTS, MACROBLOCKS, BLOCKS, SEGMENT_AC_BITS = 270, 1350, 8100, 2680
PERTURBATIONS = {1: "w(4) = 1", 2: "w(2) and w(3) swapped", 3: "area 1 begins one scan position late", 4: "class 3 not doubled",
                 5: "DC scale halved", 6: "2-4-8 sum and difference rows exchanged"}
u8p, i16p, f64p = C.POINTER(C.c_uint8), C.POINTER(C.c_int16), C.POINTER(C.c_double)
_L = None


def lib():
    global _L
    if _L is None:
        if not os.path.exists(LIB):
            subprocess.run(["make", "-C", os.path.join(ROOT, "oracle")], check=True, capture_output=True)
        _L = C.CDLL(LIB)
        ip = C.POINTER(C.c_int)
        _L.dvf_set_perturbation.argtypes = [C.c_int]
        _L.dvf_scan.argtypes = [C.c_int, u8p]
        _L.dvf_area.argtypes = [C.c_int]
        _L.dvf_shift.argtypes = [C.c_int] * 3
        _L.dvf_vlc_lookup.argtypes = [C.c_uint32, ip, ip, ip]
        _L.dvf_mb_place.argtypes = [C.c_int] * 3 + [ip, ip]
        _L.dvf_block_offset.argtypes = [C.c_int] * 2
        _L.dvf_area_offset.argtypes = [C.c_int]
        _L.dvf_weight.argtypes = [C.c_int] * 2
        _L.dvf_weight.restype = C.c_double
        _L.dvf_blocks.argtypes = [C.c_int, i16p, u8p, u8p, u8p, i16p, f64p, u8p]
        _L.dvf_blocks.restype = None
        _L.dvf_block_bits.argtypes = [i16p]
        _L.dvf_decode_frame.argtypes = [u8p, f64p, u8p, C.POINTER(C.c_long)]
        _L.dvf_parse_frame.argtypes = [u8p, u8p, i16p, u8p, u8p, i16p]
        _L.dvf_parse_frame.restype = None
        _L.dvf_write_frame.argtypes = [u8p, i16p, u8p, u8p, i16p, u8p]
        _L.dvf_encode_frame.argtypes = [u8p, u8p, C.c_int, u8p]
        _L.dvf_encode_frame.restype = None
    return _L


@contextlib.contextmanager
def perturbed(which):
    """the float DECODER model made deliberately wrong (dv_float.h); never the code under test"""
    lib().dvf_set_perturbation(which)
    try:
        yield
    finally:
        lib().dvf_set_perturbation(0)


def _p(a, t):
    return a.ctypes.data_as(t)


def _syms(dc, mode, cls, qno, levels):
    return (np.ascontiguousarray(dc, np.int16), np.ascontiguousarray(mode, np.uint8), np.ascontiguousarray(cls, np.uint8),
            np.ascontiguousarray(qno, np.uint8), np.ascontiguousarray(levels, np.int16).reshape(-1, 64))


def blocks(dc, mode, cls, qno, levels):
    """n blocks of symbols -> (n x 64 unrounded pixels, n in-range flags)"""
    dc, mode, cls, qno, levels = _syms(dc, mode, cls, qno, levels)
    n = dc.size
    px, ok = np.zeros((n, 64)), np.zeros(n, np.uint8)
    lib().dvf_blocks(n, _p(dc, i16p), _p(mode, u8p), _p(cls, u8p), _p(qno, u8p), _p(levels, i16p), _p(px, f64p), _p(ok, u8p))
    return px, ok.astype(bool)


def oracle_blocks(dc, mode, cls, qno, levels):
    """the same blocks through dvo_block_pixels"""
    dc, mode, cls, qno, levels = _syms(dc, mode, cls, qno, levels)
    L, px = D.lib(), np.zeros((dc.size, 64), np.uint8)
    for i in range(dc.size):
        L.dvo_block_pixels(int(dc[i]), int(mode[i]), int(cls[i]), int(qno[i]), _p(levels[i], i16p), _p(px[i], u8p))
    return px


def decode_info(dif):
    """one 525/60 DIF frame -> (unrounded picture, blocks outside the fixed-point range, blocks that ended in pass 1/2/3/never)"""
    dif = np.ascontiguousarray(dif, np.uint8)
    pic, fin = np.zeros(D.PICTURE_BYTES), (C.c_long * 4)()
    out = lib().dvf_decode_frame(_p(dif, u8p), _p(pic, f64p), None, fin)
    return pic, out, tuple(fin)


def decode(dif):
    return decode_info(dif)[0]


def parse(dif):
    """(qno[1350], dc[8100], mode, cls, levels[8100][64]) as the bit-serial parser reads a frame"""
    dif = np.ascontiguousarray(dif, np.uint8)
    qno, dc, mode = np.zeros(MACROBLOCKS, np.uint8), np.zeros(BLOCKS, np.int16), np.zeros(BLOCKS, np.uint8)
    cls, levels = np.zeros(BLOCKS, np.uint8), np.zeros((BLOCKS, 64), np.int16)
    lib().dvf_parse_frame(_p(dif, u8p), _p(qno, u8p), _p(dc, i16p), _p(mode, u8p), _p(cls, u8p), _p(levels, i16p))
    return qno, dc, mode, cls, levels


def encode(pic, flags=3, qno_start=None):
    """the plain encoder (no decoder's inverse); qno_start: 270 quantisation numbers the rate control begins at"""
    pic, dif = np.ascontiguousarray(pic, np.uint8), np.zeros(D.FRAME_BYTES, np.uint8)
    q = None if qno_start is None else np.ascontiguousarray(qno_start, np.uint8)
    assert q is None or q.size == SEGMENTS
    lib().dvf_encode_frame(_p(pic, u8p), _p(dif, u8p), flags, None if q is None else _p(q, u8p))
    return dif


class DoesNotFit(ValueError):
    pass


def write_frame(qno, dc, mode, cls, levels):
    """symbols -> DIF frame; raises DoesNotFit when a segment's words need more than its 2,680 AC bits"""
    dc, mode, cls, qno, levels = _syms(dc, mode, cls, qno, levels)
    assert qno.size == MACROBLOCKS and dc.size == mode.size == cls.size == BLOCKS and levels.shape == (BLOCKS, 64)
    dif = np.zeros(D.FRAME_BYTES, np.uint8)
    rc = lib().dvf_write_frame(_p(qno, u8p), _p(dc, i16p), _p(mode, u8p), _p(cls, u8p), _p(levels, i16p), _p(dif, u8p))
    if rc == -1000:
        raise ValueError("a symbol is outside its field")
    if rc:
        raise DoesNotFit(f"segment {-rc - 1} needs more than {SEGMENT_AC_BITS} AC bits")
    return dif


def block_bits(levels):
    return lib().dvf_block_bits(_p(np.ascontiguousarray(levels, np.int16), i16p))


def segment_qnos(dif):
    """the quantisation number of each of a 525/60 frame's 270 segments (its first macroblock's)"""
    return np.array([dif[D.video_block_offset(s // 27, 5 * (s % 27)) + 3] & 15 for s in range(SEGMENTS)], np.uint8)


# ---- 625/50: the same codec functions behind tests/dvsys.py's segment moves ----
def decode625_info(frame):
    outs, fins = [], []

    def one(host):
        pic, out, fin = decode_info(host)
        outs.append(out)
        fins.append(fin)
        return pic
    pic = S.decode(S.SYS_625_50, frame, decode525=one)
    return pic, sum(outs), tuple(int(x) for x in np.sum(fins, axis=0))


def encode625(pic, flags=3):
    return S.encode(S.SYS_625_50, pic, flags, encode525=encode)


# ---- comparison ----
def deviation(got, want):
    """got (uint8 pixels of the fixed-point code) minus the float statement clipped to 0..255, unrounded: an exact
    fixed-point decoder would stay within half a level"""
    return got.astype(np.float64) - np.clip(want, 0.0, 255.0)


def up(x, step):
    """x rounded up to the next multiple of step (the recorded bound of a measured worst case)"""
    return float(np.ceil(round(x / step, 9)) * step)


def bounds():
    with open(BOUNDS) as f:
        return json.load(f)


# ---- seeded inputs ----
SEEDS = {"random_blocks": 20261016, "symbol_frames": [41, 42], "picture_seed": 3}
# (noise amplitude, encoder flags) of the pictures: tests/test_gpu_dv.py's and tests/test_gpu_dv625.py's
PICTURES_525 = [(0, 0), (2, 3), (8, 3), (12, 3), (24, 1), (40, 3), (90, 2)]
PICTURES_625 = [(0, 0), (4, 1), (8, 3), (16, 2), (40, 3), (90, 3)]
TARGET = 112.0  # single-coefficient blocks: the largest level whose pattern stays within 128 +- TARGET


def sweep_index():
    """(mode, scan position, class, qno) of the 8,064 single-coefficient blocks"""
    m, k, c, q = np.meshgrid(np.arange(2), np.arange(1, 64), np.arange(4), np.arange(16), indexing="ij")
    return m.ravel(), k.ravel(), c.ravel(), q.ravel()


@functools.lru_cache(None)
def position_sweep():
    """every (mode, scan position 1..63, class, qno): dc 0 and one level, the largest (up to 255) that keeps the float
    pattern within 128 +- TARGET.  -> (dc, mode, cls, qno, levels)"""
    mode, k, cls, qno = sweep_index()
    n = mode.size
    levels = np.zeros((n, 64), np.int16)
    levels[np.arange(n), k] = 1
    dc = np.zeros(n, np.int16)
    unit = np.abs(blocks(dc, mode, cls, qno, levels)[0] - 128).max(axis=1)
    levels[np.arange(n), k] = np.clip(np.floor(TARGET / unit), 1, 255).astype(np.int16)
    levels[1::2] *= -1  # both signs
    return dc, mode.astype(np.uint8), cls.astype(np.uint8), qno.astype(np.uint8), levels


def unit_amplitude():
    """[mode][k][cls][qno] -> largest |pixel - 128| of level 1 at scan position k (k = 0 unused)"""
    dc, mode, cls, qno, levels = position_sweep()
    one = np.sign(levels).astype(np.int16)
    a = np.abs(blocks(dc, mode, cls, qno, one)[0] - 128).max(axis=1).reshape(2, 63, 4, 16)
    return np.concatenate([np.zeros((2, 1, 4, 16)), a], axis=1)


def dc_sweep():
    dc = np.tile(np.arange(-256, 256, dtype=np.int16), 2)
    mode = np.repeat(np.arange(2, dtype=np.uint8), 512)
    z = np.zeros(1024, np.uint8)
    return dc, mode, z, z, np.zeros((1024, 64), np.int16)


@functools.lru_cache(None)
def random_blocks(n=6000):
    """seeded blocks of 1..20 nonzero levels whose single patterns add up to at most 120 levels around 128 + dc / 2
    (a level of 1 can be worth more than its share, so a few blocks clip at 0 or 255; none leaves the range flag)"""
    rng = np.random.default_rng(SEEDS["random_blocks"])
    unit = unit_amplitude()
    dc, mode = rng.integers(-60, 61, n).astype(np.int16), rng.integers(0, 2, n).astype(np.uint8)
    cls, qno = rng.integers(0, 4, n).astype(np.uint8), rng.integers(0, 16, n).astype(np.uint8)
    levels = np.zeros((n, 64), np.int16)
    for i in range(n):
        cnt = int(rng.integers(1, 21))
        ks = rng.choice(np.arange(1, 64), cnt, replace=False)
        share = rng.dirichlet(np.ones(cnt)) * rng.uniform(20, 120)
        lv = np.floor(share / unit[mode[i], ks, cls[i], qno[i]])
        lv = np.clip(lv, 1, 255) * rng.choice([-1, 1], cnt)
        levels[i, ks] = lv
    return dc, mode, cls, qno, levels


def _fit(levels):
    """trims the 30 blocks of a segment (in place) until their words fit the segment"""
    bits = [block_bits(levels[i]) for i in range(30)]
    while sum(bits) > SEGMENT_AC_BITS:
        i = int(np.argmax(bits))
        nz = np.flatnonzero(levels[i])
        levels[i, nz[-max(1, nz.size // 4):]] = 0
        bits[i] = block_bits(levels[i])


@functools.lru_cache(None)
def symbol_frame(seed):
    """a symbol-written frame: class x qno x mode sweep over the picture (qno and mode by segment and block, class by
    block), light blocks of a few coefficients next to heavy ones of up to 63 small levels, so that macroblocks overflow
    into pass 2 and whole macroblocks into pass 3.  Levels are sized by the float statement's unit patterns so that the
    blocks stay around mid-grey.  -> (dif, (qno, dc, mode, cls, levels))"""
    rng = np.random.default_rng(seed)
    unit = unit_amplitude()
    qno = np.repeat((np.arange(SEGMENTS) * 7 + seed) % 16, 5).astype(np.uint8)
    b = np.arange(BLOCKS)
    cls = ((b + b // 30 + seed) % 4).astype(np.uint8)
    mode = ((b // 4 + b // 30) % 2).astype(np.uint8)
    dc = rng.integers(-40, 41, BLOCKS).astype(np.int16)
    levels = np.zeros((BLOCKS, 64), np.int16)
    for s in range(SEGMENTS):
        kind = s % 3  # 0: one heavy block per macroblock (pass 2); 1: one heavy macroblock (pass 3); 2: both
        for i in range(30):
            g, m = 30 * s + i, i // 6
            heavy = (kind != 1 and i % 6 == (s + m) % 6) or (kind != 0 and m == s % 5)
            cnt = int(rng.integers(36, 64)) if heavy else int(rng.integers(0, 7))
            if not cnt:
                continue
            ks = rng.choice(np.arange(1, 64), cnt, replace=False)
            share = rng.dirichlet(np.ones(cnt)) * rng.uniform(30, 100)
            lv = np.clip(np.floor(share / unit[mode[g], ks, cls[g], qno[5 * s + m]]), 1, 255)
            levels[g, ks] = lv * rng.choice([-1, 1], cnt)
        _fit(levels[30 * s:30 * s + 30])
    return write_frame(qno, dc, mode, cls, levels), (qno, dc, mode, cls, levels)


@functools.lru_cache(None)
def sweep_frame():
    """the 8,064 single-coefficient blocks of position_sweep() as the first blocks of one frame (the remaining 36 are
    flat): the per-position gain test on a whole decoder, in one frame.  qno belongs to the macroblock, so the sweep is
    laid out with qno slowest.  -> (dif, block order: frame block i holds sweep block order[i])"""
    dc, mode, cls, qno, levels = position_sweep()
    order = np.argsort(qno, kind="stable")
    per = order.size // 16  # 504 blocks = 84 macroblocks per qno
    assert per % 6 == 0
    fq = np.zeros(MACROBLOCKS, np.uint8)
    fq[:16 * per // 6] = np.repeat(np.arange(16), per // 6)
    fdc, fmode, fcls = np.zeros(BLOCKS, np.int16), np.zeros(BLOCKS, np.uint8), np.zeros(BLOCKS, np.uint8)
    flev = np.zeros((BLOCKS, 64), np.int16)
    n = order.size
    fdc[:n], fmode[:n], fcls[:n], flev[:n] = dc[order], mode[order], cls[order], levels[order]
    assert np.array_equal(np.repeat(fq, 6)[:n], qno[order])
    return write_frame(fq, fdc, fmode, fcls, flev), order


def block_pixels(pic):
    """a 525/60 picture (any dtype) -> 8100 x 64, block ((seq * 27 + slot) * 5 + m) * 6 + j in row-major pixels"""
    return np.asarray(pic)[_block_map()]


@functools.lru_cache(None)
def _block_map():
    idx = np.zeros((BLOCKS, 64), np.int64)
    x, y = C.c_int(), C.c_int()
    for s in range(SEGMENTS):
        for m in range(5):
            lib().dvf_mb_place(s // 27, s % 27, m, C.byref(x), C.byref(y))
            for j in range(6):
                idx[(5 * s + m) * 6 + j] = S.block411(x.value, y.value, j, D.W, D.H, D.CW)
    return idx


@functools.lru_cache(None)
def picture(system, amp):
    return S.synth(S.SYS_525_60 if system == 525 else S.SYS_625_50, 0, SEEDS["picture_seed"] + amp, amp)


@functools.lru_cache(None)
def frames(system, family):
    """the frames of a family, three encoders apart: 'a' the oracle's encoder, 'b' the plain encoder, on the same
    synthetic pictures; 'c' symbol-written.  625/50 frames carry the same codec's segments (tests/dvsys.py)."""
    pics = PICTURES_525 if system == 525 else PICTURES_625
    if family == "a":
        sys_ = S.SYS_525_60 if system == 525 else S.SYS_625_50
        return [S.encode(sys_, picture(system, amp), flags) for amp, flags in pics]
    if family == "b":
        enc = encode if system == 525 else encode625
        return [enc(picture(system, amp), flags) for amp, flags in pics]
    assert family == "c"
    if system == 525:
        return [symbol_frame(seed)[0] for seed in SEEDS["symbol_frames"]]
    a, b = (symbol_frame(seed)[0] for seed in SEEDS["symbol_frames"])
    return [S.pack(S.SYS_625_50, np.concatenate([a, b])), S.pack(S.SYS_625_50, np.concatenate([b, a]))]


def oracle_decode(system, frame):
    return S.decode(S.SYS_525_60 if system == 525 else S.SYS_625_50, frame)


def float_decode_info(system, frame):
    return decode_info(frame) if system == 525 else decode625_info(frame)


# ---- measurements (the generator records them, the tests repeat them) ----
def measure_blocks(inputs, got=None):
    """-> dict: worst |deviation|, mean signed deviation, worst |gain - 1| and where; `got` defaults to the oracle's pixels"""
    px, ok = blocks(*inputs)
    got = oracle_blocks(*inputs) if got is None else got
    d = deviation(got, px)
    w = np.clip(px, 0, 255) - 128
    den = (w * w).sum(axis=1)
    gain = np.where(den > 0, ((got.astype(np.float64) - 128) * w).sum(axis=1) / np.where(den > 0, den, 1), 1.0)
    return {"abs": float(np.abs(d).max()), "abs_at": int(np.abs(d).max(axis=1).argmax()), "mean": float(d.mean()),
            "gain": float(np.abs(gain - 1).max()), "gain_at": int(np.abs(gain - 1).argmax()), "out_of_range": int((~ok).sum())}


def psnr(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(10 * np.log10(255.0 ** 2 / max((d * d).mean(), 1e-9)))
