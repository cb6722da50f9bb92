"""What tests/test_dv_encode_cpu.py and tests/golden/make_dv_encode_bounds.py share: the 525/60 pictures the statement
tests/dvenc.py is checked on, and its measurements against code that shares nothing with it — the float statement's
parser, writer, weights and shifts (oracle/dv_float.c through dvfloat) and a numpy double orthonormal transform written
here.  TEST INFRASTRUCTURE ONLY."""
import functools
import json
import os

import numpy as np

import dvenc as E
import dvfloat as F
import dvlib as D
import dvsys as S

BOUNDS = os.path.join(F.ROOT, "tests", "golden", "dv_encode_bounds.json")
# dvlib.synth pictures at noise 0, 8 and 64, uniformly random bytes, and the drop-rule picture (tests/dvenc.py)
NAMES = ("flat", "n8", "n64", "random", "drop")
FRAMES = [(name, flags) for name in NAMES[:4] for flags in range(4)] + [("drop", 3)]
STEP_DEVIATION, STEP_DB = 0.01, 0.1


@functools.lru_cache(None)
def picture(name):
    if name == "random":
        return np.random.default_rng(20261019).integers(0, 256, D.PICTURE_BYTES, dtype=np.uint8)
    if name == "drop":
        return E.drop_picture(S.SYS_525_60)
    if name == "edges":  # not one of NAMES: tests/test_dv_encode_edges_cpu.py asks for it
        import dvenc_edges
        return dvenc_edges.picture(S.SYS_525_60)
    return D.synth(0, 1, {"flat": 0, "n8": 8, "n64": 64}[name])


@functools.lru_cache(None)
def stated(name, flags):
    """(frame, record) of the statement"""
    rec = {}
    fr = E.encode525(picture(name), flags, rec)
    fr.setflags(write=False)
    return fr, rec


def _dmat(n):
    k, i = np.mgrid[0:n, 0:n]
    return np.where(k == 0, np.sqrt(1.0 / n), np.sqrt(2.0 / n)) * np.cos((2 * i + 1) * k * np.pi / (2 * n))


def orthonormal(px, mode):
    """[n][64] pixels, [n] modes -> [n][64] double coefficients, natural order: the orthonormal 8-8 transform, or the
    4-point one on the sums and differences of line pairs over sqrt 2 (rows 2v / 2v + 1) and the 8-point one along the lines"""
    D8, D4 = _dmat(8), _dmat(4)
    p = px.reshape(-1, 8, 8).astype(np.float64) - 128.0
    t = p @ D8.T
    f88 = np.einsum("ry,nyh->nrh", D8, t)
    f248 = np.empty_like(t)
    f248[:, 0::2] = np.einsum("vi,nih->nvh", D4, t[:, 0::2] + t[:, 1::2]) / np.sqrt(2.0)
    f248[:, 1::2] = np.einsum("vi,nih->nvh", D4, t[:, 0::2] - t[:, 1::2]) / np.sqrt(2.0)
    return np.where(np.asarray(mode)[:, None, None] != 0, f248, f88).reshape(-1, 64)


@functools.lru_cache(None)
def _closed_form_tables():
    L = F.lib()
    scan = np.zeros((2, 64), np.uint8)
    for m in range(2):
        L.dvf_scan(m, scan[m].ctypes.data_as(F.u8p))
    w = np.array([[L.dvf_weight(m, int(scan[m, k])) for k in range(64)] for m in range(2)])
    area = np.array([L.dvf_area(k) for k in range(64)])
    shift = np.array([[[L.dvf_shift(q, c, a) for a in range(4)] for c in range(4)] for q in range(16)])
    return scan.astype(np.int64), w, area, shift


def deviation(name, flags):
    """the largest |level - F W / 2^s| over every block and AC position of a picture where the level is not clipped: the
    levels are the statement's at the qno and class it chose, before the overflow rule; F, W and s share nothing with it.
    Also checks that the recorded levels are those, but for dropped ones."""
    px = picture(name)[E.block_map()]
    r = E.encode_blocks(px, flags)
    mode, cls, qno = r["mode"], r["cls"], np.repeat(r["qno"], 30)
    P, neg = E.products(E.transform(px, mode), mode)
    lv = E.quantise(P, neg, cls, qno)
    kept = r["levels"] != 0
    assert np.array_equal(np.where(kept, lv, 0), r["levels"]) and int((lv != 0).sum() - kept.sum()) == int(r["dropped"].sum())
    scan, w, area, shift = _closed_form_tables()
    Fc = np.take_along_axis(orthonormal(px, mode), scan[mode], axis=1)
    quotient = Fc * w[mode] / np.exp2(shift[qno, cls][:, area])
    d = np.abs(lv - quotient)[:, 1:]
    return float(d[np.abs(lv[:, 1:]) < 255].max())


def psnr_525(name):
    """PSNR against the source of the oracle's decode of the statement's, the oracle's and the float encoder's frame (flags 3)"""
    pic = picture(name)
    return tuple(F.psnr(D.decode(fr), pic) for fr in (stated(name, 3)[0], D.encode(pic, 3), F.encode(pic, 3)))


def psnr_system(system):
    """the same for dvsys.synth(system, 0, 1, 8) through dvsys.encode / dvsys.decode"""
    pic = S.synth(system, 0, 1, 8)
    frames = (S.encode(system, pic, 3, encode525=E.encode525), S.encode(system, pic, 3), S.encode(system, pic, 3, encode525=F.encode))
    return tuple(F.psnr(S.decode(system, fr), pic) for fr in frames)


def shortfall(p):
    """how far the statement's PSNR is below the lower of the two existing encoders', rounded up to 0.1 dB"""
    return F.up(max(0.0, min(p[1], p[2]) - p[0]), STEP_DB)


def bounds():
    with open(BOUNDS) as f:
        return json.load(f)
