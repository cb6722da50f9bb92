"""DV25 625/50 (IEC 4:2:0) without a GPU: the kernels' macroblock placement (mi_dv_mb_place) against the test statement
(tests/dvsys.py) and, for 525/60, against the oracle; the host-side profile check (mi_dv_system_of); the statement's own
round trip.  PARITY UNPINNED: both statements of 625/50 are this repository's reading of the published format."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import dvlib as D
import dvsys as S
from pkg import ROOT

G = S.geometry(S.SYS_625_50)


@pytest.fixture(scope="module")
def dv():
    return importlib.import_module("gmerlin-avdecoder_amd.dv")


def test_625_placement_is_a_bijection_and_matches_the_statement(dv):
    seen = np.zeros((36, 45), np.int32)
    for seq in range(12):
        for slot in range(27):
            for m in range(5):
                x, y = dv.mb_place(dv.SYS_625_50, seq, slot, m)
                assert (x, y) == S.mb_place(S.SYS_625_50, seq, slot, m), (seq, slot, m)
                seen[y, x] += 1
    assert (seen == 1).all()


def test_525_placement_is_the_oracles(dv):
    L = D.lib()
    for seq in range(10):
        for slot in range(27):
            for m in range(5):
                x, y = C.c_int(), C.c_int()
                L.dvo_mb_place(seq, slot, m, C.byref(x), C.byref(y))
                assert dv.mb_place(dv.SYS_525_60, seq, slot, m) == (x.value, y.value), (seq, slot, m)


@pytest.mark.parametrize("args", [(0, 10, 0, 0), (1, 12, 0, 0), (1, 0, 27, 0), (1, 0, 0, 5), (1, -1, 0, 0), (2, 0, 0, 0),
                                  (-1, 0, 0, 0)])
def test_placement_refuses_what_is_out_of_range(dv, args):
    with pytest.raises(dv.MiDvError):
        dv.mb_place(*args)


@pytest.fixture(scope="module")
def dvframe():
    from test_dvframe_host import Profile  # the struct of include/mi_dvframe.h
    subprocess.run(["make", "-C", os.path.join(ROOT, "gmerlin-avdecoder_amd", "csrc"),
                    os.path.join(ROOT, "gmerlin-avdecoder_amd", "lib", "libmi_dvframe.so")], check=True, capture_output=True)
    lib = C.CDLL(os.path.join(ROOT, "gmerlin-avdecoder_amd", "lib", "libmi_dvframe.so"))
    lib.mi_dv_profile_at.restype = C.POINTER(Profile)
    lib.mi_dv_frame_profile.restype = C.POINTER(Profile)
    lib.mi_dv_frame_profile.argtypes = [C.POINTER(C.c_uint8)]
    return lib


def test_system_of_every_profile(dv, dvframe):
    from test_dvframe_host import make_frame
    rng = np.random.default_rng(3)
    for i in range(dvframe.mi_dv_num_profiles()):
        p = dvframe.mi_dv_profile_at(i).contents
        f = make_frame(p, rng, apt=1 if i == 2 else 0)
        got = dvframe.mi_dv_frame_profile(f.ctypes.data_as(C.POINTER(C.c_uint8))).contents
        assert got.frame_size == p.frame_size and got.pix_fmt == p.pix_fmt  # the frame is of profile i
        want = {0: dv.SYS_525_60, 1: dv.SYS_625_50}.get(i, -1)
        assert dv.system_of(f) == want, i
        assert dv.system_of(f[:p.frame_size - 1]) == -1, i
        assert dv.system_of(f[:400]) == -1, i
    # every APT value but 0 marks DVCPRO 625/50 4:1:1
    p = dvframe.mi_dv_profile_at(1).contents
    for apt in range(1, 8):
        assert dv.system_of(make_frame(p, rng, apt=apt)) == -1
    # a 525/60 frame is long enough at 120,000 bytes, a 625/50 one is not
    f = make_frame(p, rng)
    assert dv.system_of(f[:120000]) == -1 and dv.system_of(f) == dv.SYS_625_50


def test_statement_frames_announce_625_50(dv):
    f = S.encode(S.SYS_625_50, S.synth(S.SYS_625_50, 0, 2, 6), 3)
    assert f.size == G.frame_bytes and dv.system_of(f) == dv.SYS_625_50


def _block_means(pic):
    out = []
    for off, w, h in ((0, G.w, G.h), (G.w * G.h, G.cw, G.ch), (G.w * G.h + G.cw * G.ch, G.cw, G.ch)):
        plane = pic[off:off + w * h].reshape(h // 8, 8, w // 8, 8).astype(np.float64)
        out.append(plane.mean(axis=(1, 3)))
    return out


def _distinct_blocks(seed):
    """every plane: a level per 8 x 8 block (a 2-D gradient plus a random offset), a gentle gradient and noise inside"""
    rng = np.random.default_rng(seed)
    planes = []
    for w, h in ((G.w, G.h), (G.cw, G.ch), (G.cw, G.ch)):
        by, bx = np.mgrid[0:h // 8, 0:w // 8]
        level = 40 + (3 * bx + 5 * by + rng.integers(0, 170, bx.shape)) % 170
        px = np.repeat(np.repeat(level, 8, 0), 8, 1)
        y, x = np.mgrid[0:h, 0:w]
        px = px + (x % 8) // 3 + (y % 8) // 3 + rng.integers(-3, 4, (h, w))
        planes.append(np.clip(px, 0, 255).astype(np.uint8).ravel())
    return np.concatenate(planes)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_statement_round_trip_keeps_every_block_in_place(flags):
    """DC survives the encoder's rate control: a block or plane put anywhere else (column 22's split chroma halves, the
    Cb / Cr order, a wrong shuffle) moves a mean by far more than 4"""
    pic = _distinct_blocks(flags)
    got = S.decode(S.SYS_625_50, S.encode(S.SYS_625_50, pic, flags))
    for i, (a, b) in enumerate(zip(_block_means(got), _block_means(pic))):
        d = np.abs(a - b)
        assert d.max() <= 4, (flags, i, float(d.max()), np.unravel_index(d.argmax(), d.shape))


def test_statement_decodes_arbitrary_bytes_deterministically():
    rng = np.random.default_rng(8)
    f = rng.integers(0, 256, G.frame_bytes, dtype=np.uint8)
    a, b = S.decode(S.SYS_625_50, f), S.decode(S.SYS_625_50, f.copy())
    assert a.size == G.picture_bytes and np.array_equal(a, b)
    assert not np.array_equal(a, S.decode(S.SYS_625_50, np.zeros(G.frame_bytes, np.uint8)))
