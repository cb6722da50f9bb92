"""DVCPRO 625/50 4:1:1 (system 3) without a GPU: the kernels' macroblock placement (mi_dv_mb_place) against the test
statement (tests/dvsys.py); the host-side check over all five decodable profiles (mi_dv_kind_of) next to the two older
ones, which stay as they were; the statement's own round trip; the fixed-point oracle against the float statement in
this layout, within tests/golden/dv411p_float_bounds.json.  PARITY UNPINNED: both statements of the layout are this
repository's reading of SMPTE 314M, from memory."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import dvfloat as F
import dvlib as D
import dvsys as S
from pkg import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_dv411p_float_bounds as M  # noqa: E402

ERR_ARG = -1
G = S.geometry(S.SYS_625_50_411)


@pytest.fixture(scope="module")
def dv():
    return importlib.import_module("gmerlin-avdecoder_amd.dv")


def _c_place(dv, system, seq, slot, m):
    x, y = C.c_int(-7), C.c_int(-7)
    return dv.load().mi_dv_mb_place(system, seq, slot, m, C.byref(x), C.byref(y)), (x.value, y.value)


def test_the_python_view_states_the_same_geometry(dv):
    assert dv.SYS_625_50_411 == S.SYS_625_50_411 == 3
    assert dv.geometry(3) == (G.frame_bytes, G.picture_bytes, ((720, 576), (180, 576), (180, 576)))
    assert (G.frame_bytes, G.picture_bytes, G.segments, G.macroblocks) == (144000, 622080, 324, 1620)


def test_411p_placement_is_the_statements_for_all_1620_macroblocks(dv):
    seen = set()
    for seq in range(12):
        for slot in range(27):
            for m in range(5):
                rc, xy = _c_place(dv, 3, seq, slot, m)
                assert rc == 0 and xy == S.mb_place(3, seq, slot, m), (seq, slot, m, rc, xy)
                assert dv.place_of(3, seq, slot, m) == xy
                assert 0 <= xy[0] <= 22 and 0 <= xy[1] <= (70 if xy[0] == 22 else 71)
                seen.add(xy)
    assert len(seen) == 1620 and max(y for _, y in seen) == 71


@pytest.mark.parametrize("args", [(12, 0, 0), (0, 27, 0), (0, 0, 5), (-1, 0, 0), (0, -1, 0), (0, 0, -1)])
def test_411p_placement_refuses_what_is_out_of_range(dv, args):
    rc, xy = _c_place(dv, 3, *args)
    assert rc == ERR_ARG and xy == (-7, -7)
    with pytest.raises(dv.MiDvError, match="out of range"):
        dv.place_of(3, *args)
    assert _c_place(dv, 3, 11, 26, 4)[0] == 0  # the last macroblock of the last sequence is in range
    assert _c_place(dv, 2, 0, 0, 0)[0] == ERR_ARG  # and 2 stays no system


def test_525_placement_is_unchanged_for_its_1350_macroblocks(dv):
    L = D.lib()
    for seq in range(10):
        for slot in range(27):
            for m in range(5):
                x, y = C.c_int(), C.c_int()
                L.dvo_mb_place(seq, slot, m, C.byref(x), C.byref(y))
                assert dv.mb_place(dv.SYS_525_60, seq, slot, m) == (x.value, y.value) == dv.place_of(0, seq, slot, m)
    assert _c_place(dv, 0, 10, 0, 0)[0] == ERR_ARG  # 525/60 has ten sequences, as before


def test_the_statements_blocks_tile_the_picture_exactly_once():
    src, dst, here, b525 = S.maps(3)  # asserts the tiling itself
    assert dst.size == src.size == G.picture_bytes and np.array_equal(np.sort(dst), np.arange(G.picture_bytes))
    assert here.size == b525.size == 1620 * 80
    # lines 480..575 and columns 704..719 are reached (what 525/60 has not, and what it has at another plane base)
    hit = np.zeros(G.picture_bytes, bool)
    hit[dst] = True
    assert hit[:720 * 576].reshape(576, 720)[480:, :].all() and hit[:720 * 576].reshape(576, 720)[:, 704:].all()


@pytest.fixture(scope="module")
def dvframe():
    from test_dvframe_host import Profile  # the struct of include/mi_dvframe.h
    subprocess.run(["make", "-C", os.path.join(ROOT, "gmerlin-avdecoder_amd", "csrc"),
                    os.path.join(ROOT, "gmerlin-avdecoder_amd", "lib", "libmi_dvframe.so")], check=True, capture_output=True)
    lib = C.CDLL(os.path.join(ROOT, "gmerlin-avdecoder_amd", "lib", "libmi_dvframe.so"))
    lib.mi_dv_profile_at.restype = C.POINTER(Profile)
    return lib


def test_kind_of_every_profile_and_every_apt(dv, dvframe):
    from test_dvframe_host import make_frame
    rng = np.random.default_rng(11)
    assert dvframe.mi_dv_num_profiles() == 9
    threes = 0
    for i in range(9):
        p = dvframe.mi_dv_profile_at(i).contents
        for apt in range(8):
            f = make_frame(p, rng, apt=apt)
            is411 = p.dsf == 1 and p.video_stype == 0 and apt != 0
            if is411:
                assert p.frame_size == 144000
                want = 3
                assert dv.profile_of(f) == -1 and dv.system_of(f) == -1  # the older queries stay as they were
                threes += 1
            else:
                want = dv.profile_of(f)
            assert dv.kind_of(f) == want, (i, apt)
            assert dv.kind_of(f[:p.frame_size - 1]) == -1, (i, apt)  # a frame shorter than its system's
            assert dv.kind_of(f[:400]) == -1, (i, apt)
            if dv.profile_of(f) >= 0:
                assert dv.kind_of(f) == dv.profile_of(f), (i, apt)
            assert dv.kind_of(f) in (-1, 0, 1, 3, 4, 5)
    assert threes == 2 * 7  # the two 25 Mbit/s 625/50 profiles of the table (4:2:0 and 4:1:1 differ in APT alone) x APT 1..7
    p = dvframe.mi_dv_profile_at(2).contents  # DVCPRO 625/50 4:1:1 itself
    f = make_frame(p, rng, apt=1)
    assert dv.kind_of(f) == 3 and dv.kind_of(f[:143999]) == -1 and dv.kind_of(f[:120000]) == -1
    assert dv.kind_of(np.zeros(0, np.uint8)) == -1


def test_statement_frames_announce_kind_3(dv):
    f = S.encode(3, S.synth(3, 0, 2, 6), 3)
    assert f.size == G.frame_bytes and dv.kind_of(f) == 3 and dv.profile_of(f) == -1 and dv.system_of(f) == -1
    assert f[3] >> 7 == 1 and f[5] & 7 == 1 and f[80 * 5 + 48 + 3] & 0x1F == 0
    blocks = f.reshape(12, 150, 80)
    for seq in range(12):
        assert (blocks[seq, :, 1] >> 4 == seq).all()


def test_synth_puts_detail_where_the_layout_differs_from_525_60():
    for region, ys, xs, cys, cxs in (("bottom", slice(480, 576), slice(0, 720), slice(480, 576), slice(0, 180)),
                                     ("right", slice(0, 576), slice(704, 720), slice(0, 576), slice(176, 180))):
        pic = S.synth(3, 1, 3, 6, region=region)
        Y = pic[:720 * 576].reshape(576, 720)
        cb = pic[720 * 576:720 * 576 + 180 * 576].reshape(576, 180)
        cr = pic[720 * 576 + 180 * 576:].reshape(576, 180)
        for plane, rs, cs in ((Y, ys, xs), (cb, cys, cxs), (cr, cys, cxs)):
            inside = np.zeros(plane.shape, bool)
            inside[rs, cs] = True
            assert (plane[~inside] == 128).all() and plane[inside].std() > 4, region
    full = S.synth(3, 1, 3, 6)[:720 * 576].reshape(576, 720)
    assert full[480:].std() > 20 and full[:, 704:].std() > 20


def _distinct_blocks(seed):
    """every plane: a level per 8 x 8 block (a 2-D gradient plus a random offset), a gentle gradient and noise inside
    (tests/test_dv625_cpu.py's picture at this system's plane sizes)"""
    rng = np.random.default_rng(seed)
    planes = []
    for w, h in ((G.w, G.h), (G.cw, G.ch), (G.cw, G.ch)):
        by, bx = np.mgrid[0:h // 8, 0:(w + 7) // 8]
        level = 40 + (3 * bx + 5 * by + rng.integers(0, 170, bx.shape)) % 170
        px = np.repeat(np.repeat(level, 8, 0), 8, 1)[:, :w]
        y, x = np.mgrid[0:h, 0:w]
        px = px + (x % 8) // 3 + (y % 8) // 3 + rng.integers(-3, 4, (h, w))
        planes.append(np.clip(px, 0, 255).astype(np.uint8).ravel())
    return np.concatenate(planes)


def _block_means(pic):
    """the mean of every coded block: 8 x 8 everywhere, and the 4 x 8 halves of the split chroma blocks of column 22
    (chroma columns 176..179) one half at a time — a half is all that lies in one place there"""
    out = []
    Y = pic[:G.w * G.h].reshape(G.h // 8, 8, G.w // 8, 8).astype(np.float64)
    out.append(Y.mean(axis=(1, 3)))
    for off in (G.w * G.h, G.w * G.h + G.cw * G.ch):
        plane = pic[off:off + G.cw * G.ch].reshape(G.ch, G.cw).astype(np.float64)
        out.append(plane[:, :176].reshape(G.ch // 8, 8, 22, 8).mean(axis=(1, 3)))
        out.append(plane[:, 176:].reshape(G.ch // 8, 8, 4).mean(axis=(1, 2)))
    return out


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_statement_round_trip_keeps_every_block_in_place(flags):
    """DC survives the encoder's rate control: a block or plane put anywhere else (a row taken modulo 10, column 22's
    split chroma halves at the 480-line plane base, the Cb / Cr order, a wrong shuffle) moves a mean by far more than 4"""
    pic = _distinct_blocks(30 + flags)
    got = S.decode(3, S.encode(3, pic, flags))
    worst = 0.0
    for i, (a, b) in enumerate(zip(_block_means(got), _block_means(pic))):
        d = np.abs(a - b)
        worst = max(worst, float(d.max()))
        assert d.max() <= 4, (flags, i, float(d.max()), np.unravel_index(d.argmax(), d.shape))
    print(f"flags {flags}: largest block-mean deviation {worst:.3f}")


def test_statement_decodes_arbitrary_bytes_deterministically():
    rng = np.random.default_rng(8)
    f = rng.integers(0, 256, G.frame_bytes, dtype=np.uint8)
    a, b = S.decode(3, f), S.decode(3, f.copy())
    assert a.size == G.picture_bytes and a.dtype == np.uint8 and np.array_equal(a, b)
    assert not np.array_equal(a, S.decode(3, np.zeros(G.frame_bytes, np.uint8)))


# ---- the fixed-point oracle against the float statement, in this layout ----
@pytest.mark.parametrize("family", list(M.FAMILIES))
def test_whole_frames_stay_within_the_float_bounds(family):
    b = M.bounds()["bounds"]["frames"][family]
    for i, (frame, got, pic, out) in enumerate(M.references(family)):
        assert out == 0, f"frame {i}: {out} blocks outside the fixed-point range"
        d = F.deviation(got, pic)
        print(family, i, float(np.abs(d).max()), float(d.mean()))
        assert np.abs(d).max() <= b["abs"], (i, float(np.abs(d).max()), int(np.abs(d).argmax()))
        assert abs(d.mean()) <= b["mean"], (i, float(d.mean()))


def test_the_maker_reproduces_the_committed_bounds_byte_for_byte():
    with open(M.BOUNDS) as f:
        committed = f.read()
    assert M.text() == committed
    B = json.loads(committed)
    assert B["system"] == 3 and B["seeds"] == F.SEEDS and [tuple(p) for p in B["pictures"]] == M.PICTURES
    for fam, m in B["measured"]["frames"].items():
        assert m["abs"] <= B["bounds"]["frames"][fam]["abs"] < m["abs"] + B["step"]["abs"] + 1e-9

