"""GPU parity of the DVCPRO 625/50 4:1:1 decoder — k_dv_decode<Sys625_411> through mi_dv_decode_batch_sys and
mi_dv_decode_frame_sys with system 3 — against the test statement tests/dvsys.py (the unchanged oracle, segments
moved), bit for bit; the one-frame path's strides and its buffers across all five systems; its refusals; the float
statement's bounds of tests/golden/dv411p_float_bounds.json; the plugin seam with MI_DV_625_411=1 and without
(tests/harness/dv_stream_harness.c).  One frame is 162 waves; no launch here is larger than five frames.  PARITY
UNPINNED: see tests/dvsys.py."""
import ctypes as C
import functools
import importlib
import os
import struct
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

pytestmark = pytest.mark.gpu
YSZ, CSZ = 720 * 576, 180 * 576
ERR_FORMAT = -4
G = S.geometry(S.SYS_625_50_411)


@pytest.fixture(scope="module")
def dv():
    return importlib.import_module("gmerlin-avdecoder_amd.dv")


@pytest.fixture(scope="module")
def dev(dv):
    d = dv.MiDv(0)
    yield d
    d.close()


@functools.lru_cache(None)
def encoded(i):
    """frame i of the module's encoded frames and the checker's picture of it, made once"""
    amp, flags = [(0, 0), (8, 3), (16, 2), (40, 1), (90, 3)][i]
    f = S.encode(3, S.synth(3, i, 5 + amp, amp), flags)
    f.setflags(write=False)
    want = S.decode(3, f)
    want.setflags(write=False)
    return f, want


def differ(got, want, what):
    S.differ(S.SYS_625_50_411, got, want, what)


def same(dev, frames, what="frame"):
    frames = np.ascontiguousarray(frames, np.uint8).reshape(-1, G.frame_bytes)
    got = dev.decode_frames(frames, system=S.SYS_625_50_411)
    assert got.shape == (frames.shape[0], G.picture_bytes)
    for i, f in enumerate(frames):
        differ(got[i], S.decode(3, f), f"{what} {i}")


@pytest.mark.parametrize("n", [1, 2, 5])
def test_batches_fill_every_byte_of_every_picture(dev, dv, n):
    """into a buffer prefilled with 0xA5, with a guard behind the last picture: full coverage, the per-frame picture
    stride at blockIdx.y > 0, the 576-line chroma plane bases"""
    frames = np.stack([encoded(i)[0] for i in range(n)])
    guard = 4096
    df, dp = dev.alloc(n * G.frame_bytes), dev.alloc(n * G.picture_bytes + guard)
    try:
        dev.h2d(df, frames)
        dev.h2d(dp, np.full(n * G.picture_bytes + guard, 0xA5, np.uint8))
        dev.kernel_times()
        dev.decode_batch_sys(dv.SYS_625_50_411, df, n, dp)
        dev.sync()
        ms, launches = dev.kernel_times()
        assert launches == 1 and ms > 0
        got = dev.d2h(dp, n * G.picture_bytes + guard)
    finally:
        dev.free(df)
        dev.free(dp)
    assert (got[n * G.picture_bytes:] == 0xA5).all()
    for i in range(n):
        differ(got[i * G.picture_bytes:(i + 1) * G.picture_bytes], encoded(i)[1], f"batch of {n}, frame {i}")


@pytest.mark.parametrize("region", ["bottom", "right"])
def test_detail_only_where_the_layout_differs_from_525_60(dev, region):
    """lines 480..575 alone (rows taken modulo 12, not 10), columns 704..719 alone (the split chroma halves at the plane
    bases of a 576-line picture)"""
    f = S.encode(3, S.synth(3, 2, 11, 10, region=region), 3)
    want = S.decode(3, f)
    Y = want[:YSZ].reshape(576, 720).astype(int)
    part = Y[480:] if region == "bottom" else Y[:, 704:]
    rest = Y[:480] if region == "bottom" else Y[:, :704]
    assert part.std() > 10 and np.abs(rest - 128).max() <= 2  # the checker's picture has its detail there and only there
    same(dev, f, region)


def test_every_class_quantisation_number_and_mode_411p(dev):
    """header bits of an encoded frame rewritten at random, in all 12 sequences"""
    rng = np.random.default_rng(7)
    f = encoded(2)[0].copy()
    for seq in range(12):
        for v in range(135):
            o = D.video_block_offset(seq, v)
            f[o + 3] = rng.integers(0, 256)
            for a in D.AREA_OFF:
                f[o + a + 1] = (f[o + a + 1] & 0x8F) | (rng.integers(0, 8) << 4)
    same(dev, f, "rewritten")


def test_arbitrary_bytes_with_a_valid_header(dev, dv):
    """blocks that end in passes 2 and 3, or never"""
    rng = np.random.default_rng(13)
    frames = rng.integers(0, 256, (3, G.frame_bytes), dtype=np.uint8)
    frames[2, ::3] = 0xFF
    for f in frames:
        S.header(3, f)
        assert dv.kind_of(f) == 3
    same(dev, frames, "arbitrary")


def _decode_one(dev, dv, system, frame, strides, heights, fill=0x5A):
    planes = [np.full(strides[i] * heights[i], fill, np.uint8) for i in range(3)]
    pp = (dv.u8p * 3)(*[p.ctypes.data_as(dv.u8p) for p in planes])
    st = (C.c_int * 3)(*strides)
    frame = np.ascontiguousarray(frame, np.uint8)
    rc = dev.L.mi_dv_decode_frame_sys(dev.c, system, frame.ctypes.data_as(dv.u8p), frame.nbytes, pp, st)
    return rc, planes, dev.L.mi_dv_last_error(dev.c).decode()


@pytest.mark.parametrize("strides", [(720, 180, 180), (768, 200, 192)])
def test_one_frame_path_with_tight_and_padded_strides(dev, dv, strides):
    f, want = encoded(1)
    rc, planes, msg = _decode_one(dev, dv, dv.SYS_625_50_411, f, strides, (576, 576, 576))
    assert rc == 0, msg
    for pl, (off, w) in enumerate(((0, 720), (YSZ, 180), (YSZ + CSZ, 180))):
        rows = planes[pl].reshape(576, strides[pl])
        differ(rows[:, :w].ravel(), want[off:off + w * 576], f"plane {pl}")
        assert (rows[:, w:] == 0x5A).all(), f"plane {pl}: the bytes between rows were written"
    differ(np.concatenate(dev.decode_frame(f, system=dv.SYS_625_50_411)), want, "default strides")
    with pytest.raises(dv.MiDvError, match="strides below"):
        dev.decode_frame(f, strides=(720, 179, 180), system=dv.SYS_625_50_411)


def test_all_five_systems_interleaved_on_one_instance(dv):
    frames = {0: D.encode(D.synth(1, 2, 6), 3), 1: S.encode(1, S.synth(1, 1, 2, 6), 3), 3: encoded(1)[0],
              4: S.encode(4, S.synth(4, 2, 3, 9), 3), 5: S.encode(5, S.synth(5, 2, 3, 9), 3)}
    want = {0: D.decode(frames[0]), 1: S.decode(1, frames[1]), 3: encoded(1)[1], 4: S.decode(4, frames[4]),
            5: S.decode(5, frames[5])}
    d = dv.MiDv(0)  # a fresh instance: its buffers grow with the systems it sees, in this order
    try:
        for system in (3, 0, 5, 3, 1, 4, 3, 0, 1):
            differ(np.concatenate(d.decode_frame(frames[system], system=system)), want[system], f"system {system}")
    finally:
        d.close()


def test_one_frame_path_refusals(dev, dv):
    f, want = encoded(0)
    heights = (576, 576, 576)
    pal420 = S.encode(1, S.synth(1, 0, 1, 4), 0)  # 625/50, APT 0
    ntsc = D.encode(D.synth(0, 1, 4), 0)
    rc, _, msg = _decode_one(dev, dv, 3, pal420, (720, 180, 180), heights)
    assert rc == ERR_FORMAT and "4:1:1" in msg and "DSF 1, APT 0, stype 0x00" in msg, (rc, msg)
    rc, _, msg = _decode_one(dev, dv, 3, ntsc, (720, 180, 180), heights)
    assert rc == ERR_FORMAT and "120000 bytes" in msg and "144000" in msg, (rc, msg)
    rc, _, msg = _decode_one(dev, dv, 3, np.concatenate([ntsc, np.zeros(24000, np.uint8)]), (720, 180, 180), heights)
    assert rc == ERR_FORMAT and "DSF 0" in msg, (rc, msg)
    rc, planes, msg = _decode_one(dev, dv, 3, f[:143999], (720, 180, 180), heights)
    assert rc == ERR_FORMAT and "143999 bytes" in msg, (rc, msg)
    assert all((p == 0x5A).all() for p in planes)  # a refused frame writes nothing
    rc, _, msg = _decode_one(dev, dv, 3, S.encode(5, S.synth(5, 0, 1, 4), 0), (720, 180, 180), heights)
    assert rc == ERR_FORMAT and "stype 0x04" in msg, (rc, msg)
    with pytest.raises(dv.MiDvError, match="APT 1"):  # and a 4:1:1 frame is still no 625/50 4:2:0 frame
        dev.decode_frame(f, system=dv.SYS_625_50)
    with pytest.raises(dv.MiDvError, match="not a 525/60"):
        dev.decode_frame(f, system=dv.SYS_525_60)
    differ(np.concatenate(dev.decode_frame(f, system=3)), want, "afterwards")  # still usable


def test_kernel_times_count_the_launches(dev, dv):
    f, want = encoded(3)
    df, dp = dev.alloc(G.frame_bytes), dev.alloc(G.picture_bytes)
    try:
        dev.h2d(df, f)
        dev.kernel_times()
        for _ in range(3):
            dev.decode_batch_sys(3, df, 1, dp)
        dev.decode_frame(f, system=3)
        ms, launches = dev.kernel_times()
        assert launches == 4 and ms > 0
        assert dev.kernel_times() == (0.0, 0)
        differ(dev.d2h(dp, G.picture_bytes), want, "batch of 1")
    finally:
        dev.free(df)
        dev.free(dp)


@pytest.mark.parametrize("family", list(M.FAMILIES))
def test_the_kernel_stays_within_the_float_bounds(dev, family):
    """one frame of each family: the oracle's picture bit for bit, and the float statement's within the bound the oracle
    itself keeps on the CPU — the same number, no margin"""
    frame, want, pic, out = M.reference(family, M.COUNT[family] - 1)
    assert out == 0
    got = dev.decode_frames(frame[None], system=3)[0]
    differ(got, want, f"family {family}")
    d = F.deviation(got, pic)
    b = M.bounds()["bounds"]["frames"][family]
    print(family, float(np.abs(d).max()), float(d.mean()))
    assert np.abs(d).max() <= b["abs"], (family, float(np.abs(d).max()), int(np.abs(d).argmax()))
    assert abs(d.mean()) <= b["mean"], (family, float(d.mean()))


# ---- the plugin seam ----
def _env(opt):
    env = {k: v for k, v in os.environ.items() if k != "MI_DV_625_411"}
    if opt is not None:
        env["MI_DV_625_411"] = opt
    return env


def test_411p_stream_through_the_plugin_seam_when_opted_in(tmp_path):
    exe = S.harness()
    frames = [encoded(i)[0] for i in range(4)]
    foreign = S.encode(1, S.synth(1, 0, 1, 4), 3)  # a 625/50 4:2:0 frame (APT 0) in the stream
    pk, out = tmp_path / "p.bin", tmp_path / "o.bin"
    S.packets(pk, frames + [foreign])
    r = subprocess.run([exe, str(pk), "720", "576", "411", str(out), "skip_every=3", "pad=24"], capture_output=True, text=True,
                       env=_env("1"))
    assert r.returncode == 0, r.stderr
    assert "DV video decoder (MI355X)" in r.stderr and "format DV" in r.stderr and "frame 720x576" in r.stderr
    assert "chroma 180x576" in r.stderr  # the pixel format stayed GAVL_YUV_411_P
    assert "not a 625/50 25 Mbit/s 4:1:1" in r.stderr and "APT 0" in r.stderr  # the foreign frame ends the stream with a log line
    rec = G.picture_bytes + 8
    raw = np.fromfile(out, dtype=np.uint8)
    kept = [0, 1, 3]  # the 3rd packet is skipped (and consumed), the 5th (the foreign frame) ends the stream
    assert raw.size == len(kept) * rec, r.stderr
    for i, k in enumerate(kept):
        differ(raw[i * rec:i * rec + G.picture_bytes], encoded(k)[1], f"packet {k}")
        assert struct.unpack("<q", raw[i * rec + G.picture_bytes:(i + 1) * rec].tobytes())[0] == 1000 + 40 * k


@pytest.mark.parametrize("opt", [None, "0", "yes"])
def test_the_same_stream_is_declined_without_the_opt_in(tmp_path, opt):
    exe = S.harness()
    pk, out = tmp_path / "p.bin", tmp_path / "o.bin"
    S.packets(pk, [encoded(0)[0]])
    r = subprocess.run([exe, str(pk), "720", "576", "411", str(out)], capture_output=True, text=True, env=_env(opt))
    assert r.returncode == 3, r.stderr


def test_a_420_stream_still_opens_as_625_50_when_opted_in(tmp_path):
    exe = S.harness()
    frames = [S.encode(1, S.synth(1, n, 8, 5 + n), 3) for n in range(2)]
    pk, out = tmp_path / "p.bin", tmp_path / "o.bin"
    S.packets(pk, frames)
    r = subprocess.run([exe, str(pk), "720", "576", "420", str(out)], capture_output=True, text=True, env=_env("1"))
    assert r.returncode == 0 and "frame 720x576" in r.stderr and "chroma 360x288" in r.stderr, r.stderr
    rec = S.geometry(1).picture_bytes + 8
    raw = np.fromfile(out, dtype=np.uint8)
    assert raw.size == 2 * rec
    for i in range(2):
        assert np.array_equal(raw[i * rec:i * rec + S.geometry(1).picture_bytes], S.decode(1, frames[i]))
