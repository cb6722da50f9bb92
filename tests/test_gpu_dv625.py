"""GPU parity of the DV25 625/50 (IEC 4:2:0) decoder — k_dv_decode<Sys625> through mi_dv_decode_batch_sys and
mi_dv_decode_frame_sys — against the test statement tests/dvsys.py (the unchanged oracle, segments moved), bit for bit;
the refusals of the one-frame path; 525/60 unchanged behind the new entry points; the plugin seam with the stream's
pixel format set (tests/harness/dv_stream_harness.c).  PARITY UNPINNED: see tests/dvsys.py."""
import ctypes as C
import hashlib
import importlib
import struct
import subprocess

import numpy as np
import pytest

import dvlib as D
import dvsys as S

pytestmark = pytest.mark.gpu
G = S.geometry(S.SYS_625_50)


@pytest.fixture(scope="module")
def dv():
    return importlib.import_module("gmerlin-avdecoder_amd.dv")


@pytest.fixture(scope="module")
def dev(dv):
    d = dv.MiDv(0)
    yield d
    d.close()


def same(dev, dv, frames):
    frames = np.ascontiguousarray(frames, np.uint8).reshape(-1, G.frame_bytes)
    got = dev.decode_frames(frames, system=dv.SYS_625_50)
    for i, f in enumerate(frames):
        S.differ(S.SYS_625_50, got[i], S.decode(S.SYS_625_50, f), f"frame {i}")


@pytest.mark.parametrize("amp,flags", [(0, 0), (4, 1), (8, 3), (16, 2), (40, 3), (90, 3)])
def test_encoded_625_frames_decode_like_the_statement(dev, dv, amp, flags):
    same(dev, dv, [S.encode(S.SYS_625_50, S.synth(S.SYS_625_50, n, 5 + amp, amp), flags) for n in range(2)])


def test_every_class_quantisation_number_and_mode_625(dev, dv):
    """header bits of encoded frames rewritten at random, in all 12 sequences"""
    rng = np.random.default_rng(7)
    frames = []
    for n in range(3):
        f = S.encode(S.SYS_625_50, S.synth(S.SYS_625_50, n, 9, 10), 3).copy()
        for seq in range(12):
            for v in range(135):
                o = D.video_block_offset(seq, v)
                f[o + 3] = rng.integers(0, 256)
                for a in D.AREA_OFF:
                    f[o + a + 1] = (f[o + a + 1] & 0x8F) | (rng.integers(0, 8) << 4)
        frames.append(f)
    same(dev, dv, frames)


def test_arbitrary_bytes_625(dev, dv):
    rng = np.random.default_rng(13)
    frames = rng.integers(0, 256, (4, G.frame_bytes), dtype=np.uint8)
    frames[1] = 0
    frames[2] = 0xFF
    same(dev, dv, frames)


@pytest.mark.parametrize("n", [1, 7, 64])
def test_batch_sizes_625(dev, dv, n):
    distinct = [S.encode(S.SYS_625_50, S.synth(S.SYS_625_50, i, 31, 4 + 3 * i), 3) for i in range(min(n, 4))]
    same(dev, dv, [distinct[i % len(distinct)] for i in range(n)])


def test_a_full_batch_of_1024_625_frames(dev, dv):
    distinct = [S.encode(S.SYS_625_50, S.synth(S.SYS_625_50, i, 17, 2 + 5 * (i % 8)), i % 4) for i in range(16)]
    want = [hashlib.sha256(S.decode(S.SYS_625_50, f).tobytes()).hexdigest() for f in distinct]
    frames = np.stack([distinct[i % 16] for i in range(1024)])
    got = dev.decode_frames(frames, system=dv.SYS_625_50)
    for i in range(1024):
        assert hashlib.sha256(got[i].tobytes()).hexdigest() == want[i % 16], i


def test_one_frame_path_625_with_padded_strides(dev, dv):
    f = S.encode(S.SYS_625_50, S.synth(S.SYS_625_50, 3, 4, 12), 3)
    want = S.decode(S.SYS_625_50, f)
    planes = dev.decode_frame(f, strides=(768, 400, 392), system=dv.SYS_625_50)
    assert np.array_equal(planes[0].reshape(576, 768)[:, :720].ravel(), want[:720 * 576])
    assert np.array_equal(planes[1].reshape(288, 400)[:, :360].ravel(), want[720 * 576:720 * 576 + 360 * 288])
    assert np.array_equal(planes[2].reshape(288, 392)[:, :360].ravel(), want[720 * 576 + 360 * 288:])
    # and again with the default strides, then a 525/60 frame on the same instance (its buffers are the larger ones now)
    planes = dev.decode_frame(f, system=dv.SYS_625_50)
    assert np.array_equal(np.concatenate(planes), want)
    f5 = D.encode(D.synth(1, 2, 6), 3)
    assert np.array_equal(np.concatenate(dev.decode_frame(f5)), D.decode(f5))


def test_one_frame_path_refusals(dev, dv):
    pal = S.encode(S.SYS_625_50, S.synth(S.SYS_625_50, 0, 1, 4), 0)
    ntsc = D.encode(D.synth(0, 1, 4), 0)
    apt = pal.copy()
    apt[5] |= 1  # DVCPRO 625/50 4:1:1
    with pytest.raises(dv.MiDvError, match="625/50"):
        dev.decode_frame(ntsc, system=dv.SYS_625_50)
    with pytest.raises(dv.MiDvError, match="not a 525/60"):
        dev.decode_frame(pal[:D.FRAME_BYTES], system=dv.SYS_525_60)
    with pytest.raises(dv.MiDvError, match="APT 1"):
        dev.decode_frame(apt, system=dv.SYS_625_50)
    with pytest.raises(dv.MiDvError, match="143999 bytes"):
        dev.decode_frame(pal[:143999], system=dv.SYS_625_50)
    assert np.array_equal(np.concatenate(dev.decode_frame(pal, system=dv.SYS_625_50)), S.decode(S.SYS_625_50, pal))  # still usable


def test_an_unknown_system_is_an_argument_error(dev, dv):
    L, c = dev.L, dev.c
    d_f, d_p = dev.alloc(G.frame_bytes), dev.alloc(G.picture_bytes)
    f = S.encode(S.SYS_625_50, S.synth(S.SYS_625_50, 0, 1, 4), 0)
    planes = [np.zeros(720 * 576, np.uint8) for _ in range(3)]
    pp = (dv.u8p * 3)(*[p.ctypes.data_as(dv.u8p) for p in planes])
    st = (C.c_int * 3)(720, 360, 360)
    x, y = C.c_int(), C.c_int()
    try:
        for system in (2, -1, 525, 625):
            assert L.mi_dv_decode_batch_sys(c, system, d_f, 1, d_p) == -1
            assert L.mi_dv_decode_frame_sys(c, system, f.ctypes.data_as(dv.u8p), f.nbytes, pp, st) == -1
            assert L.mi_dv_mb_place(system, 0, 0, 0, C.byref(x), C.byref(y)) == -1
    finally:
        dev.free(d_f)
        dev.free(d_p)


def test_525_through_the_new_entry_point_is_unchanged(dev, dv):
    frames = np.stack([D.encode(D.synth(n, 6, 3 + 4 * n), 3) for n in range(5)] +
                      [np.random.default_rng(2).integers(0, 256, D.FRAME_BYTES, dtype=np.uint8)])
    n = frames.shape[0]
    df, d1, d2 = dev.alloc(frames.nbytes), dev.alloc(n * D.PICTURE_BYTES), dev.alloc(n * D.PICTURE_BYTES)
    try:
        dev.h2d(df, frames)
        dev.kernel_times()
        dev.decode_batch(df, n, d1)
        dev.decode_batch_sys(dv.SYS_525_60, df, n, d2)
        dev.sync()
        ms, launches = dev.kernel_times()
        assert launches == 2 and ms > 0
        a, b = dev.d2h(d1, n * D.PICTURE_BYTES), dev.d2h(d2, n * D.PICTURE_BYTES)
        assert np.array_equal(a, b)
        assert np.array_equal(a[:D.PICTURE_BYTES], D.decode(frames[0]))
    finally:
        for d in (df, d1, d2):
            dev.free(d)


# ---- the plugin seam ----
def test_625_stream_through_the_plugin_seam(tmp_path):
    exe = S.harness()
    frames = [S.encode(S.SYS_625_50, S.synth(S.SYS_625_50, n, 8, 5 + n), 3) for n in range(6)]
    bad = D.encode(D.synth(0, 1, 4), 3)  # a 525/60 frame in the 625/50 stream
    pk, out = tmp_path / "p.bin", tmp_path / "o.bin"
    S.packets(pk, frames[:4] + [bad] + frames[4:])
    r = subprocess.run([exe, str(pk), "720", "576", "420", str(out), "skip_every=3", "pad=24"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "DV video decoder (MI355X)" in r.stderr and "format DV" in r.stderr and "frame 720x576" in r.stderr
    assert "625/50 frames have 144000" in r.stderr  # the foreign (short) frame ends the stream with a log line
    rec = G.picture_bytes + 8
    raw = np.fromfile(out, dtype=np.uint8)
    kept = [0, 1, 3]  # the 3rd packet is skipped, the 5th (the foreign frame) ends the stream
    assert raw.size == len(kept) * rec, r.stderr
    for i, k in enumerate(kept):
        assert np.array_equal(raw[i * rec:i * rec + G.picture_bytes], S.decode(S.SYS_625_50, frames[k])), k
        assert struct.unpack("<q", raw[i * rec + G.picture_bytes:(i + 1) * rec].tobytes())[0] == 1000 + 40 * k


def test_625_stream_ends_at_a_foreign_frame(tmp_path):
    exe = S.harness()
    frames = [S.encode(S.SYS_625_50, S.synth(S.SYS_625_50, n, 9, 6), 1) for n in range(3)]
    bad = np.concatenate([D.encode(D.synth(0, 1, 4), 3), np.zeros(G.frame_bytes - D.FRAME_BYTES, np.uint8)])  # DSF 0
    pk, out = tmp_path / "p.bin", tmp_path / "o.bin"
    S.packets(pk, frames[:2] + [bad] + frames[2:])
    r = subprocess.run([exe, str(pk), "720", "576", "420", str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and "not a 625/50" in r.stderr, r.stderr
    raw = np.fromfile(out, dtype=np.uint8)
    rec = G.picture_bytes + 8
    assert raw.size == 2 * rec
    for i in range(2):
        assert np.array_equal(raw[i * rec:i * rec + G.picture_bytes], S.decode(S.SYS_625_50, frames[i]))


@pytest.mark.parametrize("pixfmt", ["411", "none"])
def test_other_720x576_streams_are_declined(tmp_path, pixfmt):
    exe = S.harness()
    pk, out = tmp_path / "p.bin", tmp_path / "o.bin"
    S.packets(pk, [S.encode(S.SYS_625_50, S.synth(S.SYS_625_50, 0, 1, 4), 3)])
    r = subprocess.run([exe, str(pk), "720", "576", pixfmt, str(out)], capture_output=True, text=True)
    assert r.returncode == 3, r.stderr


def test_720x480_stream_still_decodes(tmp_path):
    exe = S.harness()
    frames = [D.encode(D.synth(n, 4, 6), 3) for n in range(3)]
    pk, out = tmp_path / "p.bin", tmp_path / "o.bin"
    S.packets(pk, frames)
    r = subprocess.run([exe, str(pk), "720", "480", "none", str(out), "pad=8"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "frame 720x480" in r.stderr
    rec = D.PICTURE_BYTES + 8
    raw = np.fromfile(out, dtype=np.uint8)
    assert raw.size == 3 * rec
    for i in range(3):
        assert np.array_equal(raw[i * rec:i * rec + D.PICTURE_BYTES], D.decode(frames[i]))
