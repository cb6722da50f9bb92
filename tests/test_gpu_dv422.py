"""GPU parity of the 50 Mbit/s 4:2:2 DV decoder — k_dv_decode<Sys525_422> and <Sys625_422> through
mi_dv_decode_batch_sys and mi_dv_decode_frame_sys — against the test statement tests/dvsys.py (the unchanged oracle,
segments moved, areas 1 and 3 dropped), bit for bit; the one-frame path's buffers across all four systems; its refusals;
the plugin seam with the stream's pixel format set to 4:2:2 (tests/harness/dv_stream_harness.c).  PARITY UNPINNED: see
tests/dvsys.py."""
import hashlib
import importlib
import struct
import subprocess

import numpy as np
import pytest

import dvlib as D
import dvsys as P

pytestmark = pytest.mark.gpu
SYSTEMS = [P.SYS_525_60_422, P.SYS_625_50_422]


@pytest.fixture(scope="module")
def dv():
    return importlib.import_module("gmerlin-avdecoder_amd.dv")


@pytest.fixture(scope="module")
def dev(dv):
    d = dv.MiDv(0)
    yield d
    d.close()


def same(dev, system, frames):
    g = P.geometry(system)
    frames = np.ascontiguousarray(frames, np.uint8).reshape(-1, g.frame_bytes)
    got = dev.decode_frames(frames, system=system)
    assert got.shape == (frames.shape[0], g.picture_bytes)
    for i, f in enumerate(frames):
        P.differ(system, got[i], P.decode(system, f), f"frame {i}")


@pytest.mark.parametrize("system", SYSTEMS)
@pytest.mark.parametrize("amp,flags", [(0, 0), (4, 1), (8, 3), (16, 2), (40, 3), (90, 3)])
def test_encoded_422_frames_decode_like_the_statement(dev, system, amp, flags):
    same(dev, system, [P.encode(system, P.synth(system, n, 5 + amp, amp), flags) for n in range(2)])


@pytest.mark.parametrize("system", SYSTEMS)
def test_every_class_quantisation_number_and_mode_422(dev, system):
    """header bits of encoded frames rewritten at random in all six areas (1 and 3 included), in every sequence of both
    channels"""
    g = P.geometry(system)
    rng = np.random.default_rng(7 + system)
    frames = []
    for n in range(3):
        f = P.encode(system, P.synth(system, n, 9, 10), 3).copy()
        for seq in range(g.frame_seqs):
            for v in range(135):
                o = D.video_block_offset(seq, v)
                f[o + 3] = rng.integers(0, 256)
                for a in D.AREA_OFF:
                    f[o + a + 1] = (f[o + a + 1] & 0x8F) | (rng.integers(0, 8) << 4)
        frames.append(f)
    same(dev, system, frames)


@pytest.mark.parametrize("system", SYSTEMS)
def test_arbitrary_bytes_422(dev, system):
    """random, all zero, all 0xFF; and random with areas 1 and 3 of every macroblock filled with 16-bit code words, which
    never finish their blocks: those take bits in passes 2 and 3 like any block, and nothing of them reaches the picture"""
    g = P.geometry(system)
    rng = np.random.default_rng(13 + system)
    frames = rng.integers(0, 256, (5, g.frame_bytes), dtype=np.uint8)
    frames[1] = 0
    frames[2] = 0xFF
    for k in (3, 4):
        for seq in range(g.frame_seqs):
            for v in range(135):
                o = D.video_block_offset(seq, v)
                for a in (D.AREA_OFF[1], D.AREA_OFF[3]):
                    frames[k, o + a + 1] |= 0x0F
                    frames[k, o + a + 2:o + a + 14] = 0xFF if k == 3 else rng.integers(0xFE, 0x100, 12)
    same(dev, system, frames)


@pytest.mark.parametrize("system", SYSTEMS)
@pytest.mark.parametrize("n", [1, 7, 64])
def test_batch_sizes_422(dev, system, n):
    distinct = [P.encode(system, P.synth(system, i, 31, 4 + 3 * i), 3) for i in range(min(n, 4))]
    same(dev, system, [distinct[i % len(distinct)] for i in range(n)])


@pytest.mark.parametrize("system", SYSTEMS)
def test_a_full_batch_of_1024_422_frames(dev, system):
    distinct = [P.encode(system, P.synth(system, i, 17, 2 + 5 * (i % 8)), i % 4) for i in range(16)]
    want = [hashlib.sha256(P.decode(system, f).tobytes()).hexdigest() for f in distinct]
    assert len(set(want)) == 16
    frames = np.stack([distinct[i % 16] for i in range(1024)])
    dev.kernel_times()
    got = dev.decode_frames(frames, system=system)
    ms, launches = dev.kernel_times()
    assert launches == 1 and ms > 0  # the same events as every other system's launches
    for i in range(1024):
        assert hashlib.sha256(got[i].tobytes()).hexdigest() == want[i % 16], i


@pytest.mark.parametrize("system", SYSTEMS)
def test_one_frame_path_422_with_padded_strides_then_every_other_system(dv, system):
    g = P.geometry(system)
    other = P.SYS_625_50_422 if system == P.SYS_525_60_422 else P.SYS_525_60_422
    d = dv.MiDv(0)  # a fresh instance: its buffers grow with the systems it sees, in this order
    try:
        f = P.encode(system, P.synth(system, 3, 4, 12), 3)
        want = P.decode(system, f)
        ysz, csz = 720 * g.h, 360 * g.h
        planes = d.decode_frame(f, strides=(768, 400, 392), system=system)
        assert np.array_equal(planes[0].reshape(g.h, 768)[:, :720].ravel(), want[:ysz])
        assert np.array_equal(planes[1].reshape(g.h, 400)[:, :360].ravel(), want[ysz:ysz + csz])
        assert np.array_equal(planes[2].reshape(g.h, 392)[:, :360].ravel(), want[ysz + csz:])
        assert np.array_equal(np.concatenate(d.decode_frame(f, system=system)), want)  # the default strides
        f5 = D.encode(D.synth(1, 2, 6), 3)
        assert np.array_equal(np.concatenate(d.decode_frame(f5)), D.decode(f5))
        f6 = P.encode(P.SYS_625_50, P.synth(P.SYS_625_50, 1, 2, 6), 3)
        assert np.array_equal(np.concatenate(d.decode_frame(f6, system=dv.SYS_625_50)), P.decode(P.SYS_625_50, f6))
        fo = P.encode(other, P.synth(other, 2, 3, 9), 3)
        assert np.array_equal(np.concatenate(d.decode_frame(fo, system=other)), P.decode(other, fo))
        assert np.array_equal(np.concatenate(d.decode_frame(f, system=system)), want)  # and the first one again
    finally:
        d.close()


@pytest.mark.parametrize("system", SYSTEMS)
def test_one_frame_path_refusals_422(dev, dv, system):
    g = P.geometry(system)
    name = "625/50" if g.dsf else "525/60"
    f = P.encode(system, P.synth(system, 0, 1, 4), 0)
    dv25 = P.encode(P.SYS_625_50, P.synth(P.SYS_625_50, 0, 1, 4), 0) if g.dsf else D.encode(D.synth(0, 1, 4), 0)
    # a DV25 frame offered as 4:2:2: too short as it is; long enough, it does not announce the system
    with pytest.raises(dv.MiDvError, match=f"{dv25.size} bytes: {name} 50 Mbit/s 4:2:2 frames have {g.frame_bytes}"):
        dev.decode_frame(dv25, system=system)
    padded = np.concatenate([dv25, np.zeros(g.frame_bytes - dv25.size, np.uint8)])
    with pytest.raises(dv.MiDvError, match=rf"not a {name} 50 Mbit/s 4:2:2 DV frame of {g.frame_bytes} bytes \(DSF {g.dsf}, stype 0x00"):
        dev.decode_frame(padded, system=system)
    # a 4:2:2 frame offered as DV25
    with pytest.raises(dv.MiDvError, match="not a 525/60"):
        dev.decode_frame(f, system=dv.SYS_525_60)
    with pytest.raises(dv.MiDvError, match="not a 625/50 25 Mbit/s"):
        dev.decode_frame(f, system=dv.SYS_625_50)
    # the wrong DSF (long enough for either system)
    wrong = np.concatenate([f, np.zeros(288000 - f.size, np.uint8)])
    wrong[3] ^= 0x80
    with pytest.raises(dv.MiDvError, match=f"DSF {1 - g.dsf}, stype 0x04; expected DSF {g.dsf}"):
        dev.decode_frame(wrong, system=system)
    # one byte short
    with pytest.raises(dv.MiDvError, match=f"{g.frame_bytes - 1} bytes"):
        dev.decode_frame(f[:g.frame_bytes - 1], system=system)
    assert np.array_equal(np.concatenate(dev.decode_frame(f, system=system)), P.decode(system, f))  # still usable


# ---- the plugin seam ----
@pytest.mark.parametrize("system", SYSTEMS)
def test_422_stream_through_the_plugin_seam(tmp_path, system):
    """the 720 x 480 case is a DVCPRO50 stream of the 525/60 system: before the 4:2:2 systems existed the plugin took it
    for 4:1:1 and delivered no frame"""
    g = P.geometry(system)
    exe = P.harness()
    frames = [P.encode(system, P.synth(system, n, 8, 5 + n), 3) for n in range(6)]
    bad = D.encode(D.synth(0, 1, 4), 3)  # a 525/60 25 Mbit/s frame in the stream
    pk, out = tmp_path / "p.bin", tmp_path / "o.bin"
    P.packets(pk, frames[:4] + [bad] + frames[4:])
    r = subprocess.run([exe, str(pk), "720", str(g.h), "422", str(out), "skip_every=3", "pad=24"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "DV video decoder (MI355X)" in r.stderr and "format DV" in r.stderr and f"frame 720x{g.h}" in r.stderr
    assert f"4:2:2 frames have {g.frame_bytes}" in r.stderr  # the foreign (short) frame ends the stream with a log line
    rec = g.picture_bytes + 8
    raw = np.fromfile(out, dtype=np.uint8)
    kept = [0, 1, 3]  # the 3rd packet is skipped, the 5th (the foreign frame) ends the stream
    assert raw.size == len(kept) * rec, r.stderr
    for i, k in enumerate(kept):
        assert np.array_equal(raw[i * rec:i * rec + g.picture_bytes], P.decode(system, frames[k])), k
        assert struct.unpack("<q", raw[i * rec + g.picture_bytes:(i + 1) * rec].tobytes())[0] == 1000 + 40 * k


@pytest.mark.parametrize("system", SYSTEMS)
def test_422_stream_ends_at_a_frame_of_the_other_line_system(tmp_path, system):
    g = P.geometry(system)
    other = P.SYS_625_50_422 if system == P.SYS_525_60_422 else P.SYS_525_60_422
    exe = P.harness()
    frames = [P.encode(system, P.synth(system, n, 9, 6), 1) for n in range(3)]
    bad = P.encode(other, P.synth(other, 0, 1, 4), 3)
    bad = np.concatenate([bad, np.zeros(max(0, g.frame_bytes - bad.size), np.uint8)])
    pk, out = tmp_path / "p.bin", tmp_path / "o.bin"
    P.packets(pk, frames[:2] + [bad] + frames[2:])
    r = subprocess.run([exe, str(pk), "720", str(g.h), "422", str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and "50 Mbit/s 4:2:2 DV frame" in r.stderr and f"DSF {1 - g.dsf}" in r.stderr, r.stderr
    raw = np.fromfile(out, dtype=np.uint8)
    rec = g.picture_bytes + 8
    assert raw.size == 2 * rec
    for i in range(2):
        assert np.array_equal(raw[i * rec:i * rec + g.picture_bytes], P.decode(system, frames[i]))


@pytest.mark.parametrize("args,code", [(("720", "576", "411"), 3), (("720", "576", "none"), 3), (("704", "480", "422"), 3),
                                       (("720", "486", "422"), 3)])
def test_streams_that_are_not_ours_are_still_declined(tmp_path, args, code):
    exe = P.harness()
    pk, out = tmp_path / "p.bin", tmp_path / "o.bin"
    P.packets(pk, [P.encode(P.SYS_625_50, P.synth(P.SYS_625_50, 0, 1, 4), 3)])
    r = subprocess.run([exe, str(pk), *args, str(out)], capture_output=True, text=True)
    assert r.returncode == code, r.stderr


def test_25_mbit_streams_decode_as_before_through_the_422_harness(tmp_path):
    exe = P.harness()
    frames = [D.encode(D.synth(n, 4, 6), 3) for n in range(2)]
    pk, out = tmp_path / "p.bin", tmp_path / "o.bin"
    P.packets(pk, frames)
    for pixfmt in ("none", "411", "420"):  # 720 x 480 with any pixel format but 4:2:2 is 525/60 4:1:1
        r = subprocess.run([exe, str(pk), "720", "480", pixfmt, str(out)], capture_output=True, text=True)
        assert r.returncode == 0 and "frame 720x480" in r.stderr, r.stderr
        rec = D.PICTURE_BYTES + 8
        raw = np.fromfile(out, dtype=np.uint8)
        assert raw.size == 2 * rec
        for i in range(2):
            assert np.array_equal(raw[i * rec:i * rec + D.PICTURE_BYTES], D.decode(frames[i]))
