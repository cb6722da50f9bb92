"""GPU parity of the DV encoder on THE EDGE PICTURES (tests/dvenc_edges.py): k_dv_encode<Sys> against the integer statement
tests/dvenc.py, byte for byte over whole frames, on segments built to reach the level clip, amplitude 255, runs of 62,
both sides of the mode threshold and of every class limit, every quantisation number, segments of exactly 2,680 bits and
of 2,681 at the next number, an overflow rule whose every step is a tie, the longest overflow loop, and wave partners 15
numbers apart.  tests/test_dv_encode_edges_cpu.py asserts that the pictures reach all that.  A frame is the kernel's
smallest unit: every case is one launch of one or two pictures.  A difference is reported with the name of the edge
segment it is in.  UNPINNED: see tests/dvenc.py."""
import numpy as np
import pytest

import dvenc_edges as X
import dvsys as S
from test_gpu_dv_encode import dev, dv, frames_differ, gpu_encode  # noqa: F401  (dv and dev are fixtures)

pytestmark = pytest.mark.gpu
CASES = [(system, flags) for system in S.SYSTEMS for flags in range(4)]


def edge_frames_differ(system, got, want, what, reverse=False):
    """frames_differ, and which entry of the list the first differing byte belongs to"""
    try:
        frames_differ(system, got, want, what)
    except AssertionError as e:
        fs, rest = divmod(int(np.flatnonzero(got != want)[0]), 150 * 80)
        b = rest // 80 - 6
        if b < 0 or b % 16 == 0:
            raise AssertionError(f"{e}; not in a video segment") from None
        seg = 27 * fs + (b - b // 16 - 1) // 5
        raise AssertionError(f"{e}; video segment {seg}, edge segment {X.name_at(system, seg, reverse)!r}") from None


@pytest.mark.parametrize("system,flags", CASES)
def test_the_edge_frame_equals_the_statement_and_the_counters_its_census(dev, system, flags):
    want, _, cen, _ = X.stated(system, flags)
    got = gpu_encode(dev, system, X.picture(system), flags)
    edge_frames_differ(system, got[0], want, f"flags {flags}, the edge picture")
    hist, dropped = dev.encode_stats()  # all seventeen counters
    assert hist.tolist() == cen["qno"] and dropped == cen["dropped"] and dropped > 0
    if flags == 3:
        assert (hist > 0).all()


@pytest.mark.parametrize("system", S.SYSTEMS)
def test_both_partner_orders_in_one_launch(dev, system):
    """the list forwards and backwards as a batch of two: every wave of the second picture has the partners of a wave of
    the first the other way round"""
    pics = np.stack([X.picture(system), X.picture(system, True)])
    got = gpu_encode(dev, system, pics, 3)
    edge_frames_differ(system, got[0], X.stated(system, 3)[0], "forwards, picture 0 of two")
    edge_frames_differ(system, got[1], X.stated(system, 3, True)[0], "backwards, picture 1 of two", reverse=True)
    hist, dropped = dev.encode_stats()
    both = [X.stated(system, 3, reverse)[2] for reverse in (False, True)]
    assert hist.tolist() == (np.array(both[0]["qno"]) + np.array(both[1]["qno"])).tolist()
    assert dropped == both[0]["dropped"] + both[1]["dropped"]


@pytest.mark.parametrize("system", S.SYSTEMS)
def test_the_device_decodes_its_edge_frames_as_the_oracle_decodes_the_statements(dev, dv, system):
    """amplitude-255 words and runs of 62 written by k_dv_encode, through k_dv_decode (flags 0 and 3 in one launch each)"""
    g = S.geometry(system)
    dp, df, dq = dev.alloc(g.picture_bytes), dev.alloc(g.frame_bytes), dev.alloc(g.picture_bytes)
    try:
        dev.h2d(dp, X.picture(system))
        for flags in (0, 3):
            dev.encode_batch(system, dp, 1, df, flags)
            dev.decode_batch_sys(system, df, 1, dq)
            dev.sync()
            frame, back = dev.d2h(df, g.frame_bytes), dev.d2h(dq, g.picture_bytes)
            assert dv.kind_of(frame) == system
            S.differ(system, back, S.decode(system, X.stated(system, flags)[0]), f"round trip of the edge picture, flags {flags}")
    finally:
        for d in (dp, df, dq):
            dev.free(d)


@pytest.mark.parametrize("system,flags", [(S.SYS_625_50_411, 3), (S.SYS_525_60_422, 0)])
def test_encode_frame_with_padded_strides_on_the_edge_picture(dev, system, flags):
    g = S.geometry(system)
    pic = X.picture(system)
    strides = tuple(w + 24 + 8 * i for i, (w, _) in enumerate(g.planes))
    planes, at = [], 0
    for (w, h), st in zip(g.planes, strides):
        p = np.full((h, st), 0x5A, np.uint8)
        p[:, :w] = pic[at:at + w * h].reshape(h, w)
        planes.append(p.ravel())
        at += w * h
    edge_frames_differ(system, dev.encode_frame(planes, system, strides, flags), X.stated(system, flags)[0], "padded strides")
