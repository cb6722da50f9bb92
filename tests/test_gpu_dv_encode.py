"""GPU parity of the DV encoder — k_dv_encode<Sys> through mi_dv_encode_batch, mi_dv_encode_frame, mi_dv_encode_stats —
against the integer statement tests/dvenc.py, byte for byte over whole frames (ids and header bits included), in all five
systems.  A frame is the smallest unit the kernel has: batches of 1, 2 and 3 pictures.  UNPINNED: see tests/dvenc.py."""
import importlib

import numpy as np
import pytest

import dvenc as E
import dvlib as D
import dvsys as S

pytestmark = pytest.mark.gpu
ERR_ARG = -1
GUARD, FILL = 256, 0xA5


@pytest.fixture(scope="module")
def dv():
    return importlib.import_module("gmerlin-avdecoder_amd.dv")


@pytest.fixture(scope="module")
def dev(dv):
    d = dv.MiDv(0)
    yield d
    d.close()


def frames_differ(system, got, want, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        seq, rest = divmod(int(bad[0]), 150 * 80)
        raise AssertionError(f"system {system} {what}: {bad.size} bytes differ, first at {bad[0]} (sequence {seq}, DIF block "
                             f"{rest // 80}, byte {rest % 80}: got {got[bad[0]]:#x}, want {want[bad[0]]:#x})")


def gpu_encode(dev, system, pics, flags):
    """pictures -> frames through one launch; the bytes around the output keep their prefill"""
    g = S.geometry(system)
    pics = np.ascontiguousarray(pics, np.uint8).reshape(-1, g.picture_bytes)
    n = pics.shape[0]
    dp, df = dev.alloc(n * g.picture_bytes), dev.alloc(n * g.frame_bytes + 2 * GUARD)
    try:
        dev.h2d(dp, pics)
        dev.h2d(df, np.full(n * g.frame_bytes + 2 * GUARD, FILL, np.uint8))
        dev.encode_batch(system, dp, n, df + GUARD, flags)
        dev.sync()
        out = dev.d2h(df, n * g.frame_bytes + 2 * GUARD)
    finally:
        dev.free(dp)
        dev.free(df)
    assert (out[:GUARD] == FILL).all() and (out[-GUARD:] == FILL).all(), "the encoder wrote outside its frames"
    return out[GUARD:-GUARD].reshape(n, g.frame_bytes)


# ---- 1. byte equality ----
@pytest.mark.parametrize("which", E.PICTURES)
@pytest.mark.parametrize("flags", range(4))
@pytest.mark.parametrize("system", S.SYSTEMS)
def test_a_frame_equals_the_statement(dev, system, flags, which):
    got = gpu_encode(dev, system, E.picture(system, which), flags)
    frames_differ(system, got[0], E.stated(system, which, flags)[0], f"flags {flags}, picture {which}")


@pytest.mark.parametrize("region", ["right", "bottom"])
def test_the_right_edge_column_and_the_bottom_of_625_411(dev, region):
    system = S.SYS_625_50_411
    pic = S.synth(system, 1, 5, 12, region=region)
    got = gpu_encode(dev, system, pic, 3)
    frames_differ(system, got[0], E.encode(system, pic, 3), f"region {region}")


@pytest.mark.parametrize("system", S.SYSTEMS)
def test_three_pictures_in_one_launch_equal_three_launches_of_one(dev, system):
    names = ("flat", "n8", "drop")
    pics = np.stack([E.picture(system, w) for w in names])
    three = gpu_encode(dev, system, pics, 3)
    two = gpu_encode(dev, system, pics[1:], 3)
    for i, w in enumerate(names):
        frames_differ(system, three[i], E.stated(system, w, 3)[0], f"picture {i} of three")
        frames_differ(system, gpu_encode(dev, system, pics[i], 3)[0], three[i], f"picture {i} alone")
    assert np.array_equal(two, three[1:])


# ---- 2. the device round trip ----
@pytest.mark.parametrize("system", S.SYSTEMS)
def test_encoded_frames_decode_on_the_device_as_the_statement_frames_do(dev, dv, system):
    g = S.geometry(system)
    names = ("n8", "drop")
    pics = np.stack([E.picture(system, w) for w in names])
    n = len(names)
    dp, df, dq = dev.alloc(n * g.picture_bytes), dev.alloc(n * g.frame_bytes), dev.alloc(n * g.picture_bytes)
    try:
        dev.h2d(dp, pics)
        dev.encode_batch(system, dp, n, df, 3)
        dev.decode_batch_sys(system, df, n, dq)
        dev.sync()
        frames = dev.d2h(df, n * g.frame_bytes).reshape(n, -1)
        back = dev.d2h(dq, n * g.picture_bytes).reshape(n, -1)
    finally:
        for d in (dp, df, dq):
            dev.free(d)
    for i, w in enumerate(names):
        assert dv.kind_of(frames[i]) == system
        S.differ(system, back[i], S.decode(system, E.stated(system, w, 3)[0]), f"round trip of {w}")


# ---- 3. mi_dv_encode_frame ----
@pytest.mark.parametrize("system", S.SYSTEMS)
def test_encode_frame_with_padded_strides_equals_the_batch_path(dev, dv, system):
    g = S.geometry(system)
    pic = E.picture(system, "n8")
    strides = tuple(w + 24 + 8 * i for i, (w, _) in enumerate(g.planes))
    planes, at = [], 0
    for (w, h), st in zip(g.planes, strides):
        p = np.full((h, st), 0x5A, np.uint8)
        p[:, :w] = pic[at:at + w * h].reshape(h, w)
        planes.append(p.ravel())
        at += w * h
    want = E.stated(system, "n8", 3)[0]
    frames_differ(system, dev.encode_frame(planes, system, strides, 3), want, "padded strides")
    with pytest.raises(dv.MiDvError, match="room for"):
        dev.encode_frame(planes, system, strides, 3, cap=g.frame_bytes - 1)
    frames_differ(system, dev.encode_frame(planes, system, strides, 3), want, "after a refused cap")


# ---- 4. mi_dv_encode_stats ----
@pytest.mark.parametrize("system", S.SYSTEMS)
def test_encode_stats_are_the_statements_census(dev, system):
    names = ("flat", "n8", "drop")
    gpu_encode(dev, system, np.stack([E.picture(system, w) for w in names]), 3)
    hist, dropped = dev.encode_stats()
    want = [E.stated(system, w, 3) for w in names]
    assert np.array_equal(hist, sum(w[1] for w in want))
    assert dropped == sum(w[2] for w in want) and want[2][2] > 0
    gpu_encode(dev, system, E.picture(system, "flat"), 3)  # the counts are the last batch's
    hist, dropped = dev.encode_stats()
    assert np.array_equal(hist, want[0][1]) and dropped == 0


# ---- 5. refusals launch nothing and leave the instance working ----
def test_refusals_launch_nothing(dev, dv):
    system = S.SYS_625_50
    g = S.geometry(system)
    dev.encode_times()
    dev.kernel_times()
    dp, df = dev.alloc(g.picture_bytes + 16), dev.alloc(g.frame_bytes + 16)
    try:
        dev.h2d(df, np.full(g.frame_bytes + 16, FILL, np.uint8))
        L, c = dev.L, dev.c
        for args in ((2, dp, 1, df, 3), (6, dp, 1, df, 3), (system, dp, 0, df, 3), (system, dp, -1, df, 3),
                     (system, dp, 65536, df, 3), (system, None, 1, df, 3), (system, dp, 1, None, 3), (system, dp + 4, 1, df, 3),
                     (system, dp, 1, df + 2, 3), (system, dp, 1, dp + 8, 3), (system, dp, 1, df, 4), (system, dp, 1, df, -1)):
            assert L.mi_dv_encode_batch(c, *args) == ERR_ARG, args
            assert L.mi_dv_last_error(c)
        assert dev.encode_times() == (0.0, 0)
        assert (dev.d2h(df, g.frame_bytes + 16) == FILL).all()
    finally:
        dev.free(dp)
        dev.free(df)
    got = gpu_encode(dev, system, E.picture(system, "n8"), 3)
    frames_differ(system, got[0], E.stated(system, "n8", 3)[0], "after the refusals")
    ms, launches = dev.encode_times()
    assert launches == 1 and ms > 0
    assert dev.kernel_times()[1] == 0  # mi_dv_kernel_times keeps counting k_dv_decode alone


# ---- 6. the decoder is what it was ----
def test_the_old_entry_point_still_decodes_an_oracle_frame(dev, dv):
    pic = D.synth(2, 9, 8)
    gpu_encode(dev, S.SYS_525_60, pic, 3)  # the encoder has run in this process and on this instance
    dif = D.encode(pic, 3)
    d_fr, d_pic = dev.alloc(dv.FRAME_BYTES), dev.alloc(dv.PICTURE_BYTES)
    try:
        dev.h2d(d_fr, dif)
        dev.decode_batch(d_fr, 1, d_pic)
        dev.sync()
        got = dev.d2h(d_pic, dv.PICTURE_BYTES)
    finally:
        dev.free(d_fr)
        dev.free(d_pic)
    S.differ(S.SYS_525_60, got, D.decode(dif), "mi_dv_decode_batch after an encode")
