"""What the DV library's host layer (csrc/mi_dv.hip and its dv_host_*.h) keeps between calls, and no other test reaches:
the one-frame buffers that three entry points share and that grow with the system, the hold pass's descriptor and mask
buffers growing from batch to batch, the three event timers (k_dv_decode, the hold pass, k_dv_encode) with their common
pool and their cap of 4096 pairs, and refused calls leaving the timers alone.  Every result is compared bit for bit with
the statements the other DV tests use (tests/dvsys.py, dvhold.py, dvenc.py).  Every case runs on an instance of its own,
closed explicitly.  UNPINNED like everything about DV here."""
import functools
import importlib

import numpy as np
import pytest

import dvenc as E
import dvhold as H
import dvsys as S

pytestmark = pytest.mark.gpu
EVENT_CAP = 4096  # include/mi_dv.h, at mi_dv_kernel_times: the newest pairs a timer keeps when nobody asks


@pytest.fixture(scope="module")
def dv():
    return importlib.import_module("gmerlin-avdecoder_amd.dv")


@pytest.fixture
def dev(dv):
    d = dv.MiDv(0)
    yield d
    d.close()


@functools.lru_cache(None)
def encoded(system, i):
    """frame i of a system's encoded frames, made once"""
    f = S.encode(system, S.synth(system, i, 3 + system, 6 + 3 * i), 3)
    f.setflags(write=False)
    return f


def flagged(system, n, rng, k=5, distinct=2):
    """n frames that repeat the system's first `distinct` encoded ones, k macroblocks of each flagged with an error nibble"""
    out = []
    for i in range(n):
        fl = np.zeros(S.geometry(system).macroblocks, bool)
        fl[rng.choice(fl.size, k, replace=False)] = True
        out.append(H.stamp(system, encoded(system, i % distinct), H.nibbles(system, rng, fl)))
    return np.stack(out)


def padded(system, pic, pad):
    """a picture as three planes with `pad` and more bytes between rows -> (planes, strides)"""
    g = S.geometry(system)
    strides = tuple(w + pad + 8 * i for i, (w, _) in enumerate(g.planes))
    planes, at = [], 0
    for (w, h), st in zip(g.planes, strides):
        p = np.full((h, st), 0x5A, np.uint8)
        p[:, :w] = pic[at:at + w * h].reshape(h, w)
        planes.append(p.ravel())
        at += w * h
    return planes, strides


def packed(system, planes, strides):
    """the picture in planes of these strides; the bytes between rows are still the decoder's zeros"""
    g = S.geometry(system)
    rows = [planes[i].reshape(g.planes[i][1], strides[i]) for i in range(3)]
    assert all((rows[i][:, g.planes[i][0]:] == 0).all() for i in range(3)), "the bytes between rows were written"
    return np.concatenate([rows[i][:, :g.planes[i][0]].ravel() for i in range(3)])


# ---- 1. decode_frame, decode_frame_held and encode_frame share one frame, one picture and one pinned picture ----
def test_the_three_one_frame_paths_share_buffers_that_grow_with_the_system(dev):
    """525/60 (120,000 / 518,400 bytes) -> 625/50 4:2:2 (288,000 / 829,440: both grow) -> 525/60 (reused) -> 625/50 4:2:0
    (reused) -> 625/50 4:2:2; every held decode follows a frame of another system, so it has no source"""
    rng = np.random.default_rng(1100)
    for step, system in enumerate((S.SYS_525_60, S.SYS_625_50_422, S.SYS_525_60, S.SYS_625_50, S.SYS_625_50_422)):
        g = S.geometry(system)
        frame = flagged(system, 1, rng, distinct=1)[0]
        strides = tuple(w + 24 + 8 * i for i, (w, _) in enumerate(g.planes))
        want = H.decoded(system, frame)
        S.differ(system, packed(system, dev.decode_frame(frame, strides, system), strides), want, f"step {step}, plain")
        planes, held = dev.decode_frame_held(frame, system, strides)
        held_want, taken = H.hold(system, frame, [1])
        S.differ(system, packed(system, planes, strides), held_want[0], f"step {step}, held")
        assert held == taken[0] == 0
        planes, strides = padded(system, E.picture(system, "n8"), 24)
        got = dev.encode_frame(planes, system, strides, 3)
        assert np.array_equal(got, E.stated(system, "n8", 3)[0]), f"step {step}, system {system}: the encoded frame differs"


# ---- 2. the hold pass's descriptors and mask rows grow from batch to batch ----
def test_the_hold_buffers_grow_between_batches(dev):
    """3 frames in one run (one chunk), 65 frames (two chunks: descriptors and mask rows grow), 3 frames in runs [1, 2]
    behind two pictures of d_prev (two chunks, two runs)"""
    system = S.SYS_525_60
    rng = np.random.default_rng(1200)
    for n, runs, with_prev in ((3, None, False), (65, None, False), (3, [1, 2], True)):
        frames = flagged(system, n, rng)
        prev = rng.integers(0, 256, (len(runs), S.geometry(system).picture_bytes), dtype=np.uint8) if with_prev else None
        want, taken = H.hold(system, frames, runs, prev)
        assert taken.sum() > 0  # (phase 2 has work)
        got = dev.decode_frames_held(frames, system, runs=runs, prev=prev)
        for k in range(n):
            S.differ(system, got[k], want[k], f"batch of {n}, picture {k}")
        assert dev.hold_stats() == taken.sum()


# ---- 3. the timers ----
class Resident:
    """frames and pictures of one system on the device: 3 frames, 3 pictures, 3 more frames for the encoder"""

    def __init__(self, dev, system, frames):
        self.dev, self.g = dev, S.geometry(system)
        self.df, self.dp, self.de = dev.alloc(3 * self.g.frame_bytes), dev.alloc(3 * self.g.picture_bytes), dev.alloc(3 * self.g.frame_bytes)
        dev.h2d(self.df, frames)

    def free(self):
        for d in (self.df, self.dp, self.de):
            self.dev.free(d)


def test_the_three_timers_are_separate_and_recycle(dev):
    system = S.SYS_525_60
    frames = flagged(system, 3, np.random.default_rng(1300), k=1)
    r = Resident(dev, system, frames)
    try:
        for _ in range(2):
            dev.decode_batch_sys(system, r.df, 3, r.dp)
        dev.decode_batch_held(system, r.df, 2, r.dp)  # a run of 2 has a source: phase 1 and phase 2
        for _ in range(3):
            dev.encode_batch(system, r.dp, 3, r.de)
        for times, launches in ((dev.kernel_times, 3), (dev.hold_times, 3), (dev.encode_times, 3)):
            ms, n = times()
            assert n == launches and ms > 0, (times.__name__, ms, n)
            assert times() == (0.0, 0), times.__name__
        dev.decode_batch_sys(system, r.df, 1, r.dp)
        ms, n = dev.kernel_times()
        assert n == 1 and ms > 0
        assert dev.hold_times() == (0.0, 0) and dev.encode_times() == (0.0, 0)
    finally:
        r.free()


def test_a_timer_nobody_asks_keeps_its_newest_pairs(dev):
    """4,100 launches of one frame without a question in between: the times are those of the newest 4,096"""
    system = S.SYS_525_60
    frames = flagged(system, 3, np.random.default_rng(1400), k=1)
    r = Resident(dev, system, frames)
    try:
        for _ in range(EVENT_CAP + 4):
            dev.decode_batch_sys(system, r.df, 1, r.dp)
        ms, n = dev.kernel_times()
        assert n == EVENT_CAP and ms > 0
        assert dev.kernel_times() == (0.0, 0)
        S.differ(system, dev.d2h(r.dp, r.g.picture_bytes), H.decoded(system, frames[0]), "the last of 4,100 launches")
    finally:
        r.free()


def test_a_refused_call_leaves_the_timers_alone(dev, dv):
    system = S.SYS_525_60
    frames = flagged(system, 3, np.random.default_rng(1500), k=1)
    r = Resident(dev, system, frames)
    try:
        dev.decode_batch_sys(system, r.df, 1, r.dp)
        assert dev.kernel_times()[1] == 1
        with pytest.raises(dv.MiDvError, match="d_frames must be 4-byte and d_pics 8-byte aligned"):
            dev.decode_batch_sys(system, r.df, 1, r.dp + 4)
        with pytest.raises(dv.MiDvError, match="d_frames overlaps d_pics"):
            dev.encode_batch(system, r.dp, 1, r.dp + 8)
        assert dev.kernel_times() == (0.0, 0) and dev.hold_times() == (0.0, 0) and dev.encode_times() == (0.0, 0)
    finally:
        r.free()
