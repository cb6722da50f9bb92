"""mi_dv_meta_write_batch and mi_dv_meta_batch with frames above byte 2^31 and byte 2^32 of their buffer, against the
statement tests/dvmeta.py, byte for byte and value for value.

Both kernels find their frame as `(size_t)frame index * Sys::kFrameBytes` and add 32-bit offsets inside the frame; an
index multiplied in 32 bits passes every test of a few frames.  One system is enough, as in
tests/test_gpu_dv_far_offsets.py: 625/50 4:2:2 has the largest frames (288,000 bytes).  15,146 of them fill the 2^32 + 2^26
bytes of tests/far_offsets.py: frame 7,456 lies across 2^31, frame 14,913 across 2^32, the 232 behind it above.  One
launch of each kernel covers them all; the frames around the lines start as noise and must come back as the statement's,
the others are whatever the memory held and are not judged.

A frame above 2^32 has an alias window 2^32 below it, where a store through an offset narrowed to 32 bits would land.
2^32 is 23,296 bytes past a multiple of the frame size, so the alias of DIF blocks 1..5 of a sequence lies 704 bytes into
a sequence of a low frame: in its video blocks 2..7, which no launch here may touch, although the low frame's own blocks
1..5 are written like every frame's.  The windows are filled with noise first and compared outside the five blocks.
UNPINNED like everything about DV here: see the statement."""
import importlib

import numpy as np
import pytest

import dvmeta as M
import dvsys as S
import far_offsets as FO

pytestmark = pytest.mark.gpu

SYSTEM = S.SYS_625_50_422
FB = M.META[SYSTEM].frame_bytes
N = FO.BUFFER_BYTES // FB
CHECK = [0, 7455, 7456, 7457, 14912, 14913, 14914, 15000, N - 1]
FAR = [k for k in CHECK if (k + 1) * FB > FO.WRAP]  # frames with an alias window
GUARD, FILL = FO.GUARD, 0xA5
FIRST, REC = (1 << 40) - N, 1709251199 - 300  # the last frame numbers the call takes; 23:54:59 on 29 February 2024


def test_the_arithmetic_of_the_layout():
    lo, hi = FO.LINES
    assert FB == 288000 and N == 15146 and N <= 65535 and N * FB <= FO.BUFFER_BYTES
    assert 7456 * FB < lo < 7457 * FB and 14913 * FB < hi < 14914 * FB and FAR == [14913, 14914, 15000, N - 1]
    assert hi - 14913 * FB == 23296 and FB - 23296 == 22 * 12000 + 704
    mask = M.meta_mask(SYSTEM)
    at = np.flatnonzero(mask)
    for k in FAR:  # where the five blocks of a far frame would land 2^32 lower: no byte of any frame's five blocks
        alias = k * FB + at - FO.WRAP
        alias = alias[alias >= 0]
        assert alias.size and not mask[alias % FB].any()
    num, den = M.META[SYSTEM].fps
    assert (N - 1) * den // num > 600  # the batch lasts ten minutes: the recording time crosses midnight inside it


@pytest.fixture(scope="module")
def dv():
    return importlib.import_module("gmerlin-avdecoder_amd.dv")


def windows():
    """[start, end) of the alias windows of the far frames, merged: 2^32 below them, clipped to the buffer"""
    return FO.merge([(max(k * FB - FO.WRAP, 0), (k + 1) * FB - FO.WRAP) for k in FAR])


def test_timecodes_written_and_read_in_frames_across_the_lines(dv):
    mask = M.meta_mask(SYSTEM)
    frames = {k: M.noise_frame(SYSTEM, 950 + k, wiped=False) for k in CHECK}
    rng = np.random.default_rng(6)
    dev = dv.MiDv(0)
    d_fr, d_meta = dev.alloc(N * FB + GUARD), dev.alloc((N + 1) * 64)
    try:
        for a, b in windows():
            dev.h2d(d_fr, rng.integers(0, 256, b - a, dtype=np.uint8), offset=a)
        for k in CHECK:  # (frame 0 lies in the alias window of frame 14,913, which begins 23,296 bytes before the buffer)
            dev.h2d(d_fr, frames[k], offset=k * FB)
        before = [dev.d2h(d_fr, b - a, offset=a) for a, b in windows()]
        dev.h2d(d_fr, np.full(GUARD, FILL, np.uint8), offset=N * FB)
        dev.h2d(d_meta, np.full(64, FILL, np.uint8), offset=N * 64)
        dev.meta_times()
        dev.write_meta_batch(SYSTEM, d_fr, N, FIRST, 0, REC, 1)
        dev.meta_batch(SYSTEM, d_fr, N, d_meta)
        dev.sync()
        assert dev.meta_times()[1] == 2
        for k in CHECK:
            want = M.write_one(SYSTEM, frames[k], FIRST + k, 0, M.rec_of(SYSTEM, REC, k), 1)
            got = dev.d2h(d_fr, FB, offset=k * FB)
            if not np.array_equal(got, want):
                bad = np.flatnonzero(got != want)
                raise AssertionError(f"frame {k} at byte {k * FB:#x}: {bad.size} bytes differ from the statement's, "
                                     f"{int((~mask[bad]).sum())} of them outside the subcode and VAUX blocks, first at byte {int(bad[0])}")
            row = dev.d2h(d_meta, 64, offset=64 * k).view(np.int32)
            assert row.tolist() == M.extract(SYSTEM, want).tolist(), f"frame {k} at byte {k * FB:#x}: its row of d_meta"
            assert tuple(row[M.TC_H:M.TC_F + 1]) == M.timecode_of(SYSTEM, FIRST + k, 0) and row[M.FOUND] == 15
        rows = {k: dev.d2h(d_meta, 64, offset=64 * k).view(np.int32) for k in (0, N - 1)}
        assert tuple(rows[0][M.YEAR:M.SECOND + 1]) == (2024, 2, 29, 23, 54, 59) and tuple(rows[N - 1][M.YEAR:M.DAY + 1]) == (2024, 3, 1)
        for (a, b), was in zip(windows(), before):  # the alias windows: only the low frames' own five blocks changed
            now = dev.d2h(d_fr, b - a, offset=a)
            keep = ~mask[np.arange(a, b) % FB]
            bad = np.flatnonzero(keep & (now != was))
            assert not bad.size, (f"alias window [{a:#x}, {b:#x}): {bad.size} bytes outside every subcode and VAUX block changed, first at "
                                  f"byte {a + int(bad[0]):#x}: a store through an offset narrowed to 32 bits")
        assert (dev.d2h(d_fr, GUARD, offset=N * FB) == FILL).all(), "written behind the last frame"
        assert (dev.d2h(d_meta, 64, offset=N * 64) == FILL).all(), "written behind the last row"
        print(f"FAR-OFFSETS DV timecode: k_dv_meta_write and k_dv_meta_extract, 2 launches over {N} frames up to byte {N * FB:#x}", flush=True)
    finally:
        dev.free(d_fr)
        dev.free(d_meta)
        dev.close()
