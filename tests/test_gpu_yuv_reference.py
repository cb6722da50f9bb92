"""libmi_yuv.so on the device against what the reference's own lib/video_yuv.c made of the same packets:
tests/golden/yuv_ref.json (written from oracle/_ref/libvideo_yuv_ref.so by tests/golden/make_yuv_ref.py; held to the live
reference and the statement by tests/test_yuv_fixtures_cpu.py).  No reference build and no reference tree is read here.
Every case of the GPU suite's CASES in one batch of its three seeded packets, with the strides and guards of
tests/test_gpu_yuvraw.py's run_batch.  Byte equality, or the SHA-256 of a picture above 2048 bytes."""
import numpy as np
import pytest

import yuvraw as Y
import yuvref as R
from test_gpu_yuvraw import FILL, GUARD, Slots, dev, yuv  # noqa: F401  (dev, yuv: the device's fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


@pytest.mark.parametrize("codec,w,h", R.CASES, ids=[R.case_id(*c) for c in R.CASES])
def test_a_batch_of_three_equals_the_reference_s_pictures(dev, fx, codec, w, h):
    lay, rec, n = Y.layout(codec, w, h), fx[R.case_id(codec, w, h)], R.PACKETS
    packets = R.packets(codec, w, h)
    assert [R.sha(p) for p in packets] == rec["packets"], "the packets are not the ones the reference was given"
    ps, qs = (lay.packet_bytes + 15) // 16 * 16 + 48, (lay.picture_bytes + 15) // 16 * 16 + 32
    src, dst = Slots(dev, lay.packet_bytes, ps, n, packets), Slots(dev, lay.picture_bytes, qs, n, None)
    try:
        dev.unpack_batch(codec, w, h, src.base, ps, n, dst.base, qs)
        dev.sync()
        assert np.array_equal(src.read(), src.host), "the packets were written"
        got = dst.read()
    finally:
        src.free()
        dst.free()
    outside = np.ones(got.size, bool)
    for i in range(n):
        at = GUARD + i * qs
        outside[at:at + lay.picture_bytes] = False
        pic = got[at:at + lay.picture_bytes]
        if R.kept(pic) != rec["pictures"][i]:
            want = Y.unpack(codec, w, h, packets[i])  # (the statement equals the reference: the fixture's CPU test)
            bad = np.flatnonzero(pic != want)
            where = f"first at byte {int(bad[0])}: {int(pic[bad[0]]):#x}, not {int(want[bad[0]]):#x}" if bad.size else "none from the statement's"
            raise AssertionError(f"{codec} {w} x {h}: slot {i} is not the reference's picture; {bad.size} bytes differ from the statement's, {where}")
    assert (got[outside] == FILL).all(), f"{codec} {w} x {h}: written outside the pictures"
