"""libmi_yuv.so on the device against the statement (tests/yuvraw.py), byte for byte: every codec of lib/video_yuv.c at the
smallest shapes at which its kernel can still go wrong, in batches of 1, 3 and 5 with both strides larger than the sizes,
256 bytes of 0xA5 around both buffers and between the picture slots; the refusals, each with nothing written; the host
call with strides wider than the rows; the launch count of mi_yuv_times."""
import importlib

import numpy as np
import pytest

import yuvraw as Y

pytestmark = pytest.mark.gpu

GUARD, FILL = 256, 0xA5
# planes that are no multiple of 16 bytes, one-piece and many-piece planes, more than one block (720 x 2); per codec below
PACKED_422 = [(2, 1), (6, 3), (34, 2), (720, 2)]
PLANAR_420 = [(2, 2), (6, 4), (34, 2)]
PIXELS = [(1, 1), (5, 3), (67, 2), (720, 2)]
SHAPES = {
    "yuv2": PACKED_422, "2vuy": PACKED_422, "VYUY": PACKED_422,
    "yv12": PLANAR_420, "YV12": PLANAR_420, "yuv4": PLANAR_420,
    "YVU9": [(4, 4), (12, 4), (40, 8)],  # 12 x 4: stride 16, chroma width 3 at stride 4
    "v308": PIXELS, "v408": PIXELS, "v410": PIXELS,
    # tail only; one group; tail 2; tail 4; the stride's step from 128 to 256; wide items with a tail
    "v210": [(2, 1), (6, 1), (8, 2), (10, 2), (48, 2), (50, 2), (720, 2)],
}
CASES = [(c, w, h) for c in Y.CODECS for w, h in SHAPES[c]]


@pytest.fixture(scope="module")
def yuv():
    return importlib.import_module("gmerlin-avdecoder_amd.yuv")


@pytest.fixture(scope="module")
def dev(yuv):
    d = yuv.MiYuv(0)
    yield d
    d.close()


class Slots:
    """n slots of `stride` bytes (the last one `size`) behind a guard, a guard behind them; all of it on the device"""

    def __init__(self, dev, size, stride, n, content):
        self.dev, self.size, self.stride, self.n = dev, size, stride, n
        self.bytes = 2 * GUARD + (n - 1) * stride + size
        self.host = np.full(self.bytes, FILL, np.uint8)
        for i in range(n):
            if content is not None:
                self.host[GUARD + i * stride:GUARD + i * stride + size] = content[i]
        self.d = dev.alloc(self.bytes)
        dev.h2d(self.d, self.host)
        self.base = self.d + GUARD

    def read(self):
        return self.dev.d2h(self.d, self.bytes)

    def free(self):
        self.dev.free(self.d)


def run_batch(dev, codec, w, h, n, rng):
    lay = Y.layout(codec, w, h)
    ps, qs = (lay.packet_bytes + 15) // 16 * 16 + 48, (lay.picture_bytes + 15) // 16 * 16 + 32
    packets = [Y.random_packet(codec, w, h, rng) for _ in range(n)]
    src, dst = Slots(dev, lay.packet_bytes, ps, n, packets), Slots(dev, lay.picture_bytes, qs, n, None)
    try:
        dev.unpack_batch(codec, w, h, src.base, ps, n, dst.base, qs)
        dev.sync()
        assert np.array_equal(src.read(), src.host), "the packets were written"
        want = dst.host.copy()
        for i in range(n):
            want[GUARD + i * qs:GUARD + i * qs + lay.picture_bytes] = Y.unpack(codec, w, h, packets[i])
        got = dst.read()
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            at = int(bad[0]) - GUARD
            where = "the guard in front" if at < 0 else f"slot {at // qs} byte {at % qs} (picture bytes {lay.picture_bytes})"
            raise AssertionError(f"{codec} {w} x {h}, batch of {n}: {bad.size} bytes differ from the statement's, first in {where}: "
                                 f"{int(got[bad[0]]):#x}, not {int(want[bad[0]]):#x}")
    finally:
        src.free()
        dst.free()


@pytest.mark.parametrize("codec,w,h", CASES, ids=[f"{c}-{w}x{h}" for c, w, h in CASES])
def test_every_codec_byte_for_byte_in_batches_of_1_3_5(dev, codec, w, h):
    rng = np.random.default_rng(100000 * Y.CODECS.index(codec) + 100 * w + h)
    for n in (1, 3, 5):
        run_batch(dev, codec, w, h, n, rng)


def test_the_cases_are_the_issue_s():
    assert len(CASES) == 3 * 4 + 3 * 3 + 3 + 3 * 4 + 7 and {c for c, _, _ in CASES} == set(Y.CODECS)
    assert Y.layout("YVU9", 12, 4).packet_strides == (16, 4, 4) and Y.layout("YVU9", 12, 4).planes[1] == (3, 1, 1)
    assert Y.layout("v210", 48, 2).packet_strides[0] == 128 and Y.layout("v210", 50, 2).packet_strides[0] == 256
    assert all(15 * Y.layout(c, 5, 3).planes[0][2] % 16 for c in ("v308", "v408", "v410"))  # 5 x 3 planes: 15, 60, 30 bytes


# ------------------------------------------------------------------ refusals: each with nothing written
def test_refusals_write_nothing(dev, yuv):
    codec, w, h, n = "v308", 34, 2, 3
    lay = Y.layout(codec, w, h)
    ps, qs = (lay.packet_bytes + 15) // 16 * 16 + 16, (lay.picture_bytes + 15) // 16 * 16 + 16
    rng = np.random.default_rng(9)
    src = Slots(dev, lay.packet_bytes, ps, n, [Y.random_packet(codec, w, h, rng) for _ in range(n)])
    dst = Slots(dev, lay.picture_bytes, qs, n, None)
    bad_sizes = [("yuv2", 3, 2), ("2vuy", 5, 1), ("VYUY", 7, 2), ("yv12", 3, 2), ("yv12", 2, 1), ("YV12", 2, 3), ("YVU9", 6, 4),
                 ("YVU9", 4, 2), ("v210", 5, 1), ("yuv4", 2, 1), ("yuv4", 1, 2), ("v308", 0, 1), ("v408", 1, 0), ("v410", -1, 1)]
    try:
        dev.times()
        calls = [
            ("16-byte aligned", (codec, w, h, src.base + 8, ps, n, dst.base, qs)),       # a misaligned base
            ("16-byte aligned", (codec, w, h, src.base, ps, n, dst.base + 4, qs)),
            ("16-byte aligned", (codec, w, h, src.base, ps + 8, n, dst.base, qs)),       # a misaligned stride
            ("16-byte aligned", (codec, w, h, src.base, ps, n, dst.base, qs + 1)),
            ("1 to 65535", (codec, w, h, src.base, ps, 0, dst.base, qs)),                # n = 0
            ("1 to 65535", (codec, w, h, src.base, ps, 65536, dst.base, qs)),
            ("1 to 65535", (codec, w, h, src.base, ps, -1, dst.base, qs)),
            ("overlaps", (codec, w, h, src.base, ps, n, src.base + ps, qs)),             # overlap
            ("overlaps", (codec, w, h, dst.base + 16, ps, n, dst.base, qs)),
            ("strides of", (codec, w, h, src.base, ps - 32, n, dst.base, qs)),           # a stride below the size
            ("strides of", (codec, w, h, src.base, ps, n, dst.base, qs - 32)),
            ("NULL", (codec, w, h, None, ps, n, dst.base, qs)),
            ("unknown codec", (11, w, h, src.base, ps, n, dst.base, qs)),
        ] + [("multiple of|positive", (c, bw, bh, src.base, ps, 1, dst.base, qs)) for c, bw, bh in bad_sizes]
        for what, args in calls:
            with pytest.raises(yuv.MiYuvError, match=what) as e:
                dev.unpack_batch(*args)
            assert e.value.code == yuv.ERR_ARG, (what, args)
        dev.sync()
        assert dev.times()[1] == 0, "a refused call launched"
        assert (dst.read() == FILL).all() and np.array_equal(src.read(), src.host)
        dev.unpack_batch(codec, w, h, src.base, ps, n, dst.base, qs)  # and the same buffers are taken as they should be
        dev.sync()
        assert dev.times()[1] == 1 and np.array_equal(dst.read()[GUARD:GUARD + lay.picture_bytes], Y.unpack(codec, w, h, src.host[GUARD:]))
    finally:
        src.free()
        dst.free()


# ------------------------------------------------------------------ the host call
HOST_SHAPES = [("yuv2", 34, 2), ("2vuy", 6, 3), ("VYUY", 34, 2), ("yv12", 6, 4), ("YV12", 34, 2), ("YVU9", 12, 4), ("v308", 67, 2),
               ("v408", 5, 3), ("v410", 67, 2), ("v210", 50, 2), ("yuv4", 6, 4)]


@pytest.mark.parametrize("codec,w,h", HOST_SHAPES, ids=[c for c, _, _ in HOST_SHAPES])
def test_unpack_frame_into_planes_with_wide_strides(dev, yuv, codec, w, h):
    lay = Y.layout(codec, w, h)
    rng = np.random.default_rng(21)
    packet = Y.random_packet(codec, w, h, rng)
    strides = [pw * bps + 5 + 2 * i for i, (pw, _, bps) in enumerate(lay.planes)]

    def fresh():
        return [np.full(strides[i] * ph, 0x5A, np.uint8) for i, (_, ph, _) in enumerate(lay.planes)]
    planes = dev.unpack_frame(codec, w, h, np.concatenate([packet, np.full(9, 0x77, np.uint8)]), strides, fresh())
    want = Y.planes_of(codec, w, h, Y.unpack(codec, w, h, packet))
    for i, (pw, ph, bps) in enumerate(lay.planes):
        got = planes[i].reshape(ph, strides[i])
        assert np.array_equal(got[:, :pw * bps], want[i]), (codec, "plane", i)
        assert (got[:, pw * bps:] == 0x5A).all(), (codec, "the bytes between the rows of plane", i)
    # tight strides (the default) give the tight picture
    tight = dev.unpack_frame(codec, w, h, packet)
    assert np.array_equal(np.concatenate(tight), Y.unpack(codec, w, h, packet))
    # a packet of length 0 is skipped: OK, planes untouched
    untouched = dev.unpack_frame(codec, w, h, np.zeros(0, np.uint8), strides, fresh())
    assert all((p == 0x5A).all() for p in untouched)
    # a short packet: upstream would read past it
    planes = fresh()
    with pytest.raises(yuv.MiYuvError, match=f"a packet of {lay.packet_bytes - 1} bytes") as e:
        dev.unpack_frame(codec, w, h, packet[:-1], strides, planes)
    assert e.value.code == yuv.ERR_FORMAT and all((p == 0x5A).all() for p in planes)
    with pytest.raises(yuv.MiYuvError, match="below its row") as e:
        dev.unpack_frame(codec, w, h, packet, [s - 6 for s in strides], fresh())
    assert e.value.code == yuv.ERR_ARG


def test_one_instance_takes_every_codec_and_growing_sizes_through_the_host_call(dev):
    rng = np.random.default_rng(4)
    for codec, w, h in (("v308", 5, 3), ("v210", 720, 2), ("v410", 67, 2), ("yuv4", 34, 2), ("v210", 6, 1)):
        packet = Y.random_packet(codec, w, h, rng)
        assert np.array_equal(np.concatenate(dev.unpack_frame(codec, w, h, packet)), Y.unpack(codec, w, h, packet))


def test_unpack_packets_convenience(dev):
    rng = np.random.default_rng(6)
    packets = np.stack([Y.random_packet("v210", 50, 2, rng) for _ in range(4)])
    pics = dev.unpack_packets("v210", 50, 2, packets)
    for i in range(4):
        assert np.array_equal(pics[i], Y.unpack("v210", 50, 2, packets[i]))


# ------------------------------------------------------------------ mi_yuv_times
def test_times_counts_the_launches(dev):
    lay = Y.layout("yuv2", 720, 2)
    rng = np.random.default_rng(8)
    src = Slots(dev, lay.packet_bytes, lay.packet_bytes, 2, [Y.random_packet("yuv2", 720, 2, rng) for _ in range(2)])
    dst = Slots(dev, lay.picture_bytes, lay.picture_bytes, 2, None)
    try:
        dev.times()
        assert dev.times() == (0.0, 0)
        for _ in range(3):
            dev.unpack_batch("yuv2", 720, 2, src.base, lay.packet_bytes, 2, dst.base, lay.picture_bytes)
        dev.unpack_frame("2vuy", 6, 3, Y.random_packet("2vuy", 6, 3, rng))  # the host call is one launch too
        ms, launches = dev.times()
        assert launches == 4 and ms > 0
        assert dev.times() == (0.0, 0)
    finally:
        src.free()
        dst.free()
