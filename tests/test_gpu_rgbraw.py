"""libmi_rgb.so on the device against the statement (tests/rgbraw.py), byte for byte: every codec of lib/video_qtraw.c and
lib/video_aviraw.c at the smallest shapes at which its kernel can still go wrong, in batches of 1, 3 and 5 with both strides
larger than the sizes, 256 bytes of 0xA5 around both buffers and between the slots; two palettes that alternate, and
palette_of = NULL; two calls queued back to back with different palettes; the refusals, each with nothing launched and
nothing written; the host call with a stride wider than the row; the launch count of mi_rgb_times."""
import importlib

import numpy as np
import pytest

import rgbraw as R

pytestmark = pytest.mark.gpu

GUARD, FILL = 256, 0xA5
# sub-byte codecs: one byte and its padding, two bytes a row, a stride that grows from 3 to 4, more than one block's chunk
# rows; byte codecs: one pixel, a piece across two rows, odd rows of 15 to 20 bytes, rows of many pieces that end inside one,
# more than one block
SUB_BYTE = {"QT1": [(8, 1), (16, 3), (24, 2), (720, 2)], "QT2": [(4, 1), (8, 3), (12, 2), (720, 2)],
            "QT4": [(2, 1), (4, 3), (6, 2), (720, 2)]}
BYTES = [(1, 1), (2, 2), (5, 3), (67, 2), (720, 2)]
SHAPES = {c: SUB_BYTE.get(c, BYTES) for c in R.CODECS}
CASES = [(c, w, h) for c in R.CODECS for w, h in SHAPES[c]]
PALETTISED = [c for c in R.CODECS if R.layout(c, 8, 1).palette_entries]


@pytest.fixture(scope="module")
def rgb():
    return importlib.import_module("gmerlin-avdecoder_amd.rgb")


@pytest.fixture(scope="module")
def dev(rgb):
    d = rgb.MiRgb(0)
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


def strides_of(lay):
    return (lay.packet_bytes + 15) // 16 * 16 + 48, (lay.picture_bytes + 15) // 16 * 16 + 32


def judge(codec, w, h, n, lay, qs, dst, packets, palette_for):
    want = dst.host.copy()
    for i in range(n):
        want[GUARD + i * qs:GUARD + i * qs + lay.picture_bytes] = R.unpack(codec, w, h, packets[i], palette_for(i))
    got = dst.read()
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        at = int(bad[0]) - GUARD
        where = "the guard in front" if at < 0 else f"slot {at // qs} byte {at % qs} (picture bytes {lay.picture_bytes})"
        raise AssertionError(f"{codec} {w} x {h}, batch of {n}: {bad.size} bytes differ from the statement's, first in {where}: "
                             f"{int(got[bad[0]]):#x}, not {int(want[bad[0]]):#x}")


def run_batch(dev, codec, w, h, n, rng, null_palette_of=False):
    lay = R.layout(codec, w, h)
    ps, qs = strides_of(lay)
    packets = [R.random_packet(codec, w, h, rng) for _ in range(n)]
    palettes = palette_of = None
    if lay.palette_entries:  # two palettes that alternate (one for a single packet); or palette 0 for all
        palettes = np.stack([R.random_palette(codec, rng) for _ in range(min(2, n))])
        palette_of = None if null_palette_of else np.arange(n, dtype=np.uint16) % len(palettes)
    src, dst = Slots(dev, lay.packet_bytes, ps, n, packets), Slots(dev, lay.picture_bytes, qs, n, None)
    try:
        dev.unpack_batch(codec, w, h, src.base, ps, n, dst.base, qs, palettes, palette_of)
        dev.sync()
        assert np.array_equal(src.read(), src.host), "the packets were written"
        judge(codec, w, h, n, lay, qs, dst, packets,
              lambda i: None if palettes is None else palettes[0 if palette_of is None else palette_of[i]])
    finally:
        src.free()
        dst.free()


@pytest.mark.parametrize("codec,w,h", CASES, ids=[f"{c}-{w}x{h}" for c, w, h in CASES])
def test_every_codec_byte_for_byte_in_batches_of_1_3_5(dev, codec, w, h):
    rng = np.random.default_rng(100000 * R.CODECS.index(codec) + 100 * w + h)
    for n in (1, 3, 5):
        run_batch(dev, codec, w, h, n, rng)


@pytest.mark.parametrize("codec", PALETTISED)
def test_palette_of_null_is_palette_0_for_every_packet(dev, codec):
    w, h = SHAPES[codec][2]
    run_batch(dev, codec, w, h, 3, np.random.default_rng(77 + R.CODECS.index(codec)), null_palette_of=True)


def test_the_cases_are_the_issue_s():
    assert len(CASES) == 3 * 4 + 10 * 5 and {c for c, _, _ in CASES} == set(R.CODECS) and len(R.CODECS) == 13
    assert SHAPES["QT1"] == [(8, 1), (16, 3), (24, 2), (720, 2)] and SHAPES["QT2"] == [(4, 1), (8, 3), (12, 2), (720, 2)]
    assert SHAPES["QT4"] == [(2, 1), (4, 3), (6, 2), (720, 2)]
    for c in R.CODECS:
        if c not in SUB_BYTE:
            assert SHAPES[c] == [(1, 1), (2, 2), (5, 3), (67, 2), (720, 2)]
    assert R.layout("QT1", 8, 1).packet_stride == 2 and R.layout("QT1", 24, 2).packet_stride == 4  # one padding byte; 3 -> 4
    assert [R.layout("QT24", w, h).packet_stride for w, h in BYTES[:4]] == [4, 6, 16, 202]
    assert [R.layout("AVI24", w, h).packet_stride for w, h in BYTES[:4]] == [4, 8, 16, 204]
    assert [R.layout("AVI16", w, h).packet_stride for w, h in BYTES[:4]] == [4, 4, 12, 136]
    assert {h for _, h in BYTES[1:]} == {2, 3}  # the flip with an even and an odd number of rows (a middle row)
    assert PALETTISED == ["QT1", "QT2", "QT4", "QT8", "AVI8"]


# ------------------------------------------------------------------ two calls back to back, other palettes, no sync
@pytest.mark.parametrize("codec", PALETTISED)
def test_two_calls_queued_back_to_back_with_different_palettes(dev, codec):
    w, h = SHAPES[codec][3]
    lay = R.layout(codec, w, h)
    ps, qs = strides_of(lay)
    rng = np.random.default_rng(500 + R.CODECS.index(codec))
    n = 3
    packets = [R.random_packet(codec, w, h, rng) for _ in range(n)]
    first, second = (np.stack([R.random_palette(codec, rng) for _ in range(2)]) for _ in range(2))
    kept = first.copy()
    of = np.array([1, 0, 1], np.uint16)
    of_kept = of.copy()
    src = Slots(dev, lay.packet_bytes, ps, n, packets)
    a, b = Slots(dev, lay.picture_bytes, qs, n, None), Slots(dev, lay.picture_bytes, qs, n, None)
    try:
        dev.unpack_batch(codec, w, h, src.base, ps, n, a.base, qs, first, of)
        first[:] = 0xFFFF  # the call has its own copy: the caller's arrays are the caller's again
        of[:] = 0
        dev.unpack_batch(codec, w, h, src.base, ps, n, b.base, qs, second, None)
        dev.sync()
        judge(codec, w, h, n, lay, qs, a, packets, lambda i: kept[of_kept[i]])
        judge(codec, w, h, n, lay, qs, b, packets, lambda i: second[0])
    finally:
        for s in (src, a, b):
            s.free()


# ------------------------------------------------------------------ refusals: each with nothing launched, nothing written
def test_refusals_launch_nothing_and_write_nothing(dev, rgb):
    codec, w, h, n = "QT8", 67, 2, 3
    lay = R.layout(codec, w, h)
    ps, qs = (lay.packet_bytes + 15) // 16 * 16 + 16, (lay.picture_bytes + 15) // 16 * 16 + 16
    rng = np.random.default_rng(9)
    src = Slots(dev, lay.packet_bytes, ps, n, [R.random_packet(codec, w, h, rng) for _ in range(n)])
    dst = Slots(dev, lay.picture_bytes, qs, n, None)
    pal = np.stack([R.random_palette(codec, rng) for _ in range(2)])
    pal2 = np.stack([R.random_palette("QT2", rng)])
    of = np.array([0, 1, 0], np.uint16)
    try:
        dev.times()
        calls = [
            ("16-byte aligned", (codec, w, h, src.base + 8, ps, n, dst.base, qs, pal, of)),       # a misaligned base
            ("16-byte aligned", (codec, w, h, src.base, ps, n, dst.base + 4, qs, pal, of)),
            ("16-byte aligned", (codec, w, h, src.base, ps + 8, n, dst.base, qs, pal, of)),       # a misaligned stride
            ("16-byte aligned", (codec, w, h, src.base, ps, n, dst.base, qs + 1, pal, of)),
            ("1 to 65535", (codec, w, h, src.base, ps, 0, dst.base, qs, pal, None)),              # n = 0
            ("1 to 65535", (codec, w, h, src.base, ps, 65536, dst.base, qs, pal, None)),
            ("1 to 65535", (codec, w, h, src.base, ps, -1, dst.base, qs, pal, None)),
            ("overlaps", (codec, w, h, src.base, ps, n, src.base + ps, qs, pal, of)),             # overlap
            ("overlaps", (codec, w, h, dst.base + 16, ps, n, dst.base, qs, pal, of)),
            ("strides of", (codec, w, h, src.base, ps - 32, n, dst.base, qs, pal, of)),           # a stride below the size
            ("strides of", (codec, w, h, src.base, ps, n, dst.base, qs - 32, pal, of)),
            ("NULL", (codec, w, h, None, ps, n, dst.base, qs, pal, of)),
            ("NULL", (codec, w, h, src.base, ps, n, None, qs, pal, of)),
            ("unknown codec", (13, w, h, src.base, ps, n, dst.base, qs)),
            ("unknown codec", (-1, w, h, src.base, ps, n, dst.base, qs)),
            ("QT1 at 12 x 2: the width is a multiple of 8", ("QT1", 12, 2, src.base, ps, 1, dst.base, qs)),   # bad widths
            ("QT2 at 6 x 2: the width is a multiple of 4", ("QT2", 6, 2, src.base, ps, 1, dst.base, qs)),
            ("QT4 at 3 x 2: the width is a multiple of 2", ("QT4", 3, 2, src.base, ps, 1, dst.base, qs)),
            ("QT2 at 6 x 2: the width is a multiple of 4", ("QT2", 6, 2, src.base, ps, 1, dst.base, qs, pal2)),
            ("positive", ("QT24", 0, 2, src.base, ps, 1, dst.base, qs)),
            ("positive", ("AVI32", 2, -1, src.base, ps, 1, dst.base, qs)),
            ("needs a palette of 256 entries", (codec, w, h, src.base, ps, n, dst.base, qs)),     # a missing palette
            ("needs a palette of 256 entries", ("AVI8", 16, 2, src.base, ps, n, dst.base, qs, None, of)),
            ("needs a palette of 4 entries", ("QT2", 8, 2, src.base, ps, n, dst.base, qs)),
            ("palette_of\\[1\\] is palette index 2 of 2", (codec, w, h, src.base, ps, n, dst.base, qs, pal, [0, 2, 1])),  # out of range
            ("palette_of\\[2\\] is palette index 1 of 1", (codec, w, h, src.base, ps, n, dst.base, qs, pal[:1], [0, 0, 1])),
            ("palettes for 1 packets", (codec, w, h, src.base, ps, 1, dst.base, qs, pal, None)),   # more palettes than packets
            ("QT24 has no palette", ("QT24", 16, 2, src.base, ps, n, dst.base, qs, pal, None)),   # a palette handed to QT24
            ("AVI8_GRAY has no palette", ("AVI8_GRAY", 16, 2, src.base, ps, n, dst.base, qs, pal, of)),
            ("shorter palette is refused", (codec, w, h, src.base, ps, n, dst.base, qs, pal[:, :255], of)),
        ]
        for what, args in calls:
            with pytest.raises(rgb.MiRgbError, match=what) as e:
                dev.unpack_batch(*args)
            assert e.value.code == rgb.ERR_ARG, (what, args)
        dev.sync()
        assert dev.times()[1] == 0, "a refused call launched"
        assert (dst.read() == FILL).all() and np.array_equal(src.read(), src.host)
        dev.unpack_batch(codec, w, h, src.base, ps, n, dst.base, qs, pal, of)  # and the same buffers are taken as they should be
        dev.sync()
        assert dev.times()[1] == 1
        assert np.array_equal(dst.read()[GUARD:GUARD + lay.picture_bytes], R.unpack(codec, w, h, src.host[GUARD:], pal[0]))
    finally:
        src.free()
        dst.free()


# ------------------------------------------------------------------ the host call
HOST_SHAPES = [("QT1", 24, 2), ("QT2", 12, 2), ("QT4", 6, 2), ("QT8", 67, 2), ("QT16", 5, 3), ("QT24", 67, 2), ("QT32", 5, 3),
               ("AVI8", 5, 3), ("AVI8_GRAY", 67, 2), ("AVI16", 5, 3), ("MTV16", 67, 2), ("AVI24", 5, 3), ("AVI32", 2, 2)]


@pytest.mark.parametrize("codec,w,h", HOST_SHAPES, ids=[c for c, _, _ in HOST_SHAPES])
def test_unpack_frame_into_a_plane_with_a_wide_stride(dev, rgb, codec, w, h):
    lay = R.layout(codec, w, h)
    rng = np.random.default_rng(21)
    packet = R.random_packet(codec, w, h, rng)
    palette = R.random_palette(codec, rng) if lay.palette_entries else None
    row = w * lay.bytes_per_pixel
    stride = row + 7

    def fresh():
        return np.full(stride * h, 0x5A, np.uint8)
    want = R.unpack(codec, w, h, packet, palette).reshape(h, row)
    # trailing bytes behind the packet (AVI chunks carry padding) are ignored
    got = dev.unpack_frame(codec, w, h, np.concatenate([packet, np.full(9, 0x77, np.uint8)]), palette, stride, fresh()).reshape(h, stride)
    assert np.array_equal(got[:, :row], want), codec
    assert (got[:, row:] == 0x5A).all(), (codec, "the bytes between the rows")
    # a tight stride (the default) gives the tight picture
    assert np.array_equal(dev.unpack_frame(codec, w, h, packet, palette), want.reshape(-1))
    # a packet of length 0 is skipped: OK, the plane untouched
    assert (dev.unpack_frame(codec, w, h, np.zeros(0, np.uint8), palette, stride, fresh()) == 0x5A).all()
    # a short packet: upstream would read past it
    plane = fresh()
    with pytest.raises(rgb.MiRgbError, match=f"a packet of {lay.packet_bytes - 1} bytes") as e:
        dev.unpack_frame(codec, w, h, packet[:-1], palette, stride, plane)
    assert e.value.code == rgb.ERR_FORMAT and (plane == 0x5A).all()
    with pytest.raises(rgb.MiRgbError, match="below the picture's row") as e:
        dev.unpack_frame(codec, w, h, packet, palette, row - 1, plane)
    assert e.value.code == rgb.ERR_ARG and (plane == 0x5A).all()
    # the palette a codec needs, and only that
    with pytest.raises(rgb.MiRgbError, match="has no palette" if palette is None else "needs a palette") as e:
        dev.unpack_frame(codec, w, h, packet, R.random_palette("QT8", rng) if palette is None else None, stride, plane)
    assert e.value.code == rgb.ERR_ARG and (plane == 0x5A).all()


def test_one_instance_takes_every_kernel_and_growing_sizes_through_the_host_call(dev):
    rng = np.random.default_rng(4)
    for codec, w, h in (("AVI24", 5, 3), ("QT1", 720, 2), ("QT32", 67, 2), ("AVI8", 720, 2), ("MTV16", 2, 2), ("QT4", 2, 1)):
        packet = R.random_packet(codec, w, h, rng)
        palette = R.random_palette(codec, rng) if R.layout(codec, w, h).palette_entries else None
        assert np.array_equal(dev.unpack_frame(codec, w, h, packet, palette), R.unpack(codec, w, h, packet, palette))


def test_unpack_packets_convenience(dev):
    rng = np.random.default_rng(6)
    packets = np.stack([R.random_packet("QT2", 12, 2, rng) for _ in range(4)])
    palettes = np.stack([R.random_palette("QT2", rng) for _ in range(3)])
    of = [2, 0, 1, 2]
    pics = dev.unpack_packets("QT2", 12, 2, packets, palettes, of)
    for i in range(4):
        assert np.array_equal(pics[i], R.unpack("QT2", 12, 2, packets[i], palettes[of[i]]))
    packets = np.stack([R.random_packet("AVI16", 5, 3, rng) for _ in range(2)])
    pics = dev.unpack_packets("AVI16", 5, 3, packets)
    assert all(np.array_equal(pics[i], R.unpack("AVI16", 5, 3, packets[i])) for i in range(2))


# ------------------------------------------------------------------ mi_rgb_times
def test_times_counts_the_launches_and_resets(dev):
    lay = R.layout("AVI24", 720, 2)
    rng = np.random.default_rng(8)
    src = Slots(dev, lay.packet_bytes, lay.packet_bytes, 2, [R.random_packet("AVI24", 720, 2, rng) for _ in range(2)])
    dst = Slots(dev, lay.picture_bytes, lay.picture_bytes, 2, None)
    try:
        dev.times()
        assert dev.times() == (0.0, 0)
        for _ in range(3):
            dev.unpack_batch("AVI24", 720, 2, src.base, lay.packet_bytes, 2, dst.base, lay.picture_bytes)
        dev.unpack_frame("QT8", 5, 3, R.random_packet("QT8", 5, 3, rng), R.random_palette("QT8", rng))  # one launch too
        ms, launches = dev.times()
        assert launches == 4 and ms > 0
        assert dev.times() == (0.0, 0)
    finally:
        src.free()
        dst.free()
