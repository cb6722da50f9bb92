"""libmi_spu.so on the device against the statement (tests/spuraw.py), byte for byte: rectangles of every width that meets the
16-byte pieces of a row, in frames whose rows begin at every alignment; every code length at each of the last four nibbles of
the walker's window; dense and empty rows; every shape of a field upstream defines; the control section's quirks; batches
with two palettes, every status between two good packets, the refusals of the call, the host call and the launch counts.
Packets lie at odd byte addresses of one stream; 256 bytes of 0xA5 lie around the stream, the pictures and the infos and
between the picture slots, every byte outside a picture is checked, and the slots themselves start as 0xA5: a good packet's
zeros are the library's."""
import importlib

import numpy as np
import pytest

import spuraw as S

pytestmark = pytest.mark.gpu

GUARD, FILL = 256, 0xA5
WINDOW = 64  # nibbles the walker classifies at once
FRAMES = ((4, 2), (5, 3), (67, 6), (720, 8))


@pytest.fixture(scope="module")
def spu():
    return importlib.import_module("gmerlin-avdecoder_amd.spu")


@pytest.fixture(scope="module")
def dev(spu):
    d = spu.MiSpu(0)
    yield d
    d.close()


class Guarded:
    """a device buffer of `host`'s bytes"""

    def __init__(self, dev, host):
        self.dev, self.host = dev, host
        self.d = dev.alloc(host.size)
        dev.h2d(self.d, host)

    def read(self):
        return self.dev.d2h(self.d, self.host.size)

    def free(self):
        self.dev.free(self.d)


def lay_stream(packets):
    """one stream: a guard, the packets at odd byte addresses with 1 to 7 bytes of fill between them, a guard"""
    offsets, cur = [], GUARD
    for i, p in enumerate(packets):
        cur += 1 + (3 * i) % 7
        cur += 1 - cur % 2  # odd
        offsets.append(cur)
        cur += p.size
    host = np.full(cur + GUARD, FILL, np.uint8)
    for o, p in zip(offsets, packets):
        host[o:o + p.size] = p
    return host, np.array(offsets, np.uint64), np.array([p.size for p in packets], np.uint32)


def decode_and_judge(dev, spu, packets, W, H, palettes, palette_of=None, what=""):
    """the packets through mi_spu_decode_batch; the infos, the pictures, the guards and the stream against the statement.
    Returns the statuses."""
    n, size = len(packets), W * H * 4
    palettes = np.atleast_2d(palettes)
    host, offsets, lengths = lay_stream(packets)
    qs = (size + 15) // 16 * 16 + GUARD
    pics = np.full(2 * GUARD + (n - 1) * qs + size, FILL, np.uint8)
    inf = np.full(2 * GUARD + spu.INFO_BYTES * n, FILL, np.uint8)
    src, dst, dinf = Guarded(dev, host), Guarded(dev, pics), Guarded(dev, inf)
    try:
        dev.decode_batch(src.d, offsets, lengths, W, H, dst.d + GUARD, qs, palettes, dinf.d + GUARD, palette_of)
        dev.sync()
        got_pics, got_inf = dst.read(), dinf.read()
        assert np.array_equal(src.read(), host), "the stream was written"
    finally:
        src.free(), dst.free(), dinf.free()
    want_pics, keep = pics.copy(), np.ones(pics.size, bool)
    want_infos = []
    for i, p in enumerate(packets):
        st, pic, info = S.decode(p, W, H, palettes[0 if palette_of is None else palette_of[i]])
        want_infos.append(info)
        a = GUARD + i * qs
        if st == S.OK:
            want_pics[a:a + size] = pic.reshape(-1)
        elif st == S.DATA_RANGE:
            keep[a:a + size] = False
    assert np.array_equal(got_inf[:GUARD], inf[:GUARD]) and np.array_equal(got_inf[GUARD + spu.INFO_BYTES * n:], inf[:GUARD]), "the infos' guards"
    got_infos = spu.infos(got_inf[GUARD:GUARD + spu.INFO_BYTES * n])
    for i, (got, want) in enumerate(zip(got_infos, want_infos)):
        if want.status == S.DATA_RANGE:
            assert got.status == S.DATA_RANGE, f"{what}: packet {i} has status {got.status}, the statement's is DATA_RANGE"
        else:
            assert tuple(got) == tuple(want), f"{what}: packet {i}:\n{got}\nthe statement's\n{want}"
    bad = np.flatnonzero((got_pics != want_pics) & keep)
    if bad.size:
        at = int(bad[0]) - GUARD
        slot, byte = at // qs, at % qs
        where = "the guard in front" if at < 0 else f"slot {slot} byte {byte} (row {byte // (4 * W)}, pixel {byte % (4 * W) // 4}; picture bytes {size})"
        raise AssertionError(f"{what} {W} x {H}, batch of {n}: {bad.size} bytes differ from the statement's, first in {where}: "
                             f"{int(got_pics[bad[0]]):#x}, not {int(want_pics[bad[0]]):#x}")
    return [i.status for i in want_infos]


def widths(W):
    """1, W and the widths 4k - 1, 4k + 1 that fit"""
    return sorted({1, W} | {w for k in (1, 2, 5, 16) for w in (4 * k - 1, 4 * k + 1) if w <= W})


@pytest.mark.parametrize("W,H", FRAMES, ids=[f"{w}x{h}" for w, h in FRAMES])
def test_rectangles_of_every_width_in_every_frame(dev, spu, W, H):
    rng = np.random.default_rng(W + H)
    pal = S.random_palette(rng)
    packets = []
    for k, width in enumerate(widths(W)):
        idx = S.random_indices(rng, H, width, 1 + 3 * (k % 3))
        packets.append(S.encode(idx, x1=k, y1=2 * k, fill_ends=bool(k % 2), wide=k % 3 == 2))
    assert decode_and_judge(dev, spu, packets, W, H, pal, what="widths") == [0] * len(packets)
    assert decode_and_judge(dev, spu, packets[-1:], W, H, pal, what="n = 1") == [0]


def nibble_count(row):
    """the nibbles of a row's line without fill codes and without the pad"""
    return sum(len(S.code(part, c)) for length, c in S.runs_of(row) for part in [255] * (length // 255) + [length % 255] * bool(length % 255))


def placed(nibble, code_nibbles, width):
    """a row of `width` whose code of `code_nibbles` nibbles starts at `nibble` of its line, behind one-nibble codes"""
    run = {1: 2, 2: 9, 3: 40, 4: 200}[code_nibbles]
    row = np.concatenate([np.arange(nibble) % 2, np.full(run, 2), [3, 1, 1, 0, 3]]).astype(np.uint8)
    row = np.concatenate([row, np.zeros(width - row.size, np.uint8)])
    nib = S.line_nibbles(row, False)
    assert nib[nibble:nibble + code_nibbles] == S.code(run, 2) and nib[:nibble] == [4 + (k % 2) for k in range(nibble)]
    return row


@pytest.mark.parametrize("code_nibbles", (1, 2, 3, 4))
def test_every_code_length_at_the_last_four_nibbles_of_a_window(dev, spu, code_nibbles):
    rng = np.random.default_rng(code_nibbles)
    pal = S.random_palette(rng)
    W, H = 720, 8
    rows = [placed(window * WINDOW - back, code_nibbles, 624) for window in (1, 2) for back in (4, 3, 2, 1)]
    assert sum(nibble_count(r) % 2 for r in rows) >= 2  # lines that end on an odd nibble
    packets = []
    for fill_ends, order in ((False, 1), (True, 1), (False, -1)):
        f1, f2 = rows[0::2][::order], rows[1::2][::order]
        packets.append(S.build(S.field_bytes(f1, fill_ends), S.field_bytes(f2, fill_ends), [S.usual(0, 623, 0, 7)]))
    assert decode_and_judge(dev, spu, packets, W, H, pal, what=f"codes of {code_nibbles} nibbles") == [0, 0, 0]


def test_dense_and_empty_rows(dev, spu):
    rng = np.random.default_rng(3)
    pal = S.random_palette(rng)
    # 40 consecutive lines a field that are one fill code each, in a frame of odd height
    empty = np.repeat(rng.integers(0, 4, (80, 1)), 33, axis=1).astype(np.uint8)
    p = S.encode(empty, 5, 5)
    assert S.be16(p, 2) == 4 + 2 * 2 * 40  # two bytes a line
    assert decode_and_judge(dev, spu, [p], 67, 81, pal, what="fill lines") == [0]
    # a 130-pixel row of 16-bit codes of len 1: several windows a line
    dense = (np.arange(130)[None, :] + np.arange(4)[:, None]).astype(np.uint8) % 4
    p = S.encode(dense, fill_ends=False, wide=True)
    assert S.be16(p, 2) == 4 + 4 * 130 * 2
    q = S.encode(dense[:, :129], fill_ends=True, wide=True)
    assert decode_and_judge(dev, spu, [p, q, p], 130, 4, pal, what="16-bit codes of len 1") == [0, 0, 0]


def test_field_shapes(dev, spu):
    rng = np.random.default_rng(4)
    pal = S.random_palette(rng)
    idx = S.random_indices(rng, 6, 50, 4)
    W, H = 67, 6
    shapes = {"the clamp": S.clamped(50, 6), "field 1 ends mid-line": S.field_ends_mid_line(idx),
              "fewer lines than the rectangle": S.fewer_lines(idx[:2], 6), "offset2 < offset1": S.reversed_offsets(idx),
              "no 06": S.no_offsets(idx), "lines beyond y2": S.lines_beyond_y2(idx, 1)}
    assert decode_and_judge(dev, spu, list(shapes.values()), W, H, pal, what="/".join(shapes)) == [0] * len(shapes)
    # more lines than H / 2, and an odd H: the last row is nobody's line
    more = S.encode(S.random_indices(rng, 12, 5, 2))
    for w, h in ((5, 3), (67, 6), (67, 5)):
        assert decode_and_judge(dev, spu, [more, S.clamped(5, 2)], w, h, pal, what=f"12 lines into {h} rows") == [0, 0]


def test_control_sections(dev, spu):
    rng = np.random.default_rng(5)
    pal = S.random_palette(rng)
    idx = S.random_indices(rng, 6, 31, 3)
    packets = [S.two_sequences(idx, 40, 3), S.unknown_command(idx), S.encode(idx, 3, 1, (15, 0, 9, 4), (1, 2, 3, 4))]
    st = decode_and_judge(dev, spu, packets, 67, 6, pal, what="control sections")
    assert st == [0, 0, 0]
    pics, infos = dev.decode_packets(packets, 67, 6, pal)
    assert infos[0].sequences == 2 and infos[0].palette == (7, 9, 4, 12) and infos[0].alpha == (15, 3, 0, 9) and infos[0].dst_x == 36
    assert infos[1].alpha == (1, 2, 3, 4)
    assert np.array_equal(pics[0].reshape(6, 67, 4), S.expected(idx, 67, 6, infos[0], pal))


def test_two_palettes_and_batches_of_1_and_70(dev, spu):
    rng = np.random.default_rng(6)
    pals = np.stack([S.random_palette(rng), S.random_palette(rng)])
    packets = [S.encode(S.random_indices(rng, 6, 1 + (7 * k) % 67, 1 + k % 5), fill_ends=bool(k % 3)) for k in range(70)]
    of = (np.arange(70) * 5 // 3 % 2).astype(np.uint16)
    assert decode_and_judge(dev, spu, packets, 67, 6, pals, of, what="two palettes") == [0] * 70
    assert decode_and_judge(dev, spu, packets[:1], 67, 6, pals[:1], what="n = 1") == [0]
    assert decode_and_judge(dev, spu, packets[:3], 67, 6, pals, [1, 1, 0], what="n = 3") == [0] * 3


BAD_NAMES = sorted(S.bad_packets(720, 8))


@pytest.mark.parametrize("name", BAD_NAMES)
def test_every_status_between_two_good_packets(dev, spu, name):
    W, H = 720, 8
    bad, status = S.bad_packets(W, H)[name]
    rng = np.random.default_rng(len(name))
    pal = S.random_palette(rng)
    good = [S.encode(S.random_indices(rng, 8, 300, 9)), S.encode(S.random_indices(rng, 8, 720, 30), fill_ends=False)]
    assert decode_and_judge(dev, spu, [good[0], bad, good[1]], W, H, pal, what=name) == [0, status, 0]


def test_call_refusals_launch_nothing_and_write_nothing(dev, spu):
    rng = np.random.default_rng(7)
    pal = S.random_palette(rng)[None]
    packets = [S.encode(S.random_indices(rng, 2, 5, 2)) for _ in range(3)]
    host, offsets, lengths = lay_stream(packets)
    qs = 64 + GUARD  # 5 x 3 x 4 = 60
    pics, inf = np.full(2 * GUARD + 3 * qs, FILL, np.uint8), np.full(2 * GUARD + 3 * spu.INFO_BYTES, FILL, np.uint8)
    src, dst, dinf = Guarded(dev, host), Guarded(dev, pics), Guarded(dev, inf)
    base = dict(d_stream=src.d, offsets=offsets, lengths=lengths, w=5, h=3, d_pics=dst.d + GUARD, pic_stride=qs, palettes=pal,
                d_info=dinf.d + GUARD, palette_of=None)
    refusals = {
        "no packets": dict(offsets=offsets[:0], lengths=lengths[:0]),
        "width 0": dict(w=0), "height 0": dict(h=0), "width 4097": dict(w=4097, pic_stride=4097 * 3 * 4 + 12), "height 4097": dict(h=4097, pic_stride=4097 * 5 * 4 + 12),
        "pictures not aligned": dict(d_pics=dst.d + GUARD + 8), "stride not aligned": dict(pic_stride=qs + 8),
        "stride below the picture": dict(pic_stride=48), "no stream": dict(d_stream=None), "no pictures": dict(d_pics=None),
        "no infos": dict(d_info=None), "infos not aligned": dict(d_info=dinf.d + GUARD + 2),
        "palette index 1 of 1": dict(palette_of=[0, 1, 0]),
        "4 palettes for 3 packets": dict(palettes=np.repeat(pal, 4, axis=0)),
        "a packet of 2^30 bytes": dict(lengths=np.array([lengths[0], 1 << 30, lengths[2]], np.uint32)),
        "a packet inside the pictures": dict(offsets=np.array([offsets[0], (dst.d + GUARD + 4 - src.d) % (1 << 64), offsets[2]], np.uint64)),
        "the infos inside the pictures": dict(d_info=dst.d + GUARD + 16),
    }
    try:
        dev.sync()
        dev.times()
        for name, change in refusals.items():
            with pytest.raises(spu.MiSpuError) as e:
                dev.decode_batch(**{**base, **change})
            assert e.value.code == spu.ERR_ARG, name
        L = dev.L
        o, ln = offsets.ctypes.data_as(spu.u64p), lengths.ctypes.data_as(spu.u32p)
        for name, args in {"no palettes": (None, 1, None), "no palettes counted": (pal.ctypes.data_as(spu.u32p), 0, None)}.items():
            assert L.mi_spu_decode_batch(dev.c, src.d, o, ln, 3, 5, 3, dst.d + GUARD, qs, *args, dinf.d + GUARD) == spu.ERR_ARG, name
        assert L.mi_spu_decode_batch(dev.c, src.d, None, ln, 3, 5, 3, dst.d + GUARD, qs, pal.ctypes.data_as(spu.u32p), 1, None, dinf.d + GUARD) == spu.ERR_ARG
        assert L.mi_spu_decode_batch(dev.c, src.d, o, ln, 65536, 5, 3, dst.d + GUARD, qs, pal.ctypes.data_as(spu.u32p), 1, None, dinf.d + GUARD) == spu.ERR_ARG
        dev.sync()
        assert dev.times()[1] == 0
        assert np.array_equal(dst.read(), pics) and np.array_equal(dinf.read(), inf) and np.array_equal(src.read(), host)
        dev.decode_batch(**base)  # and the call itself is good
        dev.sync()
        assert dev.times()[1] == 2 and [i.status for i in spu.infos(dinf.read()[GUARD:GUARD + 3 * spu.INFO_BYTES])] == [0, 0, 0]
    finally:
        src.free(), dst.free(), dinf.free()


def test_decode_frame_at_a_wide_stride(dev, spu):
    rng = np.random.default_rng(11)
    pal = S.random_palette(rng)
    for W, H, p in ((67, 6, S.encode(S.random_indices(rng, 6, 50, 4), 30, 2)), (5, 3, S.clamped(5, 2)),
                    (720, 8, S.encode(S.random_indices(rng, 8, 719, 20), fill_ends=False))):
        st, want, info = S.decode(p, W, H, pal)
        stride = W * 4 + 12
        plane = np.full(stride * H, FILL, np.uint8)
        got, head = dev.decode_frame(p, W, H, pal, stride, plane)
        assert st == 0 and tuple(head) == tuple(info)
        rows = got.reshape(H, stride)
        assert np.array_equal(rows[:, :W * 4].reshape(H, W, 4), want) and (rows[:, W * 4:] == FILL).all()
    bad = S.bad_packets(720, 8)
    for name in ("three bytes", "no ff before the end", "width 0", "field 1 runs off the packet", "field 2 runs off the packet"):
        plane = np.full(720 * 8 * 4, FILL, np.uint8)
        with pytest.raises(spu.MiSpuError) as e:
            dev.decode_frame(bad[name][0], 720, 8, pal, 720 * 4, plane)
        assert e.value.code == spu.ERR_FORMAT and e.value.status == bad[name][1] and (plane == FILL).all(), name
    with pytest.raises(spu.MiSpuError) as e:
        dev.decode_frame(S.clamped(5, 2), 5, 3, pal, 19, np.zeros(64, np.uint8))
    assert e.value.code == spu.ERR_ARG


def test_times_counts_two_launches_a_call(dev, spu):
    rng = np.random.default_rng(12)
    pal = S.random_palette(rng)
    dev.sync()
    dev.times()
    packets = [S.encode(S.random_indices(rng, 6, 40, 3)) for _ in range(3)]
    pics, infos = dev.decode_packets(packets, 67, 6, pal)
    assert [i.status for i in infos] == [0, 0, 0]
    assert all(np.array_equal(pics[i].reshape(6, 67, 4), S.decode(packets[i], 67, 6, pal)[1]) for i in range(3))
    dev.decode_packets(packets[:1], 67, 6, pal)
    ms, launches = dev.times()
    assert launches == 4 and len(ms) == 2 and all(m >= 0 for m in ms)
    assert dev.times()[1] == 0
