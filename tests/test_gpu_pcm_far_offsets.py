"""mi_pcm_decode_batch with packets, sample slots and counts across, at and above byte 2^31 and byte 2^32 of their buffers,
against the statement (tests/pcmraw.py), byte for byte.

Every lane of k_pcm_decode makes its addresses out of the call's 64-bit bases, the packet's 64-bit offsets and a position
inside the packet that is widened before it is added, and the count of packet i lies at d_outside + 4 i; an offset narrowed
to 32 bits passes every test of a few small packets.  Both buffers are far_offsets.BUFFER_BYTES long.  Eight packets lie
where far_offsets.layout puts packets, in its three variants (the first bytes across a line, the later ones across it, the
packet at it); their sample slots lie where it puts pictures, in its two.  The counts lie near the top of the samples'
buffer, above 2^32, and are an object of the layout like the slots: their alias window, 2^32 below, must stay as it was,
like every byte around every object.  Three codecs: S24BE, LPCM20 and F64BE have three group sizes and three output widths."""
import importlib

import numpy as np
import pytest

import far_offsets as FO
import pcmraw as R

pytestmark = pytest.mark.gpu

FILL = 0xA5
K = 8
TOP = FO.BUFFER_BYTES - (1 << 20)  # the counts
CODECS = ("S24BE", "LPCM20", "F64BE")
CH = 3
pcm = importlib.import_module("gmerlin-avdecoder_amd.pcm")


@pytest.fixture(scope="module")
def far():
    dev = pcm.MiPcm(0)
    d_packets, d_samples = dev.alloc(FO.BUFFER_BYTES), dev.alloc(FO.BUFFER_BYTES)
    yield dev, d_packets, d_samples
    dev.free(d_packets)
    dev.free(d_samples)
    dev.close()


def noise(offsets):
    """bytes that depend on where they lie: what an alias window of a packet holds differs from the packet above it"""
    return ((offsets * np.uint64(2654435761)) >> np.uint64(13)).astype(np.uint8)


def fill(offsets):
    return np.full(offsets.size, FILL, np.uint8)


def packets_of(c):
    """eight packets of a tile and a bit, with a group tail and a byte under a frame; the float ones mostly outside the domain"""
    rng = np.random.default_rng(41 + c)
    a, b, g = R.GROUPS[c]
    n = pcm.TILE_BYTES * a // b + 64
    return [rng.integers(0, 256, n + 7 * i + (i % 3), dtype=np.uint8).tobytes() for i in range(K)]


def outputs_layout(c, variant):
    """the slots where far_offsets puts pictures, then the counts near the top"""
    sizes = [R.layout(c, CH, len(p))[3] for p in packets_of(c)]
    lay = FO.layout(sizes, "pictures", variant)
    return FO.Layout("pictures", variant, sizes + [4 * K], lay.roles + [("above", FO.LINES[1])], [int(o) for o in lay.offsets] + [TOP])


@pytest.mark.parametrize("variant", FO.PICTURE_VARIANTS)
@pytest.mark.parametrize("name", CODECS)
def test_the_arithmetic_of_the_layouts(name, variant):
    c = R.codec(name)
    lay = outputs_layout(c, variant)
    have = FO.check_layout(lay)
    assert FO.required_roles(variant) <= have
    assert all(int(o) % 16 == 0 for o in lay.offsets)
    assert lay.alias[K]  # the counts have an alias window of their own
    for pv in FO.PACKET_VARIANTS:
        assert FO.required_roles(pv) <= FO.check_layout(FO.layout([len(p) for p in packets_of(c)], "packets", pv))


@pytest.mark.parametrize("packet_variant", FO.PACKET_VARIANTS)
@pytest.mark.parametrize("variant", FO.PICTURE_VARIANTS)
@pytest.mark.parametrize("name", CODECS)
def test_decode_batch_packets_slots_and_counts_across_at_and_above_the_lines(far, name, variant, packet_variant):
    dev, d_packets, d_samples = far
    c = R.codec(name)
    packets = packets_of(c)
    lay_p = FO.layout([len(p) for p in packets], "packets", packet_variant)
    lay_o = outputs_layout(c, variant)
    FO.check_layout(lay_p)
    FO.fill_windows(dev, d_packets, lay_p, noise)
    for (a, _), p in zip(lay_p.spans, packets):
        dev.h2d(d_packets, np.frombuffer(p, np.uint8), offset=a)
    before = FO.read_windows(dev, d_packets, lay_p)
    FO.fill_windows(dev, d_samples, lay_o, fill)
    at_counts = int(lay_o.offsets[K])
    dev.times()
    dev.decode_batch(c, CH, d_packets, lay_p.offsets, [len(p) for p in packets], d_samples, lay_o.offsets[:K], d_samples + at_counts)
    dev.sync()
    assert dev.times()[1] == 2
    wins = FO.read_windows(dev, d_samples, lay_o)
    counts = []
    for i, p in enumerate(packets):
        want, k = R.decode(c, CH, p)
        got = FO.cut(lay_o, wins, lay_o.spans[i])
        if not np.array_equal(got, want):
            d = np.flatnonzero(got != want)
            raise AssertionError(f"packet {i}: packet {lay_p.describe(i)}, samples {lay_o.describe(i)}: {d.size} bytes differ from the "
                                 f"statement's, first at byte {int(d[0])}; " + FO.alias_report(lay_o, wins, i, want, fill))
        counts.append(k)
    want = np.array(counts, np.uint32).view(np.uint8)
    got = FO.cut(lay_o, wins, lay_o.spans[K])
    assert np.array_equal(got, want), "the counts: " + FO.alias_report(lay_o, wins, K, want, fill)
    assert (name == "F64BE") == any(counts)
    stray = FO.outside_objects(lay_o, wins, fill)
    assert stray is None, f"byte {stray[0]:#x} outside every object is {stray[1]:#x} ({stray[2]} such bytes; in an alias window: {stray[3]})"
    after = FO.read_windows(dev, d_packets, lay_p)
    assert all(np.array_equal(x, y) for x, y in zip(before, after)), "a packet was written"
    print("FAR-OFFSETS PCM", name, variant, packet_variant, f"packets at {[hex(int(o)) for o in lay_p.offsets]}, samples at "
          f"{[hex(int(o)) for o in lay_o.offsets[:K]]}, counts at {at_counts:#x}", flush=True)
