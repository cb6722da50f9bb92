"""mi_gsm_decode_batch with streams, sample slots, states and counts across, at and above byte 2^31 and byte 2^32 of their
buffers, against the statement (tests/gsmraw.py), byte for byte.

Every lane of k_gsm_decode makes its own addresses out of the call's 64-bit bases and the stream's 64-bit offsets, and the
state of stream i lies at d_state + 288 i; an offset narrowed to 32 bits passes every test of a few small streams.  Both
buffers are far_offsets.BUFFER_BYTES long.  Eight two-unit streams lie where far_offsets.layout puts packets, in its three
variants (the first bytes across a line, the later ones across it, the stream at it); their sample slots lie where it puts
pictures, in its two.  The states and the counts lie near the top of the samples' buffer, above 2^32, and are objects of the
layout like the slots: their alias windows, 2^32 below, must stay as they were, like every byte around every object."""
import importlib

import numpy as np
import pytest

import far_offsets as FO
import gsmraw as G

pytestmark = pytest.mark.gpu

FILL = 0xA5
K = 8
TOP = FO.BUFFER_BYTES - (1 << 20)  # states from here, counts a guard behind them


@pytest.fixture(scope="module")
def far():
    gsm = importlib.import_module("gmerlin-avdecoder_amd.gsm")
    dev = gsm.MiGsm(0)
    d_stream, d_pcm = dev.alloc(FO.BUFFER_BYTES), dev.alloc(FO.BUFFER_BYTES)
    yield dev, d_stream, d_pcm
    dev.free(d_stream)
    dev.free(d_pcm)
    dev.close()


def noise(offsets):
    """bytes that depend on where they lie: what an alias window of the stream holds differs from the stream above it"""
    return ((offsets * np.uint64(2654435761)) >> np.uint64(13)).astype(np.uint8)


def fill(offsets):
    return np.full(offsets.size, FILL, np.uint8)


def outputs_layout(fmt, variant):
    """the slots where far_offsets puts pictures, then the states and the counts near the top"""
    slot = 2 * 2 * G.FRAME_SAMPLES * (1 + fmt)
    lay = FO.layout([slot] * K, "pictures", variant)
    at_state = TOP
    at_bad = TOP + 288 * K + 2 * FO.GUARD
    return FO.Layout("pictures", variant, [slot] * K + [288 * K, 4 * K], lay.roles + [("above", FO.LINES[1])] * 2,
                     [int(o) for o in lay.offsets] + [at_state, at_bad])


@pytest.mark.parametrize("variant", FO.PICTURE_VARIANTS)
@pytest.mark.parametrize("fmt", (0, 1))
def test_the_arithmetic_of_the_layouts(fmt, variant):
    lay = outputs_layout(fmt, variant)
    have = FO.check_layout(lay)
    assert FO.required_roles(variant) <= have
    assert all(int(o) % 16 == 0 for o in lay.offsets)
    assert lay.alias[K] and lay.alias[K + 1]  # states and counts have alias windows of their own
    for pv in FO.PACKET_VARIANTS:
        assert FO.required_roles(pv) <= FO.check_layout(FO.layout([2 * G.unit_bytes(fmt)] * K, "packets", pv))


@pytest.mark.parametrize("packet_variant", FO.PACKET_VARIANTS)
@pytest.mark.parametrize("variant", FO.PICTURE_VARIANTS)
@pytest.mark.parametrize("fmt", (0, 1))
def test_decode_batch_streams_slots_states_and_counts_across_at_and_above_the_lines(far, fmt, variant, packet_variant):
    dev, d_stream, d_pcm = far
    rng = np.random.default_rng(23 + fmt)
    streams = [b"".join(G.implode(G.random_params(rng, fmt), fmt) for _ in range(2)) for _ in range(K)]
    if fmt == 0:  # one stream's second frame has a bad magic: its count is not 0
        streams[3] = streams[3][:33] + bytes([0x10 | streams[3][33] & 15]) + streams[3][34:]
    lay_s = FO.layout([len(s) for s in streams], "packets", packet_variant)
    lay_o = outputs_layout(fmt, variant)
    FO.check_layout(lay_s)
    FO.fill_windows(dev, d_stream, lay_s, noise)
    for (a, _), s in zip(lay_s.spans, streams):
        dev.h2d(d_stream, np.frombuffer(s, np.uint8), offset=a)
    before = FO.read_windows(dev, d_stream, lay_s)
    FO.fill_windows(dev, d_pcm, lay_o, fill)
    # the states the streams start from: those after another unit, so that a state read at a wrong place shows
    first = [G.decode_stream(G.implode(G.random_params(rng, fmt), fmt), fmt)[1].words() for _ in range(K)]
    at_state, at_bad = int(lay_o.offsets[K]), int(lay_o.offsets[K + 1])
    dev.h2d(d_pcm, np.concatenate(first).view(np.uint8), offset=at_state)
    dev.times()
    dev.decode_batch(d_stream, lay_s.offsets, np.full(K, 2, np.uint32), fmt, d_pcm, lay_o.offsets[:K], d_pcm + at_state, d_pcm + at_bad)
    dev.sync()
    assert dev.times()[1] == 1
    wins = FO.read_windows(dev, d_pcm, lay_o)
    want_states, want_bad = [], []
    for i, s in enumerate(streams):
        pcm, S, bad = G.decode_stream(s, fmt, G.State.from_words(first[i]))
        want = pcm.view(np.uint8)
        got = FO.cut(lay_o, wins, lay_o.spans[i])
        if not np.array_equal(got, want):
            d = np.flatnonzero(got != want)
            raise AssertionError(f"stream {i}: stream {lay_s.describe(i)}, samples {lay_o.describe(i)}: {d.size} bytes differ from the "
                                 f"statement's, first at byte {int(d[0])}; " + FO.alias_report(lay_o, wins, i, want, fill))
        want_states.append(S.words())
        want_bad.append(bad)
    want = np.concatenate(want_states).view(np.uint8)
    got = FO.cut(lay_o, wins, lay_o.spans[K])
    assert np.array_equal(got, want), "the states: " + FO.alias_report(lay_o, wins, K, want, fill)
    want = np.array(want_bad, np.uint32).view(np.uint8)
    got = FO.cut(lay_o, wins, lay_o.spans[K + 1])
    assert np.array_equal(got, want), "the counts: " + FO.alias_report(lay_o, wins, K + 1, want, fill)
    assert fmt == 1 or want_bad[3] == 1
    stray = FO.outside_objects(lay_o, wins, fill)
    assert stray is None, f"byte {stray[0]:#x} outside every object is {stray[1]:#x} ({stray[2]} such bytes; in an alias window: {stray[3]})"
    after = FO.read_windows(dev, d_stream, lay_s)
    assert all(np.array_equal(x, y) for x, y in zip(before, after)), "the stream was written"
    print("FAR-OFFSETS GSM", fmt, variant, packet_variant, f"streams at {[hex(int(o)) for o in lay_s.offsets]}, samples at "
          f"{[hex(int(o)) for o in lay_o.offsets[:K]]}, states at {at_state:#x}, counts at {at_bad:#x}", flush=True)
