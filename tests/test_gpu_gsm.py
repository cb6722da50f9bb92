"""libmi_gsm.so on the device against the statement (tests/gsmraw.py), byte for byte: samples, states and counts.

Streams lie at odd byte addresses of one buffer, sample slots at multiples of 16 that are mostly none of 256, with GUARD
bytes of 0xA5 around and between everything, states and counts included.  Every buffer is compared whole with what it must
hold afterwards, so every byte outside the named outputs is checked, and the stream must come back as it was.

The kernel stages no output (a lane stores the 16 bytes of eight samples as it makes them), so there is no staging length
whose neighbours would need shapes of their own; the shapes are one stream of one unit, one of two (the carry inside a
call), and 65 streams of 0, 1, 2, 3, 5 and 7 units in turn (one past a wave, lanes that end at different times, empty
streams), in both framings."""
import importlib
import json
import os

import numpy as np
import pytest

import gsmraw as G
from pkg import ROOT

pytestmark = pytest.mark.gpu

GUARD, FILL = 256, 0xA5
VECTORS = json.load(open(os.path.join(ROOT, "tests", "golden", "gsm_vectors.json")))["vectors"]
SHORT = [v for v in VECTORS if "pcm" in v]


@pytest.fixture(scope="module")
def dev():
    gsm = importlib.import_module("gmerlin-avdecoder_amd.gsm")
    d = gsm.MiGsm(0)
    yield d
    d.close()


_seen = {}


def statement(data, fmt, state=None):
    """(samples, state words after, bad) of the statement, computed once for the same bytes, framing and state"""
    key = (bytes(data), fmt, None if state is None else np.asarray(state, np.int16).tobytes())
    if key not in _seen:
        pcm, S, bad = G.decode_stream(data, fmt, None if state is None else G.State.from_words(state))
        _seen[key] = (pcm, S.words(), bad)
    return _seen[key]


def pool(fmt, count, units, seed):
    """`count` distinct streams of `units` units from the statement's packer over seeded parameters"""
    rng = np.random.default_rng(seed)
    return [b"".join(G.implode(G.random_params(rng, fmt), fmt) for _ in range(units)) for _ in range(count)]


class Run:
    """one call over the given streams: lays out the four buffers, calls, reads them back whole"""

    def __init__(self, dev, streams, fmt, states=None, with_state=True, with_bad=True, units=None):
        n = len(streams)
        self.units = np.array([len(s) // G.unit_bytes(fmt) for s in streams] if units is None else units, np.uint32)
        # the stream buffer: every stream at an odd address
        at, offs = GUARD, []
        for s in streams:
            at += 1 - at % 2
            offs.append(at)
            at += len(s) + GUARD
        stream = np.full(at, FILL, np.uint8)
        for o, s in zip(offs, streams):
            stream[o:o + len(s)] = np.frombuffer(s, np.uint8)
        # the sample slots: multiples of 16, every other one no multiple of 256
        at, pcm_offs = 0, []
        for i, u in enumerate(self.units):
            at = (at + GUARD + 255) // 256 * 256 + (16 * (1 + i % 15) if i % 2 == 0 else 0)
            pcm_offs.append(at)
            at += int(u) * 2 * G.FRAME_SAMPLES * (1 + fmt)
        pcm = np.full(at + GUARD, FILL, np.uint8)
        st = np.full(2 * GUARD + n * 288, FILL, np.uint8)
        if with_state:
            fresh = G.State().words()
            for i in range(n):
                st[GUARD + 288 * i:GUARD + 288 * (i + 1)] = (fresh if states is None else np.asarray(states[i], np.int16)).view(np.uint8)
        bad = np.full(2 * GUARD + 4 * n, FILL, np.uint8)
        self.offs, self.pcm_offs, self.stream, self.n, self.fmt = np.array(offs, np.uint64), np.array(pcm_offs, np.uint64), stream, n, fmt
        self.before = (pcm.copy(), st.copy(), bad.copy())
        with dev._resident(stream, pcm, st, bad) as (ds, dp, dst, db):
            dev.times()
            dev.decode_batch(ds, self.offs, self.units, fmt, dp, self.pcm_offs, dst + GUARD if with_state else None, db + GUARD if with_bad else None)
            dev.sync()
            self.launches = dev.times()[1]
            self.stream_after = dev.d2h(ds, stream.nbytes)
            self.pcm, self.st, self.bad = dev.d2h(dp, pcm.nbytes), dev.d2h(dst, st.nbytes), dev.d2h(db, bad.nbytes)

    def expect(self, streams, states=None, with_state=True, with_bad=True):
        """the three buffers as the statement says they must be"""
        pcm, st, bad = (x.copy() for x in self.before)
        for i, s in enumerate(streams):
            used = s[:int(self.units[i]) * G.unit_bytes(self.fmt)]
            p, w, b = statement(used, self.fmt, None if states is None or not with_state else states[i])
            o = int(self.pcm_offs[i])
            pcm[o:o + p.nbytes] = p.view(np.uint8)
            if with_state:
                st[GUARD + 288 * i:GUARD + 288 * (i + 1)] = w.view(np.uint8)
            if with_bad:
                bad[GUARD + 4 * i:GUARD + 4 * i + 4] = np.array([b], np.uint32).view(np.uint8)
        return pcm, st, bad

    def check(self, streams, states=None, with_state=True, with_bad=True):
        pcm, st, bad = self.expect(streams, states, with_state, with_bad)
        assert self.launches == 1
        assert np.array_equal(self.stream_after, self.stream), "the stream was written"
        for name, got, want in (("samples", self.pcm, pcm), ("states", self.st, st), ("counts", self.bad, bad)):
            if not np.array_equal(got, want):
                d = np.flatnonzero(got != want)
                raise AssertionError(f"{name}: {d.size} bytes differ from the statement's, the first at byte {int(d[0])} of the buffer: "
                                     f"{int(got[d[0]]):#x}, not {int(want[d[0]]):#x}")


def shapes(fmt):
    size = G.unit_bytes(fmt)
    a = pool(fmt, 4, 8, 40 + fmt)
    many = [a[i % 4][(i // 4 % 2) * size:][:(0, 1, 2, 3, 5, 7)[i % 6] * size] for i in range(65)]
    return {"one stream of one unit": [a[0][:size]], "one stream of two units": [a[1][:2 * size]], "65 streams": many}


@pytest.mark.parametrize("outputs", ("state and counts", "neither"))
@pytest.mark.parametrize("shape", ("one stream of one unit", "one stream of two units", "65 streams"))
@pytest.mark.parametrize("fmt", (0, 1))
def test_decode_batch_against_the_statement(dev, fmt, shape, outputs):
    streams = shapes(fmt)[shape]
    both = outputs != "neither"
    r = Run(dev, streams, fmt, with_state=both, with_bad=both)
    r.check(streams, with_state=both, with_bad=both)


@pytest.mark.parametrize("fmt", (0, 1))
def test_five_units_equal_two_and_three_through_d_state(dev, fmt):
    size = G.unit_bytes(fmt)
    streams = pool(fmt, 3, 5, 50 + fmt)
    whole = Run(dev, streams, fmt)
    whole.check(streams)
    a = Run(dev, [s[:2 * size] for s in streams], fmt)
    a.check([s[:2 * size] for s in streams])
    carried = [a.st[GUARD + 288 * i:GUARD + 288 * (i + 1)].view(np.int16) for i in range(3)]
    b = Run(dev, [s[2 * size:] for s in streams], fmt, states=carried)
    b.check([s[2 * size:] for s in streams], states=carried)
    assert np.array_equal(b.st, whole.st)
    for i in range(3):
        got = np.concatenate([x.pcm[int(x.pcm_offs[i]):][:u * 320 * (1 + fmt)] for x, u in ((a, 2), (b, 3))])
        o = int(whole.pcm_offs[i])
        assert np.array_equal(got, whole.pcm[o:o + got.size])


@pytest.mark.parametrize("fmt", (0, 1))
def test_every_short_vector_against_upstream_s_recorded_samples(dev, fmt):
    vs = [v for v in SHORT if v["fmt"] == fmt]
    streams = [bytes.fromhex(v["input"]) for v in vs]  # (bad_magic carries a tail: the unit count drops it)
    r = Run(dev, streams, fmt)
    r.check(streams)
    for i, v in enumerate(vs):
        want = np.frombuffer(bytes.fromhex(v["pcm"]), "<i2").reshape(-1, 160)
        o = int(r.pcm_offs[i])
        got = r.pcm[o:o + want.nbytes].view(np.int16).reshape(-1, 160)
        for f in range(want.shape[0]):
            assert np.array_equal(got[f], want[f]) or f in v["not_compared"], (v["name"], f)
        s = v["state"]
        assert [int(x) for x in r.st[GUARD + 288 * i:GUARD + 288 * (i + 1)].view(np.int16)] == s["dp"] + s["v"] + [s["msr"], s["nrp"]] + s["LARpp"] + [0] * 5
        assert int(r.bad[GUARD + 4 * i:GUARD + 4 * i + 4].view(np.uint32)[0]) == len(v["not_compared"])


def test_a_bad_magic_first_in_the_middle_and_last(dev):
    good = pool(0, 1, 3, 60)[0]
    streams = []
    for where in (0, 1, 2, None):
        s = bytearray(good)
        if where is not None:
            s[33 * where] = 0x50 | s[33 * where] & 15
        streams.append(bytes(s))
    streams.append(bytes([0x00]) + good[1:33])  # a stream that is one bad frame
    r = Run(dev, streams, 0)
    r.check(streams)
    counts = r.bad[GUARD:GUARD + 20].view(np.uint32)
    assert list(counts) == [1, 1, 1, 0, 1]
    for i, where in enumerate((0, 1, 2)):
        o = int(r.pcm_offs[i]) + 320 * where
        assert not r.pcm[o:o + 320].any()
    assert np.array_equal(r.st[GUARD + 4 * 288:GUARD + 5 * 288].view(np.int16), G.State().words())  # untouched: still fresh
    without = Run(dev, streams, 0, with_state=False, with_bad=False)
    without.check(streams, with_state=False, with_bad=False)


def test_the_refusals_launch_nothing(dev):
    gsm = importlib.import_module("gmerlin-avdecoder_amd.gsm")
    s = pool(0, 1, 1, 70)[0]
    stream = np.frombuffer(s, np.uint8)
    pcm = np.full(1024, FILL, np.uint8)
    one, zero = np.array([1], np.uint32), np.array([0], np.uint64)
    with dev._resident(stream, pcm, 288 + 16, 64) as (ds, dp, dst, db):
        dev.times()
        bad_calls = [
            lambda: dev.decode_batch(ds, zero[:0], one[:0], 0, dp, zero[:0]),                  # n = 0
            lambda: dev.decode_batch(ds, zero, one, 2, dp, zero),                              # no such framing
            lambda: dev.decode_batch(ds, zero, one, -1, dp, zero),
            lambda: dev.decode_batch(ds, zero, one, 0, dp + 8, zero),                          # d_pcm not 16-byte aligned
            lambda: dev.decode_batch(ds, zero, one, 0, dp, np.array([8], np.uint64)),          # pcm_offsets[0] neither
            lambda: dev.decode_batch(ds, zero, np.array([(1 << 24) + 1], np.uint32), 0, dp, zero),
            lambda: dev.decode_batch(ds, zero, one, 0, dp, zero, dst + 8),                     # d_state not 16-byte aligned
            lambda: dev.decode_batch(ds, zero, one, 0, dp, zero, None, db + 2),                # d_bad not 4-byte aligned
            lambda: dev.decode_batch(None, zero, one, 0, dp, zero),
            lambda: dev.decode_batch(ds, zero, one, 0, None, zero),
            lambda: dev.state_reset(dst + 8, 1),
            lambda: dev.state_reset(dst, 0),
        ]
        for k, call in enumerate(bad_calls):
            with pytest.raises(gsm.MiGsmError) as e:
                call()
            assert e.value.code == gsm.ERR_ARG, k
        too_many = (1 << 20) + 1
        with pytest.raises(gsm.MiGsmError):
            dev.decode_batch(ds, np.zeros(too_many, np.uint64), np.zeros(too_many, np.uint32), 0, dp, np.zeros(too_many, np.uint64))
        dev.sync()
        assert dev.times()[1] == 0
        assert np.array_equal(dev.d2h(dp, pcm.nbytes), pcm)
        # and the instance still works
        dev.decode_batch(ds, zero, one, 0, dp, zero)
        dev.sync()
        assert dev.times()[1] == 1
        assert np.array_equal(dev.d2h(dp, 320).view(np.int16), statement(s, 0)[0])


def test_state_reset_writes_fresh_states_and_nothing_else(dev):
    n = 67
    buf = np.full(2 * GUARD + 288 * n, FILL, np.uint8)
    with dev._resident(buf) as (d,):
        dev.state_reset(d + GUARD, n)
        dev.sync()
        got = dev.d2h(d, buf.nbytes)
    want = buf.copy()
    want[GUARD:GUARD + 288 * n] = np.tile(G.State().words().view(np.uint8), n)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("fmt", (0, 1))
def test_decode_stream_drops_a_tail_and_carries_a_state(dev, fmt):
    size = G.unit_bytes(fmt)
    data = pool(fmt, 1, 3, 80 + fmt)[0]
    want, words, _ = statement(data, fmt)
    for tail in (0, 1, 16, 32):
        dev.times()
        pcm, bad = dev.decode_stream(np.frombuffer(data + bytes(range(tail)), np.uint8), fmt)
        assert np.array_equal(pcm, want) and bad == 0 and dev.times()[1] == 1, tail
    state = G.State().words()
    a, _ = dev.decode_stream(np.frombuffer(data[:size] + b"\x01", np.uint8), fmt, state)
    b, _ = dev.decode_stream(np.frombuffer(data[size:], np.uint8), fmt, state)
    assert np.array_equal(np.concatenate([a, b]), want) and np.array_equal(state, words)
    pcm, bad = dev.decode_stream(np.frombuffer(data[:size - 1], np.uint8), fmt)  # no whole unit
    assert pcm.size == 0 and bad == 0
    if fmt == 0:
        pcm, bad = dev.decode_stream(np.frombuffer(b"\x30" + data[1:], np.uint8), 0)
        assert bad == 1 and not pcm[:160].any() and np.array_equal(pcm[160:], statement(data[33:], 0)[0])
