"""libmi_pcm.so on the device against the statement (tests/pcmraw.py), byte for byte: samples and counts.

Packets lie at chosen byte phases of a 16-byte word in one buffer, sample slots at multiples of 16 that are mostly none of
256, with GUARD bytes of 0xA5 around and between everything, the counts included.  Every buffer is compared whole with what
it must hold afterwards, so every byte outside the named outputs is checked, and the packets must come back as they were.

T is the tile, MI_PCM_TILE_BYTES of output: a workgroup's work.  A lane makes 16-byte pieces, a packet's last piece goes
another way, and a tile is found by a search over the call's packets; so the shapes are, for every codec and 1, 2, 3 and 6
channels (which give F * ch mod 4 = 0, 1, 2, 3 for the LPCM group tails): lengths of 0, under a frame, one frame, one
group and one group +- 1 byte at all 16 phases, and what makes T - one group, T and T + one group of output and two tiles
and a tail, at phases in turn, all in one call, empty packets among them."""
import hashlib
import importlib
import json
import os

import numpy as np
import pytest

import pcmraw as R
from pkg import ROOT

pytestmark = pytest.mark.gpu

GUARD, FILL = 256, 0xA5
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "pcm_vectors.json")))
pcm = importlib.import_module("gmerlin-avdecoder_amd.pcm")
T = pcm.TILE_BYTES
CHANNELS = (1, 2, 3, 6)


@pytest.fixture(scope="module")
def dev():
    d = pcm.MiPcm(0)
    yield d
    d.close()


_seen = {}


def statement(c, ch, data):
    """(output bytes, count) of the statement's numpy form, computed once for the same packet"""
    key = (c, ch, bytes(data))
    if key not in _seen:
        _seen[key] = R.decode(c, ch, data)
    return _seen[key]


def channels_of(c):
    return (1,) if c in R.MONO else CHANNELS


def bytes_for(c, ch, frames):
    """the shortest packet of that many sample frames"""
    a = R.GROUPS[c][0]
    if R.CODECS[c].startswith("LPCM20"):
        return -(-5 * frames * ch // 2)
    if R.CODECS[c].startswith("LPCM24"):
        return 3 * frames * ch
    return frames * ch * a


def length_for(c, ch, out_bytes):
    """the shortest packet whose samples are at least out_bytes"""
    return bytes_for(c, ch, -(-out_bytes // (ch * R.sample_bytes(c))))


class Run:
    """one call over the given packets: lays out the three buffers, calls, reads them back whole"""

    def __init__(self, dev, c, ch, packets, phases=None, with_outside=True):
        n = len(packets)
        self.c, self.ch, self.packets, self.n = c, ch, packets, n
        at, offs = GUARD, []
        for i, p in enumerate(packets):
            phase = (5 * i + 1) % 16 if phases is None else phases[i]
            at += (phase - at) % 16
            offs.append(at)
            at += len(p) + GUARD
        buf = np.full(at, FILL, np.uint8)
        for o, p in zip(offs, packets):
            buf[o:o + len(p)] = np.frombuffer(p, np.uint8)
        self.sizes = [R.layout(c, ch, len(p))[3] for p in packets]
        at, slots = 0, []
        for i, s in enumerate(self.sizes):
            at = (at + GUARD + 255) // 256 * 256 + (16 * (1 + i % 15) if i % 4 else 0)
            slots.append(at)
            at += s
        out = np.full(at + GUARD, FILL, np.uint8)
        counts = np.full(2 * GUARD + 4 * n, FILL, np.uint8)
        self.offs, self.slots, self.buf = np.array(offs, np.uint64), np.array(slots, np.uint64), buf
        self.before = (out.copy(), counts.copy())
        self.lens = np.array([len(p) for p in packets], np.uint32)
        with dev._resident(buf, out, counts) as (dp, do, dc):
            dev.times()
            dev.decode_batch(c, ch, dp, self.offs, self.lens, do, self.slots, dc + GUARD if with_outside else None)
            dev.sync()
            self.launches = dev.times()[1]
            self.buf_after = dev.d2h(dp, buf.nbytes)
            self.out, self.counts = dev.d2h(do, out.nbytes), dev.d2h(dc, counts.nbytes)
        self.with_outside = with_outside

    def slot(self, i):
        o = int(self.slots[i])
        return self.out[o:o + self.sizes[i]]

    def count(self, i):
        return int(self.counts[GUARD + 4 * i:GUARD + 4 * i + 4].view(np.uint32)[0])

    def check(self):
        out, counts = (x.copy() for x in self.before)
        for i, p in enumerate(self.packets):
            want, k = statement(self.c, self.ch, p)
            o = int(self.slots[i])
            out[o:o + want.size] = want
            if self.with_outside:
                counts[GUARD + 4 * i:GUARD + 4 * i + 4] = np.array([k], np.uint32).view(np.uint8)
        assert self.launches == (1 if any(self.sizes) else 0) + (1 if self.with_outside else 0)
        assert np.array_equal(self.buf_after, self.buf), "a packet was written"
        for name, got, want in (("samples", self.out, out), ("counts", self.counts, counts)):
            if not np.array_equal(got, want):
                d = np.flatnonzero(got != want)
                raise AssertionError(f"{R.CODECS[self.c]} x{self.ch} {name}: {d.size} bytes differ from the statement's, the first at byte "
                                     f"{int(d[0])} of the buffer: {int(got[d[0]]):#x}, not {int(want[d[0]]):#x}")


def shapes(c, ch, seed):
    """(packets, phases) of the module docstring for one codec and channel count"""
    a, b, g = R.GROUPS[c]
    frame = length_for(c, ch, 1)
    short = sorted({0, frame - 1, frame, a * g - 1, a * g, a * g + 1, 2 * frame + 1})
    packets, phases = [], []
    for n in short:
        for phase in range(16):
            packets.append(R.content(c, n, seed + 31 * n + phase))
            phases.append(phase)
    per_tile = T // (ch * R.sample_bytes(c))  # whole frames in a tile: T - one group (or one frame), T, and just past it
    big = [length_for(c, ch, T - b), bytes_for(c, ch, per_tile - 1), bytes_for(c, ch, per_tile), bytes_for(c, ch, per_tile) + 1,
           bytes_for(c, ch, per_tile + 1), length_for(c, ch, T + b), length_for(c, ch, 2 * T + 5 * b) + a * g - 1]
    for i, n in enumerate(big):
        for k in range(3):
            packets.append(R.content(c, n, seed + 7919 * i + k))
            phases.append((5 * i + 6 * k + 3) % 16)
    return packets, phases


@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("name", R.CODECS)
def test_decode_batch_against_the_statement(dev, name, ch):
    c = R.codec(name)
    if ch not in channels_of(c):
        with pytest.raises(pcm.MiPcmError) as e:  # the mono forms take one channel
            Run(dev, c, ch, [bytes(10)])
        assert e.value.code == pcm.ERR_ARG
        return
    packets, phases = shapes(c, ch, 100 * c + ch)
    sizes = {R.layout(c, ch, len(p))[3] for p in packets}
    assert any(T - 64 <= s <= T for s in sizes) and any(T < s <= T + 64 for s in sizes) and any(s > 2 * T for s in sizes)
    if c in R.LPCM and c not in R.MONO:  # every group tail: F * ch mod 4
        assert {R.layout(c, k, len(p))[0] * k % 4 for k in CHANNELS for p in shapes(c, k, 0)[0]} == {0, 1, 2, 3}
    Run(dev, c, ch, packets, phases).check()


@pytest.mark.parametrize("with_outside", (True, False))
@pytest.mark.parametrize("name", R.CODECS)
def test_65_packets_of_mixed_lengths_with_and_without_counts(dev, name, with_outside):
    c = R.codec(name)
    ch = 1 if c in R.MONO else 2
    a, b, g = R.GROUPS[c]
    rng = np.random.default_rng(200 + c)
    lens = [(0, 1, a * g, 37, 1000, 0, length_for(c, ch, T) + 3, 4097, a * ch, 12345)[i % 10] for i in range(65)]
    # noise: for the float codecs most samples are outside the domain, so the counts are not 0
    packets = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lens]
    r = Run(dev, c, ch, packets, with_outside=with_outside)
    r.check()
    if with_outside:
        assert (c in R.FLOATS) == any(r.count(i) for i in range(65))


def test_a_call_of_empty_packets_launches_only_the_counts(dev):
    c = R.codec("F32LE")
    r = Run(dev, c, 2, [b"", bytes(7), b""])
    r.check()
    assert r.launches == 1 and [r.count(i) for i in range(3)] == [0, 0, 0]
    r = Run(dev, c, 2, [b"", bytes(7), b""], with_outside=False)
    r.check()
    assert r.launches == 0


@pytest.mark.parametrize("name", [R.CODECS[c] for c in R.FLOATS])
def test_every_exponent_field_with_counts_and_nan_payloads(dev, name):
    c = R.codec(name)
    a = R.GROUPS[c][0]
    fields = list(range(256)) if a == 4 else [0, 1, 992, 993, 1023, 1053, 1054, 2046, 2047]
    lo, hi = (97, 157) if a == 4 else (993, 1053)
    packets = [R.float_edges(c, [e]) for e in fields]  # three mantissas, both signs: six samples a packet
    packets.append(R.float_edges(c, fields))            # and all of them in one packet
    r = Run(dev, c, 1, packets)
    r.check()
    for i, e in enumerate(fields):
        want, count = R.expected(c, 1, packets[i])  # the loop form, sample by sample
        assert np.array_equal(r.slot(i), want) and r.count(i) == count
        inside = lo <= e <= hi
        # six samples: a float's exponent field 0 is zeros and denormals, all defined; a double's is two zeros and four outside
        assert count == (0 if inside else 6 if e else 0 if a == 4 else 4)
        if e == max(fields):  # infinities and NaNs: the payload is there, byte for byte
            ieee = np.frombuffer(packets[i], np.uint8).reshape(-1, a)
            assert np.array_equal(r.slot(i).reshape(-1, a), ieee[:, ::-1] if name.endswith("BE") else ieee)
    assert r.count(len(fields)) == sum(r.count(i) for i in range(len(fields)))
    two = Run(dev, c, 2, packets, with_outside=False)
    two.check()


def marked(c, ch, got, nbytes):
    """the kernel's samples with upstream's pattern put where upstream writes nothing (they must be zeros)"""
    _, written, _, out_bytes = R.layout(c, ch, nbytes)
    got = got.copy()
    tail = got[written * R.sample_bytes(c):out_bytes]
    assert not tail.any()
    tail[:] = R.PATTERN
    return got.tobytes()


@pytest.mark.parametrize("name", R.CODECS)
def test_every_recorded_vector_directly(dev, name):
    c = R.codec(name)
    for ch in channels_of(c):
        vs = [v for v in GOLDEN["vectors"] if v[0] == name and v[1] == ch]
        packets = [bytes.fromhex(v[2]) if isinstance(v[2], str) else R.content(c, v[2][1], v[2][0]) for v in vs]
        r = Run(dev, c, ch, packets)
        r.check()
        for i, v in enumerate(vs):
            got = marked(c, ch, r.slot(i), len(packets[i]))
            assert (hashlib.sha256(got).hexdigest() == v[5][1]) if isinstance(v[5], list) else (got.hex() == v[5]), v[:2]
            assert r.count(i) == 0 and r.sizes[i] == sum(v[3]) * ch * R.sample_bytes(c)


@pytest.mark.parametrize("name", ("SWAP16", "S24LE", "LPCM24", "LPCM20", "LPCM20_MONO", "F32BE", "F64LE", "ALAW"))
def test_decode_packet_equals_decode_batch(dev, name):
    c = R.codec(name)
    ch = 1 if c in R.MONO else 3
    for n in (0, 1, 29, length_for(c, ch, T) + 7):
        data = np.random.default_rng(300 + n).integers(0, 256, n, dtype=np.uint8)
        dev.times()
        out, count = dev.decode_packet(c, ch, data)
        want, k = statement(c, ch, data.tobytes())
        assert np.array_equal(out, want) and count == k
        assert dev.times()[1] == 1 + (1 if want.size else 0)
    r = Run(dev, c, ch, [data.tobytes()])
    assert np.array_equal(r.slot(0), out) and r.count(0) == count


def test_the_refusals_launch_nothing(dev):
    c = R.codec("S24BE")
    data = np.arange(60, dtype=np.uint8)
    out = np.full(1024, FILL, np.uint8)
    lens, zero = np.array([60], np.uint32), np.array([0], np.uint64)
    with dev._resident(data, out, 64) as (dp, do, dc):
        dev.times()
        bad_calls = [
            lambda: dev.decode_batch(c, 2, dp, zero[:0], lens[:0], do, zero[:0]),                     # n = 0
            lambda: dev.decode_batch(-1, 2, dp, zero, lens, do, zero),                               # no such codec
            lambda: dev.decode_batch(len(R.CODECS), 2, dp, zero, lens, do, zero),
            lambda: dev.decode_batch(c, 0, dp, zero, lens, do, zero),                                # channels
            lambda: dev.decode_batch(c, pcm.MAX_CHANNELS + 1, dp, zero, lens, do, zero),
            lambda: dev.decode_batch(R.codec("LPCM24_MONO"), 2, dp, zero, lens, do, zero),           # a mono codec
            lambda: dev.decode_batch(R.codec("LPCM20_MONO"), 6, dp, zero, lens, do, zero),
            lambda: dev.decode_batch(c, 2, dp, zero, lens, do + 8, zero),                            # d_samples not 16-byte aligned
            lambda: dev.decode_batch(c, 2, dp, zero, lens, do, np.array([8], np.uint64)),            # sample_offsets[0] neither
            lambda: dev.decode_batch(c, 2, dp, zero, np.array([1 << 31], np.uint32), do, zero),      # a length of 2^31
            lambda: dev.decode_batch(c, 2, dp, zero, lens, do, zero, dc + 2),                        # d_outside not 4-byte aligned
            lambda: dev.decode_batch(c, 2, None, zero, lens, do, zero),
            lambda: dev.decode_batch(c, 2, dp, zero, lens, None, zero),
            lambda: dev.decode_packet(c, 0, data),
            lambda: dev.decode_packet(R.codec("LPCM24_MONO"), 2, data),
        ]
        for k, call in enumerate(bad_calls):
            with pytest.raises(pcm.MiPcmError) as e:
                call()
            assert e.value.code == pcm.ERR_ARG, k
        too_many = (1 << 20) + 1
        with pytest.raises(pcm.MiPcmError):
            dev.decode_batch(c, 2, dp, np.zeros(too_many, np.uint64), np.zeros(too_many, np.uint32), do, np.zeros(too_many, np.uint64))
        # more tiles than a launch has workgroups: 2^20 packets that would each give 2^32 - 2 bytes of A-law samples
        many = 1 << 20
        with pytest.raises(pcm.MiPcmError):
            dev.decode_batch(R.codec("ALAW"), 1, dp, np.zeros(many, np.uint64), np.full(many, (1 << 31) - 1, np.uint32), do, np.zeros(many, np.uint64))
        dev.sync()
        assert dev.times()[1] == 0
        assert np.array_equal(dev.d2h(do, out.nbytes), out)
        # and the instance still works
        dev.decode_batch(c, 2, dp, zero, lens, do, zero)
        dev.sync()
        assert dev.times()[1] == 1
        assert np.array_equal(dev.d2h(do, 80), statement(c, 2, data.tobytes())[0])
