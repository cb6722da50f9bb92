"""Runs of chunks in the speculative index (csrc/rtj_spec_kernels.h): one walker lane walks up to S consecutive
2048-byte chunks of a packet behind ONE lead and leaves, at every chunk boundary inside its run, the hand-over pair a
walker per chunk leaves at its chunk's start and end.  MI_RTJ_SPEC_RUN forces S (1 = a walker per chunk, as before);
MI_RTJ_SPEC=1 forces the speculation with the short lead and no policy.  Every case runs at S = 1, 2, 3, 4 and holds the
block-offset index and the planes to the oracle's.

Packet lengths are made by zero bytes behind the last block (the oracle stops at the last macroblock; the walkers parse
them on as blocks of 64 bytes, which the index clips) and by pictures of nothing but unchanged blocks, which are one
0xFF byte each, so that a packet's length in bytes is its number of blocks."""
import functools

import numpy as np
import pytest

import rtjlib as R
import test_gpu_parity as T
from pkg import P

pytestmark = pytest.mark.gpu

CHUNK = 2048
RUNS = (1, 2, 3, 4)
GEOMETRIES = [(320, 240, 255), (320, 240, 128), (640, 368, 255), (640, 368, 128)]  # Q = 128: lb8 == cb8


@pytest.fixture(params=RUNS, ids=[f"S{s}" for s in RUNS])
def S(request, monkeypatch):
    monkeypatch.setenv("MI_RTJ_SPEC", "1")
    monkeypatch.setenv("MI_RTJ_SPEC_RUN", str(request.param))
    return request.param


@pytest.fixture
def dev(S):
    d = P.MiRtj()
    yield d
    d.close()


def header(w, h, Q, n):
    t = 12 + n
    return np.array([t & 255, (t >> 8) & 255, (t >> 16) & 255, (t >> 24) & 255, 12, 0, w & 255, w >> 8, h & 255, h >> 8, Q, 0], np.uint8)


def padded(pkt, n):
    """the packet with n stream bytes: zeros behind its last block, the length in the header put right"""
    assert n >= pkt.size - 12
    p = np.concatenate([pkt, np.zeros(12 + n - pkt.size, np.uint8)])
    p[0:4] = header(0, 0, 0, n)[0:4]
    return p


def unchanged(w, h, Q):
    """every block unchanged: one 0xFF byte per block, the last block ends with the packet"""
    n = (w // 16) * (h // 16) * 6
    return np.concatenate([header(w, h, Q, n), np.full(n, 255, np.uint8)])


@functools.lru_cache(maxsize=None)
def encoded(w, h, Q, amp=8, i=0):
    return R.OracleEncoder(w, h, Q).encode(R.synth_frame(w, h, i, seed=7, amp=amp))


def length_cases(w, h, Q, S):
    """(name, packet): the lengths at which a run list can go wrong, for runs of S chunks"""
    base = encoded(w, h, Q)
    n = base.size - 12
    unit = S * CHUNK
    up = (n + unit - 1) // unit * unit  # whole runs
    return [("as encoded", base),
            ("a whole number of runs", padded(base, up)),            # the end position has a chunk, and a run, of its own
            ("whole runs + 1 byte", padded(base, up + 1)),
            ("last run a single chunk", padded(base, up + 1000)),    # chunks = up / 2048 + 1
            ("one chunk short of whole runs", padded(base, up - 1) if up - 1 >= n else base),
            ("shorter than a chunk", unchanged(320, 240, Q))]        # 1800 blocks, 1800 bytes


def wanted(pkt, prefill):
    w, h = T.packet_size(pkt)
    want = np.full(T.frame_bytes(w, h), prefill, np.uint8)
    dec = R.OracleDecoder()
    dec.decode(pkt, want)
    return want, dec.block_offsets(pkt).astype(np.int64) - 12


def decode_and_check(dev, pkts, prefill=0x3C):
    """one plan over the packets; index and planes against the oracle's; returns (proven, chunks, repaired)"""
    d_stream, po, pl, hdrs = dev.upload_packets(pkts, align=1)
    sizes = [T.frame_bytes(*T.packet_size(p)) for p in pkts]
    oo = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    d_out = dev.alloc(int(oo[-1]))
    dev.memset(d_out, prefill, int(oo[-1]))
    plan = dev.plan(hdrs, po, pl, oo[:-1].copy())
    plan.decode(d_stream, d_out)
    dev.sync()
    idx = plan.read_index()
    proven, chunks = plan.spec_stats()
    repaired = plan.repaired
    whole = dev.d2h(d_out, int(oo[-1]))
    plan.close()
    dev.free(d_stream)
    dev.free(d_out)
    assert chunks == sum((p.size - 12) // CHUNK + 1 for p in pkts), "stream_chunks counts 2048-byte chunks whatever S"
    k = 0
    for i, p in enumerate(pkts):
        want, want_idx = wanted(p, prefill)
        got_idx = idx[k:k + want_idx.size].astype(np.int64)
        k += want_idx.size
        bad = np.nonzero(got_idx != want_idx)[0]
        assert bad.size == 0, f"packet {i} ({p.size - 12} bytes): index differs from block {bad[0]} on: got {got_idx[bad[0]]} want {want_idx[bad[0]]}"
        assert T.first_diff(whole[int(oo[i]):int(oo[i + 1])], want) is None, (i, p.size - 12)
    return proven, chunks, repaired


@pytest.mark.parametrize("w,h,Q", GEOMETRIES)
def test_packet_lengths_around_the_run_boundaries(dev, S, w, h, Q):
    cases = length_cases(w, h, Q, S)
    pkts = [p for _, p in cases]
    assert (pkts[1].size - 12) % (S * CHUNK) == 0 and (pkts[2].size - 12) % (S * CHUNK) == 1
    assert ((pkts[3].size - 12) // CHUNK + 1) % S == 1 % S and pkts[5].size - 12 < CHUNK
    proven, _, repaired = decode_and_check(dev, pkts)
    print(f"S={S} {w}x{h} Q={Q}: proven {proven} of {len(pkts)}, repaired {repaired}")
    # encoder-made content with noise of +-8 is proven, and so is its padding (zeros parse as blocks of 64 bytes; walkers
    # that start inside them are out of step and are walked again); the short packet is one chunk, from byte 0
    assert proven == len(pkts), (proven, len(pkts))


def test_last_block_ends_on_a_run_boundary(dev, S):
    """1024x1024 has 24,576 blocks: a picture of unchanged blocks is 12 chunks, whole runs for every S, and its last
    block ends where the last run does; the end position is the first byte of a run of its own.  With it a packet that
    mixes coded and unchanged blocks (0xFF bytes inside ordinary runs)."""
    w, h, Q = 1024, 1024, 128
    still = unchanged(w, h, Q)
    assert (still.size - 12) % (4 * CHUNK) == 0 and (still.size - 12) % (3 * CHUNK) == 0
    enc = R.OracleEncoder(320, 240, 200, 6, 3, 3)
    mixed = [enc.encode(R.synth_frame(320, 240, n // 4, seed=9, amp=2)) for n in range(6)]
    assert any((p[12:] == 255).any() and not (p[12:] == 255).all() for p in mixed)
    # (no count of proven packets here: where luma and chroma blocks parse differently, walkers inside one-byte blocks keep
    # the phase they assumed and such packets go to the exact kernels, by design)
    decode_and_check(dev, [still, unchanged(w, h, 255)] + mixed)


def test_runs_of_different_length_share_a_wave(dev, S):
    """every length case of every geometry in ONE plan: a wave's 64 lanes hold runs of 1 .. S chunks of different packets"""
    pkts = []
    for w, h, Q in GEOMETRIES:
        pkts += [p for _, p in length_cases(w, h, Q, S)]
    pkts += [encoded(320, 240, 255, 8, i) for i in range(1, 4)]
    order = np.random.default_rng(S).permutation(len(pkts))
    decode_and_check(dev, [pkts[i] for i in order])


@functools.lru_cache(maxsize=None)
def noisy_packets():
    w, h = 640, 368
    return tuple(encoded(w, h, 255, 32, i) for i in range(6))


def proven_flags(dev, pkts):
    """which packets the speculative index proves, each in a plan of its own (the proof is per packet)"""
    return [decode_and_check(dev, [p])[0] for p in pkts]


@functools.lru_cache(maxsize=None)
def noisy_reference():
    """what a walker per chunk (S = 1) proves and refuses of the noisy packets, found once"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MI_RTJ_SPEC", "1")
        mp.setenv("MI_RTJ_SPEC_RUN", "1")
        d = P.MiRtj()
        try:
            return tuple(proven_flags(d, noisy_packets())), decode_and_check(d, list(noisy_packets()))
        finally:
            d.close()


def test_noisy_content_is_repaired_and_proven_as_with_a_walker_per_chunk(dev, S):
    """noise of +-32 at Q = 255: many walkers have not fallen into step behind the short lead and are walked again
    (k_spec_repair rewrites single chunks of a run; the run's other chunks keep the run walker's bits).  The same
    packets are proven or refused as at S = 1, and index and planes are the oracle's either way."""
    want_flags, (want_proven, _, want_repaired) = noisy_reference()
    pkts = list(noisy_packets())
    proven, _, repaired = decode_and_check(dev, pkts)
    flags = proven_flags(dev, pkts)
    print(f"S={S}: proven {proven} (S=1: {want_proven}), repaired {repaired} (S=1: {want_repaired}), per packet {flags} (S=1: {list(want_flags)})")
    assert want_repaired > 0, "the content does not force repairs"
    assert repaired > 0
    assert tuple(flags) == want_flags and proven == want_proven
