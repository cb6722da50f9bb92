"""The speculative walker's byte step keeps the macroblock phase — which block of the macroblock a byte belongs to and
how many DC + raw bytes that block's type has — in a table of six entries per lane in LDS (MIRTJ_SPEC_STEP,
csrc/rtj_spec_kernels.h): every step reads the next block's entry and takes it when the byte ends a block.  What can go
wrong there: an entry taken before it arrived (block ends on consecutive bytes: 0xFF one-byte blocks), the wrap from the
macroblock's last block to its first, the state carried from one 128-byte tile to the next, and lanes of one wave whose
packets have different tables.  Every case holds the block index and the planes to the oracle's, bit for bit, with a
walker per chunk and with runs of 2, 3 and 4 chunks (MI_RTJ_SPEC_RUN), behind the short lead (MI_RTJ_SPEC=1) and, for the
last test, behind the two longer ones (MI_RTJ_SPEC=3 / 4).

The exact kernels index whatever the proof refuses, so a wrong walker can hide behind them.  Where a case says "proven",
that is what pins the walker: the proof accepts a packet only if consecutive walkers met on the same byte in the same
phase.  For the packets built here it follows from how they are built (aligned_packet): a macroblock starts at every
byte 2048 c - 768, where the walker of chunk c — and of every run that begins with chunk c — starts on the assumption
that one does, so every walker is on the true chain from its first byte and none is walked again."""
import functools
import hashlib

import numpy as np
import pytest

import rtjlib as R
import test_gpu_parity as T
import test_gpu_spec_runs as RS
from pkg import P

pytestmark = pytest.mark.gpu

CHUNK, LEAD, TILE = 2048, 768, 128
SIZES = [(320, 240), (640, 368)]
RUNS = (1, 2, 3, 4)


@pytest.fixture(params=RUNS, ids=[f"S{s}" for s in RUNS])
def dev(request, monkeypatch):
    monkeypatch.setenv("MI_RTJ_SPEC", "1")
    monkeypatch.setenv("MI_RTJ_SPEC_RUN", str(request.param))
    d = P.MiRtj()
    yield d
    d.close()


@pytest.fixture(params=["3", "4"], ids=["lead1536", "lead6144"])
def dev_long(request, monkeypatch):
    monkeypatch.setenv("MI_RTJ_SPEC", request.param)
    d = P.MiRtj()
    yield d
    d.close()


def tables(Q):
    _, _, lb8, cb8, _, _ = R.oracle_tables(Q)
    return int(lb8), int(cb8)


@functools.lru_cache(maxsize=None)
def other_quality():
    """a quality whose luma and chroma blocks differ in raw bytes, and differ from Q = 255's"""
    for Q in range(254, 128, -1):
        lb8, cb8 = tables(Q)
        if lb8 != cb8 and (lb8, cb8) != tables(255):
            return Q
    raise AssertionError("no second quality with lb8 != cb8")


def coded_block(rng, n, bt8):
    """a block of exactly n bytes: DC, bt8 raw bytes, n - bt8 - 2 coefficients spelled out, one zero run to the end"""
    assert bt8 + 2 <= n <= 64
    spelled = n - bt8 - 2
    return bytes([int(rng.integers(0, 255))] + [int(x) for x in rng.integers(0, 256, bt8)] +
                 [int(x) & 0xFF for x in rng.integers(-64, 64, spelled)] + [63 + (63 - bt8 - spelled)])


def macroblock(rng, total, lb8, cb8):
    """six coded blocks of `total` bytes together"""
    low = [lb8 + 2] * 4 + [cb8 + 2] * 2
    n = list(low)
    extra = total - sum(low)
    assert 0 <= extra <= 6 * 64 - sum(low)
    while extra > 0:
        k = int(rng.integers(0, 6))
        d = min(extra, 64 - n[k], int(rng.integers(1, 33)))
        n[k] += d
        extra -= d
    return b"".join(coded_block(rng, n[k], lb8 if k < 4 else cb8) for k in range(6))


def aligned_packet(w, h, Q, seed, ff_runs):
    """Coded blocks of every length, with a macroblock starting at every byte 2048 c - 768.  ff_runs: now and then at
    least 13 consecutive unchanged blocks (0xFF, one byte each) that begin at any block of a macroblock — so they cross
    two wraps of the macroblock — and reach over a multiple of 128 bytes, a tile boundary of every walker that parses
    them.  Returns the packet and the number of such runs."""
    rng = np.random.default_rng(seed)
    lb8, cb8 = tables(Q)
    low = 4 * (lb8 + 2) + 2 * (cb8 + 2)
    nblk = (w // 16) * (h // 16) * 6
    body = bytearray()
    b, c, runs = 0, 1, 0
    while b < nblk:
        assert b % 6 == 0
        if len(body) == CHUNK * c - LEAD:
            c += 1
        D = CHUNK * c - LEAD - len(body)
        assert D >= low
        if D <= 384:
            body += macroblock(rng, D, lb8, cb8)  # ends on the walker's first byte
        elif D <= 2 * 384 + low:
            body += macroblock(rng, int(rng.integers(low, min(384, D - low) + 1)), lb8, cb8)
        elif ff_runs and D > 3 * 384 + 160 and nblk - b > 200 and rng.random() < 0.15:
            k = int(rng.integers(0, 6))  # the run begins with block k of this macroblock
            for j in range(k):
                body += coded_block(rng, int(rng.integers((lb8 if j < 4 else cb8) + 2, 65)), lb8 if j < 4 else cb8)
            L = int(rng.integers(13, 20))
            while len(body) // TILE == (len(body) + L - 1) // TILE:
                L += 1
            body += b"\xff" * L
            runs += 1
            b += k + L
            while b % 6:  # the rest of the macroblock the run ends in
                bt8 = lb8 if b % 6 < 4 else cb8
                body += coded_block(rng, int(rng.integers(bt8 + 2, 65)), bt8)
                b += 1
            continue
        else:
            body += macroblock(rng, int(rng.integers(low, 385)), lb8, cb8)
        b += 6
    return np.frombuffer(bytes(RS.header(w, h, Q, len(body))) + bytes(body), dtype=np.uint8).copy(), runs


@functools.lru_cache(maxsize=None)
def built(w, h, Q, ff_runs):
    pkt, runs = aligned_packet(w, h, Q, seed=w + Q, ff_runs=ff_runs)
    assert not ff_runs or runs >= 3, runs
    assert pkt.size - 12 > 4 * CHUNK  # runs of four chunks, and more than one of them
    return pkt


_wanted = {}


def wanted(pkt, prefill):
    """the oracle's planes and index of a packet, computed once for all cases and run lengths"""
    key = (hashlib.sha1(pkt.tobytes()).digest(), prefill)
    if key not in _wanted:
        want, idx = RS.wanted(pkt, prefill)
        want.setflags(write=False)
        idx.setflags(write=False)
        _wanted[key] = (want, idx)
    return _wanted[key]


def decode_and_check(dev, pkts, prefill=0x3C):
    """one plan over the packets; index and planes against the oracle's; returns (proven, repaired)"""
    d_stream, po, pl, hdrs = dev.upload_packets(pkts, align=1)
    sizes = [T.frame_bytes(*T.packet_size(p)) for p in pkts]
    oo = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    d_out = dev.alloc(int(oo[-1]))
    dev.memset(d_out, prefill, int(oo[-1]))
    plan = dev.plan(hdrs, po, pl, oo[:-1].copy())
    plan.decode(d_stream, d_out)
    dev.sync()
    idx = plan.read_index()
    proven, _ = plan.spec_stats()
    repaired = plan.repaired
    whole = dev.d2h(d_out, int(oo[-1]))
    plan.close()
    dev.free(d_stream)
    dev.free(d_out)
    k = 0
    for i, p in enumerate(pkts):
        want, want_idx = wanted(p, prefill)
        got_idx = idx[k:k + want_idx.size].astype(np.int64)
        k += want_idx.size
        bad = np.nonzero(got_idx != want_idx)[0]
        assert bad.size == 0, f"packet {i} ({p.size - 12} bytes): index differs from block {bad[0]} on: got {got_idx[bad[0]]} want {want_idx[bad[0]]}"
        assert T.first_diff(whole[int(oo[i]):int(oo[i + 1])], want) is None, (i, p.size - 12)
    return proven, repaired


def encoder_made(Q, n=2):
    return [RS.encoded(w, h, Q, 8, i) for w, h in SIZES for i in range(n)]


def test_encoder_made_content_with_two_block_types_is_proven_without_repairs(dev):
    assert tables(255)[0] != tables(255)[1]
    pkts = encoder_made(255)
    proven, repaired = decode_and_check(dev, pkts)
    print(f"proven {proven} of {len(pkts)}, repaired {repaired}")
    assert proven == len(pkts) and repaired == 0, (proven, repaired)


def test_runs_of_one_byte_blocks_across_macroblock_wraps_and_tile_boundaries(dev):
    """block ends on 13 and more consecutive bytes: the entry read in one step is taken in that step and the one read in
    the next step must be the one after it; proven without repairs (module docstring), also without the runs"""
    pkts = [built(w, h, 255, ff) for w, h in SIZES for ff in (True, False)]
    proven, repaired = decode_and_check(dev, pkts)
    print(f"proven {proven} of {len(pkts)}, repaired {repaired}")
    assert proven == len(pkts) and repaired == 0, (proven, repaired)


def test_packets_of_nothing_but_one_byte_blocks(dev):
    """every byte ends a block.  320x240 is 1800 bytes, one chunk, walked from byte 0: proven.  640x368 is three chunks
    whose walkers start at bytes that are no multiple of 6 and keep the phase they assumed: refused by design, and the
    index is the exact kernels'."""
    pkts = [RS.unchanged(w, h, 255) for w, h in SIZES]
    assert pkts[0].size - 12 < CHUNK < pkts[1].size - 12 and (CHUNK - LEAD) % 6 != 0
    proven, _ = decode_and_check(dev, pkts)
    assert proven >= 1, proven
    proven, repaired = decode_and_check(dev, pkts[:1])
    assert proven == 1 and repaired == 0, (proven, repaired)


def test_lanes_of_one_wave_hold_packets_of_two_qualities(dev):
    """packets alternate between two qualities with different (lb8, cb8): a 320x240 packet is a few dozen chunks, so
    every wave of 64 walkers has lanes of both, each with its own table"""
    Q2 = other_quality()
    w, h = SIZES[0]
    pkts = [RS.encoded(w, h, Q2 if i & 1 else 255, 8, i // 2) for i in range(8)]
    pkts += [built(w, h, 255, True), built(w, h, Q2, True), RS.encoded(SIZES[1][0], SIZES[1][1], Q2, 8, 0), built(SIZES[1][0], SIZES[1][1], 255, True)]
    assert max((p.size - 12) // CHUNK + 1 for p in pkts[:10]) < 64
    proven, repaired = decode_and_check(dev, pkts)
    print(f"Q = 255 {tables(255)}, Q = {Q2} {tables(Q2)}: proven {proven} of {len(pkts)}, repaired {repaired}")
    assert proven == len(pkts) and repaired == 0, (proven, repaired)


def test_one_block_type_runs_the_step_without_a_phase(dev):
    """lb8 == cb8: the 10-instruction step, no table; results as before"""
    assert tables(128)[0] == tables(128)[1]
    pkts = encoder_made(128) + [built(w, h, 128, True) for w, h in SIZES]
    proven, repaired = decode_and_check(dev, pkts)
    print(f"proven {proven} of {len(pkts)}, repaired {repaired}")
    assert proven == len(pkts) and repaired == 0, (proven, repaired)


def test_the_longer_leads_use_the_table_too(dev_long):
    """a walker per chunk behind 1,536 and 6,144 bytes of lead.  Encoder-made content is proven; the built packets'
    walkers do not start on macroblocks here, so only their index and planes are held (what the proof refuses, the
    exact kernels index)."""
    pkts = encoder_made(255, n=1)
    proven, repaired = decode_and_check(dev_long, pkts)
    assert proven == len(pkts) and repaired == 0, (proven, repaired)
    decode_and_check(dev_long, [built(w, h, 255, True) for w, h in SIZES] + [RS.unchanged(w, h, 255) for w, h in SIZES] +
                     [RS.encoded(SIZES[0][0], SIZES[0][1], other_quality(), 8, 0)])
