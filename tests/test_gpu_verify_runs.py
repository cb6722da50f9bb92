"""k_spec_verify's emission per run (csrc/rtj_spec_kernels.h, spec_ver_emit_runs): where a launch's walkers walked runs,
a wave of the first proof pass turns a whole run's start bits into block offsets at once — the bits read once from the
piece that holds the first chunk's hand-over point, one popcount scan, a window of 1,024 ranks — while the proof stays per
chunk and the second pass, behind repairs, emits per chunk.  The cases are those where an emission per run can go wrong
and one per chunk could not.  MI_RTJ_SPEC=1 forces the speculation (short lead, no policy), MI_RTJ_SPEC_RUN the run
length S = 2, 3, 4; index and planes are held to the oracle's, as tests/test_gpu_spec_runs.py does it.

Pass 2 emits a packet with repaired chunks again, chunk by chunk, so only packets proven WITHOUT a repair show what the
emission per run wrote.  Next to the content the cases are defined with, pictures of nothing but zero bytes stand in
where that content is repaired: a zero byte counts one unit whatever its place in a block, so every block is 64 bytes and
a macroblock 384, and a walker that starts on that grid is in step from its first byte."""
import functools

import numpy as np
import pytest

import rtjlib as R
import test_gpu_spec_runs as SR
from pkg import P

pytestmark = pytest.mark.gpu

CHUNK = SR.CHUNK
LEAD = 768
TILE = 512      # chunks of a packet k_spec_verify scans at a time
WINDOW = 1024   # ranks a wave orders at a time
RUNS = (2, 3, 4)


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


def chunks_of(pkt):
    return (pkt.size - 12) // CHUNK + 1


def runs_of(pkt, S):
    return (chunks_of(pkt) + S - 1) // S


def zeros(w, h, Q):
    """every block 64 zero bytes: blocks start every 64 bytes, macroblocks every 384"""
    n = (w // 16) * (h // 16) * 6 * 64
    return np.concatenate([SR.header(w, h, Q, n), np.zeros(n, np.uint8)])


def in_step_from_the_first_byte(S, Q):
    """all-zero content: every run walker starts on a unit start (r * S * 2048 - 768 on the 64- or 384-byte grid)"""
    unit = 64 if Q == 128 else 384
    return all((r * S * CHUNK - LEAD) % unit == 0 for r in range(1, 7))


@pytest.mark.parametrize("Q", [255, 128])  # 128: lb8 == cb8, the block is the unit
def test_more_than_one_window_per_run(dev, S, Q):
    """1280x720 of unchanged blocks: 21,600 one-byte blocks, every start bit set, every dword of every lane full, a run of
    S chunks holds S * 2048 ranks: 4 to 8 windows.  Twice in one plan: the second packet's first run is not the first
    wave's of its workgroup's eight."""
    still = SR.unchanged(1280, 720, Q)
    assert still.size - 12 == 21600 and chunks_of(still) == 11
    assert 4 * WINDOW <= S * CHUNK <= 8 * WINDOW
    assert runs_of(still, S) % 8 != 0
    proven, _, repaired = SR.decode_and_check(dev, [still, still])
    print(f"S={S} Q={Q}: proven {proven} of 2, repaired {repaired}")
    # Q = 128: a walker that takes its first byte for a block start is right.  S = 3: 6144 r - 768 bytes are whole
    # macroblocks of six one-byte blocks, the phase is right as well.  Nothing to repair: pass 1 emitted the index.
    if Q == 128 or S == 3:
        assert (proven, repaired) == (2, 0)


@functools.lru_cache(maxsize=None)
def noisy_1080():
    return R.OracleEncoder(1920, 1088, 255).encode(R.synth_frame(1920, 1088, 0, seed=7, amp=64))


def test_tile_boundary_inside_a_run_noisy_1080p(dev, S):
    """one packet of more than 512 chunks: 1080p at Q = 255 with noise of +-64"""
    pkt = noisy_1080()
    assert chunks_of(pkt) > TILE
    if S == 3:  # runs start at chunks 0, 3, 6, ... (the first from byte 0): chunks 511 and 512 are of one run
        assert TILE % S != 0 and (TILE - 1) // S == TILE // S
    proven, chunks, repaired = SR.decode_and_check(dev, [pkt])
    print(f"S={S}: {chunks} chunks, proven {proven}, repaired {repaired}")


@pytest.mark.parametrize("Q", [255, 128])
def test_tile_boundary_inside_a_run_proven_in_pass_one(dev, S, Q):
    """1280x720 of zero blocks: 675 chunks.  Where the walkers start on the unit grid nothing is repaired and the index
    is what the emission per run wrote, across the tile boundary."""
    pkt = zeros(1280, 720, Q)
    assert chunks_of(pkt) == 676 and chunks_of(pkt) > TILE + 4 * S
    proven, _, repaired = SR.decode_and_check(dev, [pkt, pkt])
    print(f"S={S} Q={Q}: proven {proven} of 2, repaired {repaired}")
    if in_step_from_the_first_byte(S, Q):
        assert (proven, repaired) == (2, 0)


def last_run_cases(w, h, Q, S):
    base = SR.encoded(w, h, Q)
    n = base.size - 12
    unit = S * CHUNK
    k = (n + unit - 1) // unit
    return [SR.padded(base, unit * k + d) for d in (0, 1, 2047, 2048, 2049, 2 * CHUNK + 1, 3 * CHUNK + 1)]


@pytest.mark.parametrize("Q", [255, 128])
def test_last_run_of_every_length(dev, S, Q):
    """packets of S * 2048 * k + {0, 1, 2047, 2048, 2049} bytes (and + 4097, + 6145, for the last runs of three and four
    chunks) in one plan: runs of different packets are neighbours in the bit buffer"""
    pkts = []
    for w, h in ((320, 240), (640, 368)):
        pkts += last_run_cases(w, h, Q, S)
    last = sorted({chunks_of(p) % S for p in pkts})
    assert last == list(range(S))  # chunks of the last run (0: a whole one): every length
    proven, _, repaired = SR.decode_and_check(dev, pkts)
    print(f"S={S} Q={Q}: proven {proven} of {len(pkts)}, repaired {repaired}")
    assert proven == len(pkts)


@pytest.mark.parametrize("Q", [255, 128])
def test_last_run_of_every_length_proven_in_pass_one(dev, S, Q):
    """the padded packets above are proven behind repairs (their zeros put walkers out of step), so pass 2 wrote their
    index.  Pictures of zero blocks, 64 wide and 8 .. 16 macroblock rows high, are 7 .. 13 chunks of blocks to their last
    byte: last runs of every length that the emission per run alone numbers."""
    pkts = [zeros(64, 16 * rows, Q) for rows in range(8, 17)]
    assert sorted({chunks_of(p) for p in pkts}) == list(range(7, 14))
    assert sorted({chunks_of(p) % S for p in pkts}) == list(range(S))
    proven, _, repaired = SR.decode_and_check(dev, pkts)
    print(f"S={S} Q={Q}: proven {proven} of {len(pkts)}, repaired {repaired}")
    if in_step_from_the_first_byte(S, Q):
        assert (proven, repaired) == (len(pkts), 0)


def test_hand_over_point_at_its_farthest(dev, S):
    """zeros parse as 64-byte blocks, so a macroblock start can lie up to 384 bytes before a run's first chunk: an
    encoded 640x368 packet with 3 * S * 2048 zero bytes behind it, and a 640x368 picture of zero blocks, whose macroblocks
    start exactly at every third chunk (the hand-over point is then the start before, 384 bytes back)."""
    base = SR.encoded(640, 368, 255)
    pkts = [SR.padded(base, base.size - 12 + 3 * S * CHUNK), zeros(640, 368, 255), zeros(640, 368, 128)]
    assert (3 * CHUNK) % 384 == 0
    proven, _, repaired = SR.decode_and_check(dev, pkts)
    print(f"S={S}: proven {proven} of {len(pkts)}, repaired {repaired}")
    proven, _, repaired = SR.decode_and_check(dev, pkts[1:] if S == 3 else pkts[2:])
    if S == 3:  # both pictures of zeros in step from the first byte: pass 1 wrote their index
        assert (proven, repaired) == (2, 0)
    else:
        assert (proven, repaired) == (1, 0)


def test_repairs_behind_a_run_emission(dev, S):
    """noise of +-32 at Q = 255, six 640x368 packets: pass 1 emits runs whose chunks are then walked again, pass 2 emits
    those packets chunk by chunk.  Index and planes are the oracle's for proven and refused packets alike.
    (With the emission per chunk the same content had 218 / 139 / 118 chunks repaired at S = 2 / 3 / 4, and so it has
    now: no S is left out.)"""
    pkts = list(SR.noisy_packets())
    proven, _, repaired = SR.decode_and_check(dev, pkts)
    print(f"S={S}: proven {proven} of {len(pkts)}, repaired {repaired}")
    assert repaired >= 1, "pass 2 did not run"
