"""The packets built to break the transform's arithmetic, through every form of a batch launch.

With no environment set a handful of small pictures runs k_decode<false, false> (one part per wave, blocks outside the
packed passes' budget transformed in the same kernel), so the edge packets of tests/test_gpu_parity.py and
tests/test_gpu_dc_only.py never met the form that carries a batch: k_decode_split — luma waves that leave a part with
a block over the 16-bit budget to a list, chroma waves that pool the busy blocks of three groups, k_decode_list for
what either declines — nor k_decode<true, false>.  Here every lifted edge set (tests/edge_packets.py) and the packets
directed at the pooling wave's decisions (tests/pool_model.py) run through the split form, the classic form, the form
of one part per wave and the classic form with the fewest waves, each forced by the environment and checked against
what the plan says ran; in the split form the number of group parts left to the list must be what the models say.
Guard bytes, odd output offsets, the block index and the failure message are those of tests/test_gpu_launch_shapes.py.
Integer work: every byte of every picture equals the oracle's, in outputs prefilled with two different bytes."""
import re

import numpy as np
import pytest

import edge_packets as E
import launch_shapes as LS
import pool_model as PM
import rtjlib as R
import test_gpu_launch_shapes as L
import test_gpu_parity as T
from pkg import P

pytestmark = pytest.mark.gpu

S = L.S
M = PM.Model(S)
PREFILLS = L.PREFILLS


@pytest.fixture(scope="module")
def dev():
    d = P.MiRtj()
    yield d
    d.close()


def oracle_in_order(pkts, prefill):
    """one decoder, the packets in order: the header state machine of a plan (every picture into its own buffer)"""
    dec, out = R.OracleDecoder(), []
    for p in pkts:
        want = np.full(T.frame_bytes(*T.packet_size(p)), prefill, np.uint8)
        dec.decode(p, want)
        out.append(want)
    return out


def every_form(dev, monkeypatch, pkts, name, launches=1, in_order=False, only=None):
    """the plan in every form and both prefills; returns what the split form's launches reported"""
    mg = max(S.groups(*T.packet_size(p)) for p in pkts)
    reps = []
    for prefill in PREFILLS:
        wants = oracle_in_order(pkts, prefill) if in_order else L.oracle_pictures(pkts, prefill)
        for form, (env, expect) in L.forms(mg).items():
            if only and form not in only:
                continue
            rep = L.run_form(dev, monkeypatch, pkts, wants, name, form, env, expect, prefill, max_groups=mg, launches=launches)
            if form == "split":
                reps.append(rep)
    return reps


def kat_packets():
    G = np.load(R.GOLDEN + "/rtjpeg_golden.npz")
    return [G[f"kat_{ki}_pkt"] for (ki, *_) in G["kat_meta"]]


EDGE_SETS = {
    "low4x4": E.low_4x4_packets,
    "dc_spellings": E.dc_spelling_packets,
    "chunks": E.chunk_boundary_packets,
    "kat": kat_packets,
    "adversarial": lambda: E.adversarial_packets()[0],  # Q = 1, 2, 3, 8, 31, 129, 192, 255 in one plan
}


# --------------------------------------------------------------------------- 1. every lifted edge set in every form
@pytest.mark.parametrize("name", list(EDGE_SETS))
def test_edge_set_in_every_form(dev, monkeypatch, name):
    pkts = EDGE_SETS[name]()
    if name == "adversarial":
        assert sorted({int(p[10]) for p in pkts}) == sorted(E.ADVERSARIAL_QUALITIES)
    every_form(dev, monkeypatch, pkts, name, in_order=name in ("adversarial", "kat"))


def luma_parts(meta, need_beyond):
    """(group, part) pairs of a budget packet that hold a luma block over the budget (and, need_beyond, one of whose
    dequantised coefficients lies outside the low 4x4)"""
    over = meta["sums"] > meta["budget"]
    if need_beyond:
        over = over & meta["beyond_low4"]
    b = np.nonzero(over)[0]
    b = b[b % 6 < 4]
    return {(int(x) // 6 // S.kMbPerGroup, int(x) % 6 // 2) for x in b}


def test_budget_packets_in_every_form(dev, monkeypatch):
    """The packed passes' budget in the kList instantiation: a luma part with a block over the budget goes to the list.
    Per mix, the two qualities in one plan, in the split form:

    lower bound: a part holding a block that is over the budget AND reaches outside the low 4x4 is listed whatever the
    wave's history (try_lo_y) was — such a block fails the low-4x4 test where it is tried, and the packed passes' range
    test either way.  This bound alone is exact in that sense; a part whose over-budget blocks all lie inside the low
    4x4 is listed only if an earlier part of its wave had stopped the low-4x4 test.
    upper bound: no part without an over-budget block is listed, and the chroma parts listed are the pool model's.

    The mix "all_in" as the pinned builder makes it holds 9 + 27 luma blocks that stepping one token left above the
    budget, so its count is bounded like the others'; built strictly (every block inside, the just-inside ones
    included) no luma part may be listed: parts_listed is the chroma model's count, exactly."""
    pkts, seen, meta = E.budget_packets()
    every_form(dev, monkeypatch, pkts, "budget")
    mixes = sorted({m["mix"] for m in meta})
    assert mixes == ["all_in", "mixed", "one_out_per_group"]
    for mix in mixes:
        sub = [(p, m) for p, m in zip(pkts, meta) if m["mix"] == mix]
        lo = sum(len(luma_parts(m, True)) for _, m in sub)
        hi = sum(len(luma_parts(m, False)) for _, m in sub) + M.parts_listed([p for p, _ in sub])
        assert lo > 0
        for rep in every_form(dev, monkeypatch, [p for p, _ in sub], f"budget/{mix}", only=("split",)):
            print(f"budget/{mix}: parts_listed {rep['parts_listed']}, bounds {lo} .. {hi}")
            assert lo <= rep["parts_listed"] <= hi, (mix, lo, rep["parts_listed"], hi)
    spk, _, smeta = E.budget_packets(mixes=((512, 32, "all_in"),), strict_in=True)
    assert all((m["sums"] <= m["budget"]).all() for m in smeta)
    near = sum(int((m["budget"] - m["sums"] < m["budget"] // 50).sum()) for m in smeta)
    assert near > 100, near  # the just-inside blocks are there
    chroma = M.parts_listed(spk)
    for rep in every_form(dev, monkeypatch, spk, "budget/all_in built strictly", only=("split",)):
        assert rep["parts_listed"] == chroma, (rep["parts_listed"], chroma)


# --------------------------------------------------------------------------- 2. when a luma wave appends to the list
def luma_timing_packet(rng, over, unchanged, Q=255, w=1024, h=416):
    """DC-only chroma, DC-only luma but for: over = {(group, part): lane}: one block far over the packed passes'
    budget, reaching outside the low 4x4; unchanged = {(group, part)}: all 64 blocks of the part 0xFF"""
    B = E.Budget()
    liqt, _, lb8, cb8, _, _ = R.oracle_tables(Q)
    assert cb8 == 0
    tok = np.zeros(64, np.int64)
    tok[0] = 200
    tok[1:41] = -128
    assert B.weighted(tok, liqt) > 2 * B.budget
    big = E.block_bytes(tok, lb8)
    blocks = []
    for mb in range((w // 16) * (h // 16)):
        g, dmb = mb // S.kMbPerGroup, mb % S.kMbPerGroup
        for k in range(4):
            part = k // 2
            if (g, part) in unchanged:
                blocks.append([255])
            elif over.get((g, part)) == 2 * dmb + (k & 1):
                blocks.append(big)
            else:
                blocks.append([int(rng.integers(0, 255))] + [0] * lb8 + [63 + 63 - lb8])
        blocks += [[int(rng.integers(0, 255)), 126], [int(rng.integers(0, 255)), 126]]
    return E.packet_from_blocks(w, h, Q, blocks)


def test_luma_wave_lists_a_part_in_its_first_middle_and_last_round(dev, monkeypatch):
    """A luma wave appends behind the counted wait in a round that is not its last and behind the loop in its last one.
    1024x416: the luma wave 0 of stripe 0 takes the super groups of its stripe in turn, three groups of two parts each."""
    w, h = 1024, 416
    groups = S.groups(w, h)
    lw = S.split_luma_waves(groups)
    mine = [sg for sg in range(S.super_groups(groups))
            if (lambda o: o["stripe"] == 0 and o["wave"] == 0)(S.split_owner(sg, lw, S.kSplitXcdRot, 0))]
    assert len(mine) >= 2 and [S.split_owner(sg, lw, S.kSplitXcdRot, 0)["round"] for sg in mine] == list(range(len(mine)))
    gs = [S.kPoolGroups * sg + q for sg in mine for q in range(S.kPoolGroups)]  # the wave's groups, in its order
    assert gs[-1] < groups
    first, mid, last = gs[0], gs[len(gs) // 2], gs[-1]
    rng = np.random.default_rng(8)
    cases = [
        (dict([((first, 0), 27), ((mid, 0), 0), ((last, 0), 63)]), set()),   # part 0: first, middle, last group
        (dict([((first, 1), 5), ((mid, 1), 40), ((last, 1), 62)]), set()),   # part 1: the last one is the wave's last iteration
        (dict([((last, 1), 1)]), set()),                                     # nothing but the last iteration
        # a part of nothing but unchanged blocks between two stored parts, then a listed one; and one right before a listed part
        (dict([((gs[2], 0), 9), ((mid, 1), 33)]), {(gs[1], 0), (mid, 0)}),
        (dict([((first, 0), 2), ((first, 1), 3), ((gs[1], 0), 4)]), {(last, 0)}),  # three listed in a row from the start
    ]
    pkts = [luma_timing_packet(rng, over, ff) for over, ff in cases]
    want_listed = sum(len(over) for over, _ in cases)
    assert M.parts_listed(pkts) == 0  # the chroma is DC only
    for rep in every_form(dev, monkeypatch, pkts, "luma list timing", launches=2):
        assert rep["parts_listed"] == want_listed, (rep["parts_listed"], want_listed)


# --------------------------------------------------------------------------- 3. the pooling wave's decisions
@pytest.fixture(scope="module")
def pool():
    return PM.pool_packets(S)


def test_pool_packets_in_every_form(dev, monkeypatch, pool):
    """Pictures of the same size share a plan (a plan of one geometry: the wave counts are the picture's own).  Every
    plan twice back to back without a sync: the list counters flip, the second launch must give the same bytes and
    leave the same number of parts to the list — the model's, exactly (the luma is DC only: never listed)."""
    by_size = {}
    for name, p in pool:
        by_size.setdefault(T.packet_size(p), []).append((name, p))
    for (w, h), items in by_size.items():
        pkts = [p for _, p in items]
        if len(pkts) == 1:
            pkts = pkts * 2
        want = M.parts_listed(pkts)
        for rep in every_form(dev, monkeypatch, pkts, f"pool packets {w}x{h}: " + ", ".join(n for n, _ in items), launches=2):
            assert rep["parts_listed"] == want, (w, h, rep["parts_listed"], want)


def test_pool_packet_at_every_byte_alignment(dev, monkeypatch, pool):
    """the 12-byte window of a pooled block is read at byte alignment (packet's first data byte + block start) & 3"""
    byname = dict(pool)
    for name in ("lengths-1024x224", "forms-1024x224-q20"):
        pkts, at = PM.aligned_plan(byname[name])
        want = M.parts_listed(pkts)
        for rep in every_form(dev, monkeypatch, pkts, f"alignment of {name}", only=("split", "classic")):
            assert rep["parts_listed"] == want, (name, rep["parts_listed"], want)


# --------------------------------------------------------------------------- 4. a list longer than k_decode_list's grid
def test_list_longer_than_the_grid_of_k_decode_list(dev, monkeypatch):
    """24 pictures of 1024x512 of arbitrary bytes, qualities alternating: nearly every part of every group goes to the
    list, k_decode_list's workgroups take a second entry — of the other quality's tables as likely as not (the order
    of the entries comes from atomics) — and rewrite their slot tables in between."""
    grid = int(re.search(r"constexpr unsigned kDecListGrid = (\d+);", open(LS.CSRC + "/rtj_decode_chroma.h").read()).group(1))
    w, h, n = 1024, 512, 24
    rng = np.random.default_rng(4096)
    nbytes = (w // 16) * (h // 16) * 6 * 24
    pkts = [np.concatenate([L.header(w, h, (255, 60)[i & 1], 12 + nbytes), rng.integers(0, 256, nbytes, dtype=np.uint8)])
            for i in range(n)]
    assert 3 * S.groups(w, h) * n > grid
    wants = L.oracle_pictures(pkts, 0xA5)
    env, expect = L.forms(S.groups(w, h))["split"]  # MI_RTJ_SPLIT=1: forced, no policy
    rep = L.run_form(dev, monkeypatch, pkts, wants, "long list", "split", env, expect, 0xA5, launches=2)
    assert rep["parts_listed"] > grid, (rep["parts_listed"], grid)


# --------------------------------------------------------------------------- 5. a session: the kPrev instantiation
def session(dev, pkts, w, h):
    """the packets as one stream through mi_rtj_pipe_*, depth 4, behind a whole picture of ordinary content; against
    one oracle decoder taking them in order into one picture"""
    first = R.OracleEncoder(w, h, 200).encode(R.synth_frame(w, h, 0, seed=3, amp=20))
    stream = [first] + list(pkts)
    dec, pic = R.OracleDecoder(), np.zeros(T.frame_bytes(w, h), np.uint8)
    pipe = dev.pipe(depth=4, coded_w=w, coded_h=h)
    fed = got = 0
    while got < len(stream):
        while fed < len(stream) and pipe.room() > 0:
            pipe.submit(stream[fed], fed)
            fed += 1
        y, u, v, tag = pipe.next()
        assert tag == got
        dec.decode(stream[got], pic)
        d = np.nonzero(np.concatenate([y, u, v]) != pic)[0]
        assert d.size == 0, (f"{w}x{h} session, packet {got}: {d.size} bytes differ, first at {int(d[0])}: "
                             + S.describe_byte(w, h, int(d[0]), "span1"))
        got += 1
    assert pipe.pending() == 0
    pipe.close()


def test_sessions_on_the_budget_and_pool_packets(dev, pool):
    pkts, _, meta = E.budget_packets()
    session(dev, [p for p, m in zip(pkts, meta) if (m["w"], m["h"]) == (1024, 64)], 1024, 64)
    session(dev, [p for _, p in pool if T.packet_size(p) == (1024, 224)], 1024, 224)
