"""The row hand-back of the pooling chroma wave and the block bookkeeping of the split form's luma waves.

k_decode_split's chroma wave hands a group's rows back two at a time: one 16-byte LDS read per pair of rows, a DC-only
lane reading its pixel from its own scratch, a busy lane the rows of its rank.  Its luma waves (decode_wave<kSuper>) add
a block's index and its place in the picture up from a wave-uniform share and a constant per lane.  What can go wrong
there depends on the geometry (rows as wide as a group, a row wrap inside a group, rows narrower than a group, a last
super group of a single macroblock) and on which lanes are busy, so every case here is a plan of small pictures of one
geometry, decoded in every form of a batch launch (tests/test_gpu_split_edges.py: split, classic, one part per wave,
classic with the fewest waves) into outputs prefilled with two different bytes and compared byte for byte with the CPU
oracle; in the split form the number of parts left to k_decode_list must be what tests/pool_model.py says.

Content, per geometry: the directed rounds of pool_model.pool_packets() rebuilt on it (every partition of three groups,
the bails, every block length, both sides of the three-input budget); busy blocks on the odd lanes alone, on the even
lanes alone (busy and DC-only blocks alternate lane by lane: a wrong pairing of rows shows in every second row), on the
lanes of the odd or of the even macroblock rows alone; and busy blocks whose only coefficient outside the low 4x4 is a
single one, on 512x48 at each of the 48 places there are, which must all bail.  Last, two 720x576 pictures whose luma
waves run two super groups each and whose blocks all differ between the two: the second must come out as itself."""
import numpy as np
import pytest

import edge_packets as E
import pool_model as PM
import rtjlib as R
import test_gpu_split_edges as SE
import test_gpu_parity as T
from pkg import P

S = SE.S
M = SE.M
PG, MB = S.kPoolGroups, S.kMbPerGroup
GEOMETRIES = ((512, 48), (720, 48), (208, 112), (1552, 16))
BRANCHES = {(512, 48): {"no-wrap"}, (720, 48): {"no-wrap", "wrap"}, (208, 112): {"narrow"}, (1552, 16): {"no-wrap"}}
OUTSIDE_LOW4 = [n for n in range(64) if (n >> 3) >= 4 or (n & 7) >= 4]  # natural order: 48 places
# on the other geometries: the last place in natural and in zig-zag order, the corners, and the four next to the low 4x4
OUTSIDE_PICK = (63, 7, 56, 4, 32, 28, 35)


@pytest.fixture(scope="module")
def dev():
    d = P.MiRtj()
    yield d
    d.close()


def test_geometries_are_what_they_are_chosen_for():
    assert (512 // 16, 720 // 16, 208 // 16) == (MB, 45, 13)
    for (w, h), want in BRANCHES.items():
        assert {M.store_branch(w, h, g) for g in range(S.groups(w, h))} == want, (w, h)
    assert S.groups(720, 48) == 5 and S.last_group_mbs(720, 48) == 7          # a last group that is partly empty
    assert S.groups(1552, 16) == 4 and S.last_group_mbs(1552, 16) == 1        # a second super group of one macroblock
    assert S.super_groups(S.groups(1552, 16)) == 2 and S.super_groups(S.groups(512, 48)) == 1


def every_round(w, h, make):
    """the same kind of round in every super group of the picture (make(sg) -> kPoolGroups group specs)"""
    return {sg: make(sg) for sg in range(S.super_groups(S.groups(w, h)))}


def outside_block(rng, nat):
    """DC, a run, one value at natural place `nat` (outside the low 4x4), the run to the end if there is one"""
    blk = PM.tokens_block(int(rng.integers(0, 201)), [(E.ZZ.index(nat), int(rng.choice([-3, -2, 2, 3])))])
    assert 3 <= len(blk) <= 4
    return blk


def directed(w, h, seed):
    """[(name, packet)] of one geometry"""
    rng = np.random.default_rng(seed)
    B3 = E.Budget(S.csrc).budget3
    mbw = w // 16
    out = []

    def add(name, make, Q=255):
        out.append((f"{name}-{w}x{h}", PM.build_packet(rng, w, h, Q, every_round(w, h, make), S)))

    # ---- the pooling wave's decisions, as pool_packets() directs them ----
    for c in PM.PARTITIONS:
        add("partition-" + "-".join(map(str, c)), lambda sg, c=c: [PM.group(rng, busy=n) for n in c])
    add("all-unchanged", lambda sg: [PM.group(rng, rest="ff") for _ in range(PG)])
    add("unchanged-among-busy", lambda sg: [PM.group(rng, busy=20, rest="ff"), PM.group(rng, rest="ff"), PM.group(rng, busy=9)])
    add("bail-pool-of-one", lambda sg: [PM.group(rng, busy=40, put={5: PM.b_bail(rng)}), PM.group(rng, busy=40), PM.group(rng, busy=10)])
    add("bail-pool-of-two", lambda sg: [PM.group(rng, busy=20), PM.group(rng, busy=20, put={63: PM.b_bail(rng, 14)}), PM.group(rng, busy=60)])

    def bail3(sg):
        g = [PM.group(rng, busy=n, scatter=False) for n in (21, 21, 22)]
        g[2][3] = PM.b_bail(rng)
        return g
    add("bail-pool-of-three", bail3)
    add("lengths", lambda sg: [PM.group(rng, busy=18, lengths=(3, 4, 5, 6, 7, 8), run127=True) for _ in range(PG)])
    add("lengths-8low3", lambda sg: [PM.group(rng, busy=10, lengths=("8low3", 7, 3)), PM.group(rng, busy=0, run127=True),
                                     PM.group(rng, busy=30, lengths=(8,))])
    add("nine-bytes", lambda sg: [PM.group(rng, busy=12), PM.group(rng, busy=12, put={0: PM.b_busy(rng, 9)}), PM.group(rng, busy=12)])
    for Q in PM.BUDGET_QUALITIES:
        quiet = lambda n=14: PM.group(rng, busy=n, lengths=(3, 4, 5, 6, 7, "8low3"))
        lane = lambda side, v=0, Q=Q: E.block_bytes(PM.budget3_tokens(Q, side, B3, v), 0)
        add(f"budget-q{Q}-in", lambda sg: [quiet(), quiet(), PM.group(rng, busy=14, put={7: lane("in")})], Q)
        add(f"budget-q{Q}-out", lambda sg: [quiet(), PM.group(rng, busy=14, put={40: lane("out")}), quiet()], Q)
        add(f"budget-q{Q}-far", lambda sg: [PM.group(rng, busy=14, put={22: lane("far")}), quiet(), quiet()], Q)
        add(f"budget-q{Q}-four", lambda sg: [quiet(), PM.group(rng, busy=14, put={9: PM.b_four(rng, 9)}), PM.group(rng, busy=14, put={1: PM.b_four(rng, 6)})], Q)
        add(f"budget-q{Q}-mixed", lambda sg: [PM.group(rng, busy=14, put={l: lane("in" if (sg + q) & 1 else "out", 1 + l % 7 + 7 * q)
                                                                              for l in range(0, 64, 9)}) for q in range(PG)], Q)

    # ---- which lanes are busy: the row hand-back ----
    lengths = (4, 5, 6, 7, "8low3", 8, 3)

    def on_lanes(lanes, rest="dc"):
        lanes = list(lanes)
        put = {l: (PM.b_busy8_low3(rng) if lengths[i % 7] == "8low3" else PM.b_busy(rng, lengths[i % 7], vmax=6)) for i, l in enumerate(lanes)}
        return PM.group(rng, busy=0, rest=rest, put=put)

    def on_rows(sg, q, parity):
        g = sg * PG + q
        return on_lanes(l for l in range(2 * MB) if ((g * MB + l % MB) // mbw) & 1 == parity)

    add("odd-lanes", lambda sg: [on_lanes(range(1, 64, 2)) for _ in range(PG)])
    add("even-lanes", lambda sg: [on_lanes(range(0, 64, 2)) for _ in range(PG)])
    add("odd-then-even-lanes", lambda sg: [on_lanes(range(1, 64, 2)), on_lanes(range(0, 64, 2)), on_lanes(range(1, 64, 2))])
    add("odd-lanes-rest-unchanged", lambda sg: [on_lanes(range(1, 64, 2), "ff"), on_lanes(range(0, 64, 2), "ff"), on_lanes(range(0, 64, 4))])
    add("odd-macroblock-rows", lambda sg: [on_rows(sg, q, 1) for q in range(PG)])
    add("even-macroblock-rows", lambda sg: [on_rows(sg, q, 0) for q in range(PG)])
    add("every-lane-busy", lambda sg: [on_lanes(range(64)) for _ in range(PG)])

    # ---- a single coefficient outside the low 4x4: every pool of the round must bail ----
    places = OUTSIDE_LOW4 if (w, h) == (512, 48) else OUTSIDE_PICK
    for i in range(0, len(places), PG):
        three = [places[(i + q) % len(places)] for q in range(PG)]
        # 64 busy blocks per group: every group is a pool of its own, and each holds one such block, as the Cb or the Cr
        # block of its first macroblock (which every group has)
        add("outside-" + "-".join(map(str, three)),
            lambda sg, three=three: [PM.group(rng, busy=64, put={MB * ((n + q) & 1): outside_block(rng, n)}) for q, n in enumerate(three)])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", GEOMETRIES)
def test_directed_rounds_in_every_form(dev, monkeypatch, w, h):
    items = directed(w, h, seed=1000 + w)
    pkts = [p for _, p in items]
    groups = S.groups(w, h)
    for name, p in items:
        pic = M.picture(p)
        if name.startswith("outside-"):  # every group that exists is listed, none stored
            assert sorted(pic.listed) == list(range(groups)), (name, pic.listed)
        if name.rsplit("-", 1)[0] in ("odd-lanes", "even-lanes", "odd-then-even-lanes", "every-lane-busy"):
            assert not pic.listed and all(r.stored == sum(g.exists for g in r.groups) for r in pic.rounds), name
    want = M.parts_listed(pkts)
    assert want >= groups * sum(n.startswith("outside-") for n, _ in items)
    for rep in SE.every_form(dev, monkeypatch, pkts, f"split trim {w}x{h}: " + ", ".join(n for n, _ in items), launches=2):
        print(f"{w}x{h}: {len(pkts)} packets, parts_listed {rep['parts_listed']}, the model's {want}")
        assert rep["parts_listed"] == want, (w, h, rep["parts_listed"], want)


# --------------------------------------------------------------------------- a luma wave's second super group
def carry_packet(w, h, salt, rng):
    """every luma block its own DC and two raw coefficients, by macroblock, block and `salt`; chroma: ordinary groups"""
    _, _, lb8, cb8, _, _ = R.oracle_tables(255)
    assert cb8 == 0 and lb8 >= 2
    nmb = (w // 16) * (h // 16)
    specs = [PM.group(rng, busy=int(rng.integers(8, 20))) for _ in range(S.groups(w, h))]
    blocks, luma = [], []
    for mb in range(nmb):
        for k in range(4):
            tok = np.zeros(64, np.int64)
            n = 4 * mb + k
            tok[0] = (37 * n + salt) % 251
            tok[1] = (n + salt) % 7 - 3
            tok[2] = (n // 7 + salt) % 5 - 2
            luma.append(E.block_bytes(tok, lb8))
            blocks.append(luma[-1])
        blocks.append(specs[mb // MB][mb % MB])
        blocks.append(specs[mb // MB][MB + mb % MB])
    return E.packet_from_blocks(w, h, 255, blocks), luma


@pytest.mark.gpu
def test_second_super_group_of_a_luma_wave(dev, monkeypatch):
    w, h = 720, 576
    groups = S.groups(w, h)
    lw = S.split_luma_waves(groups)
    step = S.kXcds * lw
    nsg = S.super_groups(groups)
    assert nsg > step  # some luma wave runs a second super group ...
    a, b = S.split_owner(0, lw, S.kSplitXcdRot, 0), S.split_owner(step, lw, S.kSplitXcdRot, 0)
    assert (a["stripe"], a["wave"], a["round"], b["stripe"], b["wave"], b["round"]) == (0, 0, 0, 0, 0, 1)
    assert M.store_branch(w, h, 1) == "wrap"
    rng = np.random.default_rng(576)
    (p0, l0), (p1, l1) = carry_packet(w, h, 0, rng), carry_packet(w, h, 101, rng)
    for luma in (l0, l1):  # ... whose blocks differ, lane by lane, from the first one's
        for sg in range(step, nsg):
            for mb in range(sg * PG * MB, min((sg + 1) * PG * MB, (w // 16) * (h // 16))):
                for k in range(4):
                    assert luma[4 * mb + k] != luma[4 * (mb - step * PG * MB) + k]
    assert all(x != y for x, y in zip(l0, l1))
    pkts = [p0, p1]
    want = M.parts_listed(pkts)
    for rep in SE.every_form(dev, monkeypatch, pkts, "two super groups per luma wave", launches=2):
        assert rep["parts_listed"] == want, (rep["parts_listed"], want)
