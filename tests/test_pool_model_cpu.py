"""The directed packets of tests/pool_model.py reach, by the model's own account, every decision of a pooling chroma
wave they are built for — so that tests/test_gpu_split_edges.py cannot lose a case without this census saying so — and
the model's class of every chroma block agrees with the oracle's picture.  Every scenario is counted and required."""
import numpy as np
import pytest

import edge_packets as E
import launch_shapes as LS
import pool_model as PM
import rtjlib as R

S = LS.Shapes()
M = PM.Model(S)


@pytest.fixture(scope="module")
def built():
    pk = PM.pool_packets(S)
    assert len({n for n, _ in pk}) == len(pk)
    return {n: (p, M.picture(p)) for n, p in pk}


def rounds_of(built, prefix):
    return [(n, r) for n, (_, P) in built.items() if n.startswith(prefix) for r in P.rounds]


def stripe(P, x):
    """the rounds of the wave that owns stripe x, wave 0, in order"""
    return [r for r in P.rounds if r.owner["stripe"] == x and r.owner["wave"] == 0]


def test_constants_are_the_headers():
    text = open(LS.CSRC + "/rtj_decode_chroma.h").read()
    assert f"len > {PM.SHORT_MAX}u" in text and f"tot + cnt[q] <= {PM.POOL_LANES}u" in text
    assert "pos + len > f.data_len" in text and "len == 2u ? 1u : 2u" in text
    assert "12u * 32768u - (uint32_t)(kPkBudget / 4)" in open(LS.CSRC + "/rtj_idct_pk.h").read()
    assert M.budget3 == 32670 == E.Budget().budget // 4


def test_luma_is_dc_only_everywhere(built):
    """no luma part of these packets can be listed: every luma block is its DC and one run"""
    for n, (p, P) in built.items():
        if n.startswith("cut-"):
            continue
        _, _, lb8, _, _, _ = R.oracle_tables(P.Q)
        off = R.OracleDecoder().block_offsets(p)
        for mb in range(P.nmb):
            for k in range(4):
                a, b = int(off[6 * mb + k]), int(off[6 * mb + k + 1])
                assert b - a == lb8 + 2 and not p[a + 1:b - 1].any() and p[b - 1] == 63 + 63 - lb8, (n, mb, k)


def test_shapes_reach_every_branch_of_the_store_address(built):
    seen = {}
    for n, (_, P) in built.items():
        if n.startswith("one-round"):
            assert P.groups == S.kPoolGroups and P.nsg == 1, n
            for g in range(P.groups):
                seen.setdefault(M.store_branch(P.w, P.h, g), set()).add((P.w, P.h))
    assert seen["narrow"] == {(256, 96)} and (768, 32) in seen["wrap"] and {(512, 48), (1536, 16)} <= seen["no-wrap"], seen
    P = built["partitions-1024x416"][1]
    assert (P.groups, P.nsg) == (52, 18) and P.cw == 1
    assert [r.sg for r in stripe(P, 0)] == [0, 8, 16] and [r.sg for r in stripe(P, 1)] == [1, 9, 17]
    assert [r.have_nn for r in stripe(P, 0)] == [True, False, False] and [r.last for r in stripe(P, 0)] == [False, False, True]
    assert [g.exists for g in P.rounds[17].groups] == [True, False, False]  # the last super group is partial
    P = built["lengths-1024x224"][1]
    assert (P.groups, P.nsg) == (28, 10)
    assert [len(stripe(P, x)) for x in range(S.kXcds)] == [2, 2, 1, 1, 1, 1, 1, 1]  # two waves run two rounds
    for n in ("two-groups-176x48-busy-tail", "two-groups-176x48-dc-tail"):
        P = built[n][1]
        assert P.nmb == 33 and P.groups == 2
        g1 = P.rounds[0].groups[1]
        assert g1.valid.sum() == 2 and not g1.gslow and (g1.cls[~g1.valid] == PM.NONE).all()
    assert built["two-groups-176x48-busy-tail"][1].rounds[0].groups[1].cnt == 2
    assert (built["two-groups-176x48-dc-tail"][1].rounds[0].groups[1].cls[[0, 32]] == PM.DC_ONLY).all()


@pytest.mark.parametrize("counts", list(PM.PARTITIONS))
def test_every_partition_appears(built, counts):
    """in a one-round picture and in a round of 1024x416, with the pools the kernel must make of the counts"""
    want = PM.PARTITIONS[counts]
    for prefix in ("one-round", "partitions-1024x416"):
        hits = [r for _, r in rounds_of(built, prefix) if r.counts == counts and any(g.gstore for g in r.groups)]
        assert len(hits) >= 1, (prefix, counts)
        for r in hits:
            assert r.partition == want and not r.listed and r.stored == S.kPoolGroups, (prefix, counts, r.partition)
            if counts == (0, 0, 0):
                assert all((g.cls == PM.DC_ONLY).all() for g in r.groups)
    if sum(counts) == PM.POOL_LANES:
        assert len(want) == 1  # one pool of exactly 64: the test's own claim


def test_rounds_of_nothing_but_unchanged_blocks(built):
    for n, sg in (("one-round-512x48-all-unchanged", 0), ("partitions-1024x416", 8)):
        r = built[n][1].rounds[sg]
        assert all((g.cls == PM.UNCHANGED).all() and not g.gstore for g in r.groups)
        assert r.stored == 0 and not r.listed and all(p.skipped for p in r.pools)
    # in the big picture it lies between two rounds of the same wave that store
    st = stripe(built["partitions-1024x416"][1], 0)
    assert [r.stored for r in st] == [3, 0, 3]


def test_lengths(built):
    P = built["lengths-1024x224"][1]
    lens = {L: 0 for L in range(2, 9)}
    runs = {126: 0, 127: 0}
    for r in P.rounds:
        for g in r.groups:
            for l in np.nonzero(g.cls == PM.BUSY)[0]:
                lens[int(g.len[l])] += 1
            for l in np.nonzero(g.cls == PM.DC_ONLY)[0]:
                lens[2] += 1
                runs[int(g.bytes[l][1])] += 1
    assert all(v >= 10 for v in lens.values()), lens
    assert runs[126] >= 50 and runs[127] >= 50, runs
    # a nine-byte block in exactly one group of a round: that group is listed, the other two are pooled and stored;
    # once in a round that is not its wave's last, once in one that is
    for sg, q, last in ((1, 1, False), (8, 0, True)):
        r = P.rounds[sg]
        assert r.last == last and r.listed == [S.kPoolGroups * sg + q] and r.stored == 2
        assert int((r.groups[q].len == 9).sum()) == 1 and r.groups[q].gslow
        assert [g.gslow for g in r.groups].count(True) == 1
        # (what a kernel that took nine bytes for short would do: parse eight, bail the pool the group is in — so the
        # group must share its pool for `parts_listed` to tell)
        assert len(r.pools) == 1 and r.pools[0].form is not None
    assert P.listed == [4, 24]


def test_packet_end(built):
    whole, P = built["lengths-1024x224"]
    last = P.rounds[-1].groups[0]
    assert last.g == P.groups - 1 and not last.gslow and last.cls[63] == PM.BUSY
    assert int(last.pos[63] + last.len[63]) == P.data_len  # pos + len == data_len: still pooled
    short = built["cut-one-byte-short-1024x224"][1]
    assert short.data_len == P.data_len - 1 and short.rounds[-1].groups[0].gslow
    assert short.listed == P.listed + [P.groups - 1]
    alone = built["cut-header-alone-1024x224"][1]
    assert alone.data_len == 0 and alone.listed == list(range(P.groups))


def test_bail(built):
    P = built["bail-1024x416"][1]
    want = {  # super group: (partition, the pool that bails, groups stored, is the round its wave's last)
        0: (((0,), (1, 2)), 0, 2, False), 10: (((0,), (1, 2)), 0, 2, True),
        1: (((0, 1), (2,)), 0, 1, False), 11: (((0, 1), (2,)), 0, 1, True),
        4: (((0, 1, 2),), 0, 0, False), 12: (((0, 1, 2),), 0, 0, True),
    }
    for sg, (part, bp, stored, last) in want.items():
        r = P.rounds[sg]
        assert r.partition == part and r.last == last and r.stored == stored, (sg, r.partition, r.last, r.stored)
        assert [p.bail for p in r.pools] == [i == bp for i in range(len(part))]
        assert r.listed == [S.kPoolGroups * sg + q for q in part[bp]]
        # the block that bails is four bytes, DC, run, value, run, and the only one of its kind in the pool
        four = [(q, l) for q in part[bp] for l in np.nonzero(r.groups[q].cls == PM.BUSY)[0]
                if (PM.short_coefficients(r.groups[q].bytes[l], R.oracle_tables(P.Q)[1])[~PM._LOW4] != 0).any()]
        assert len(four) == 1 and r.groups[four[0][0]].len[four[0][1]] == 4
        if len(part) > 1:
            assert r.pools[1].form is not None  # another pool of the round stores
    assert want[4][0] == ((0, 1, 2),) and sum(P.rounds[4].counts) == PM.POOL_LANES == sum(P.rounds[12].counts)
    assert sorted(P.listed) == sorted(g for sg, (part, bp, *_) in want.items() for g in [S.kPoolGroups * sg + q for q in part[bp]])


@pytest.mark.parametrize("Q", PM.BUDGET_QUALITIES)
def test_forms_and_both_sides_of_the_three_input_budget(built, Q):
    P = built[f"forms-1024x224-q{Q}"][1]
    forms = [r.pools[0].form for r in P.rounds]
    assert all(len(r.pools) == 1 and not r.listed for r in P.rounds)
    assert forms[:7] == ["packed3", "packed3", "plain3", "packed3", "four", "plain3", "four"], forms
    B = M.budget3
    # round 2: one lane of group 1 is the smallest sum above the budget, everything else far inside; round 3: one lane
    # of group 2 the largest sum not above it; round 5: a lane far outside (under twice the budget)
    s2, s3, s5 = (sorted(P.rounds[i].pools[0].sums) for i in (2, 3, 5))
    assert B < s2[-1] < B + B // 50 and s2[-2] < B - B // 10
    assert B - B // 50 < s3[-1] <= B and s3[-2] < B - B // 10
    assert B + 3000 < s5[-1] < 2 * B and s5[-2] < B - B // 10
    assert P.rounds[2].groups[1].cnt and P.rounds[2].groups[0].cnt  # the lane's pool holds other groups' blocks
    # the near band, both sides, over the whole picture
    sums = np.array([s for r in P.rounds for s in r.pools[0].sums])
    near_in = int(((sums <= B) & (sums > B - B // 50)).sum())
    near_out = int(((sums > B) & (sums < B + B // 50)).sum())
    assert near_in >= 20 and near_out >= 20 and int((sums < B // 2).sum()) > 100, (near_in, near_out)
    assert "plain3" in forms[7:]


@pytest.mark.parametrize("Q", (255, 128, 1))
def test_dc_only_pixel_of_every_dc_byte(built, Q):
    p, P = built[f"dc-bytes-1024x32-q{Q}"]
    q0 = int(R.oracle_tables(Q)[1][0])
    assert (q0 == 2730) == (Q == 1)
    seen = set()
    for r in P.rounds:
        assert r.counts == (0,) * len(r.counts) and not r.listed
        for g in r.groups:
            if g.exists:
                seen |= {int(b[0]) for b in g.bytes if b is not None}
                assert (g.cls[g.valid] == PM.DC_ONLY).all()
    assert seen == set(range(255))
    wraps = [b for b in range(255) if b * q0 > 32767]
    assert (wraps[:1] == [13] and len(wraps) == 242) if Q == 1 else not wraps


def test_wait_arms(built):
    for order in PM.WAIT_ORDERS:
        P = built[f"wait-arms-{''.join(map(str, order))}-1024x416"][1]
        st = stripe(P, 0)
        assert tuple(r.stored for r in st) == order and [r.last for r in st] == [False, False, True]
        # the rounds that follow an arm hold busy blocks: their pixels depend on the loads the arm waited for
        assert all(sum(r.counts) > 0 or r.stored == 0 for r in st[1:])
    arms = {o[i] for o in PM.WAIT_ORDERS for i in (0, 1)}  # (the last round waits for nothing)
    assert arms == {0, 1, 2, 3}


def test_alignment_plan():
    pkts, at = PM.aligned_plan(np.zeros(1001, np.uint8))
    assert len(pkts) == 8 and [a % 4 for a in at] == [0, 1, 2, 3]
    assert all(12 <= pkts[i].size <= 15 for i in range(0, 8, 2))


def test_model_classes_agree_with_the_oracles_picture(built):
    """a DC-only block decodes to 64 equal pixels — the model's own statement of the pixel —, an unchanged one leaves
    the prefill (bytes no decoded pixel can be: outside 16..235); a busy one is neither"""
    for n, (p, P) in built.items():
        q0 = int(R.oracle_tables(P.Q)[1][0])
        pic = {}
        for fill in (3, 250):
            o = np.full(P.w * P.h * 3 // 2, fill, np.uint8)
            R.OracleDecoder().decode(p, o)
            ysz, cw = P.w * P.h, P.w // 2
            pic[fill] = [o[ysz:ysz + ysz // 4].reshape(P.h // 2, cw), o[ysz + ysz // 4:].reshape(P.h // 2, cw)]
        mbw = P.w // 16
        for r in P.rounds:
            for g in r.groups:
                if not g.exists or g.gslow:
                    continue
                for l in np.nonzero(g.valid)[0]:
                    mb = g.g * S.kMbPerGroup + l % S.kMbPerGroup
                    y, x = 8 * (mb // mbw), 8 * (mb % mbw)
                    a, b = (pic[f][l // S.kMbPerGroup][y:y + 8, x:x + 8] for f in (3, 250))
                    if g.cls[l] == PM.UNCHANGED:
                        assert (a == 3).all() and (b == 250).all(), (n, g.g, l)
                    else:
                        assert np.array_equal(a, b) and 16 <= a.min() and a.max() <= 235, (n, g.g, l)
                        if g.cls[l] == PM.DC_ONLY:
                            assert (a == PM.dc_pixel(int(g.bytes[l][0]), q0)).all(), (n, g.g, l)
