"""The edge pictures of tests/dvenc_edges.py do what they claim, without a GPU: the statement's census of them in all five
systems is the recorded one (tests/golden/dv_encode_edges.json, make_dv_encode_edges.py) and meets the conditions the
entries were built for; the two claims of the kernel's header about its 24-bit multiplier hold on them; the independent
checks of test_dv_encode_cpu.py hold on the 525/60 edge frames; and a statement with one rule swapped encodes the entry
named for that rule differently, while the four older pictures (dvenc.PICTURES) let most of those swaps through.

Statement frames take a few seconds of numpy each and are made once a process (dvenc_edges.stated).  PARITY UNPINNED."""
import numpy as np
import pytest

import dvenc as E
import dvenc_check as K
import dvenc_edges as X
import dvfloat as F
import dvsys as S

CASES = [(system, flags) for system in S.SYSTEMS for flags in range(4)]


def test_the_list():
    names, segs = X.segments()
    assert list(names) == X.fixture()["entries"] and len(names) % 2 == 1
    carrying = np.zeros(30, bool)
    carrying[X.SLOTS] = True
    for name, seg in zip(names, segs):
        if name not in ("ties", "drops"):
            assert (seg[~carrying] == 128).all(), name  # the same segment in the 4:2:2 systems
    for system in S.SYSTEMS:  # every entry occurs, with its successor and with its predecessor as wave partner
        at = X.entry_of(system).reshape(-1, 2)
        L = len(names)
        assert {(int(a), int(b)) for a, b in at} == {(i, (i + 1) % L) for i in range(L)}
        back = X.entry_of(system, True).reshape(-1, 2)  # and backwards every wave has the other order
        assert {(int(a), int(b)) for a, b in back} == {((i + 1) % L, i) for i in range(L)}


def test_the_extremal_blocks_are_the_sign_patterns_of_the_basis():
    """a coefficient is linear in the pixels, so the 0 / 255 sign pattern of its basis function is the picture that drives
    it furthest: no other pattern of the list gives a position more than the position's own.  And the flat blocks' DC is
    -256 and 254: the upper DC clip cannot be reached"""
    ext = X.extremal_blocks()
    for mode in (0, 1):
        c = np.abs(E.transform(ext[:126], np.full(126, mode)))[:, 1:]  # [pattern][position]
        own = c[63 * mode + np.arange(63), np.arange(63)]
        assert np.array_equal(own, c.max(axis=0))
    r = E.encode_blocks(X.with_blocks(ext[126:], X.SLOTS[[0, 5]]), 0)
    assert r["dc"][X.SLOTS[[0, 5]]].tolist() == [-256, 254]


@pytest.mark.parametrize("system,flags", CASES)
def test_the_census_is_the_recorded_one_and_meets_its_conditions(system, flags):
    fr, rec, cen, arr = X.stated(system, flags)
    print(f"system {system} flags {flags}: {cen}")
    assert cen == X.fixture()["census"][f"{system}/{flags}"]
    # the kernel header's two claims, on extremal input
    assert cen["mul_operand_bits"] <= 23 and cen["P_bits"] <= 31
    # the conditions
    if not flags & 2:
        assert cen["clipped"] > 0 and cen["largest_amplitude"] == 255
    else:
        assert cen["clipped"] == 0  # class 3 halves the levels: the census does not pretend otherwise
    if flags == 3:
        assert all(n > 0 for n in cen["qno"]), cen["qno"]
    at64, at65 = arr["d1"] == 2 * arr["d2"] + 64, arr["d1"] == 2 * arr["d2"] + 65
    assert at64.any() and at65.any()
    assert not rec["mode"][at64].any() and (rec["mode"][at65] == (flags & 1)).all()
    for t, cls in zip(X.CLASS_TARGETS, (0, 1, 1, 2, 2, 3)):
        assert cen["big_at"][str(t)] > 0
        assert (rec["cls"][arr["big"] == t] == (cls if flags & 2 else 0)).all()
    assert cen["fit_exactly"] > 0 and cen["next_one_over"] > 0
    if not flags & 1:
        assert cen["runs_of_62"] > 0 and cen["longest_run"] == 62 and cen["longest_word"] == 29
    assert cen["waves_dropping_then_15"] > 0 and cen["waves_15_then_dropping"] > 0
    assert cen["waves_15_then_0"] > 0 and cen["waves_0_then_15"] > 0
    assert 0 < cen["most_dropped_in_a_segment"] < 30 * 63  # the kernel's loop bound
    assert arr["total"].max() <= E.SEGMENT_AC_BITS
    assert ((arr["next"] > E.SEGMENT_AC_BITS) | (rec["qno"] == 15)).all()


@pytest.mark.parametrize("system,flags", CASES)
def test_every_step_of_the_overflow_rule_on_ties_is_a_tie(system, flags):
    """before the rule runs, the blocks of `ties` that carry pixels (all 30; 20 in the 4:2:2 systems) need the same bits"""
    fr, rec, cen, arr = X.stated(system, flags)
    g = S.geometry(system)
    px = X.blocks_of(system, X.picture(system))
    for s in X.where(system, "ties")[:2]:
        blocks = px[30 * s:30 * s + 30]
        mode = E.choose_mode(blocks, flags)
        P, neg = E.products(E.transform(blocks, mode), mode)
        bits = E.block_bits(E.quantise(P, neg, E.choose_class(P, flags), 0))
        shown = np.array([j in g.shown for j in range(6)] * 5)
        assert len(set(bits[shown].tolist())) == 1 and shown.sum() == 5 * len(g.shown)
        assert bits.sum() > E.SEGMENT_AC_BITS and rec["qno"][s] == 0 and rec["dropped"][s] > 0
        left = E.block_bits(rec["levels"][30 * s:30 * s + 30].astype(np.int64))[shown]
        assert left.max() - left.min() <= 29  # round robin: no block is ever two words ahead of another


# ---- the independent checks of test_dv_encode_cpu.py, on the 525/60 edge frames ----
@pytest.mark.parametrize("flags", range(4))
def test_the_float_statement_reads_and_rewrites_the_edge_frame(flags):
    fr, rec, _, _ = X.stated(S.SYS_525_60, flags)
    qno, dc, mode, cls, levels = F.parse(fr)
    assert np.array_equal(F.write_frame(qno, dc, mode, cls, levels), fr)
    assert np.array_equal(qno, np.repeat(rec["qno"], 5))
    assert np.array_equal(dc, rec["dc"]) and np.array_equal(mode, rec["mode"]) and np.array_equal(cls, rec["cls"])
    assert np.array_equal(levels[:, 1:], rec["levels"][:, 1:])
    bits = np.array([F.block_bits(lv) for lv in levels])
    assert np.array_equal(bits, E.block_bits(rec["levels"].astype(np.int64)))
    assert bits.reshape(-1, 30).sum(axis=1).max() <= E.SEGMENT_AC_BITS


@pytest.mark.parametrize("flags", range(4))
def test_an_unclipped_level_of_the_edge_frame_is_never_a_whole_step_off_the_closed_form(flags):
    worst = K.deviation("edges", flags)
    print(f"edges/{flags}: worst |level - F W / 2^s| = {worst:.4f}")
    assert worst < 1.0
    assert worst <= X.fixture()["deviation"][str(flags)]


# ---- sensitivity ----
@pytest.mark.parametrize("name", X.VARIANTS)
def test_a_swapped_rule_changes_the_entry_named_for_it(name):
    names, segs = X.segments()
    for flags in X.VARIANTS[name][2]:
        seg = segs[names.index(X.named_for(name, flags))]
        plain = E.segment(seg, flags)
        with X.variant(name):
            swapped = E.segment(seg, flags)
        assert np.array_equal(plain, E.segment(seg, flags)), "the hooks are back in place"
        assert not np.array_equal(plain, swapped), (name, flags)


@pytest.fixture(scope="module")
def old_records():
    return X.old_records()


@pytest.mark.parametrize("name", X.VARIANTS)
def test_what_the_four_older_pictures_make_of_a_swapped_rule(name, old_records):
    """THE ASYMMETRY: the pictures of dvenc.PICTURES (525/60, flags 0 and 3; the records determine the frames) are encoded
    the same under the swapped fit comparison, mode rule and shift row, and under the removed clip.  The swapped tie-break
    they do notice, where noise overflows (noise 64 and the drop-rule picture: accidental ties), and the moved class limits too.  Which
    picture notices what is recorded in the fixture"""
    with X.variant(name):
        noticed = X.noticed_by(old_records, X.old_records())
    print(f"{name}: noticed by {noticed or 'none of the older pictures'}")
    assert noticed == X.fixture()["old_pictures_notice"][name]
    if name in X.OLD_PICTURES_MUST_NOT_NOTICE:
        assert not noticed
