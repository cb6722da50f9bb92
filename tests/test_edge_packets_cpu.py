"""The builders of tests/edge_packets.py build, with the seeds of the tests they were lifted from, byte for byte the
packets those tests built while the builders were nested inside them: tests/golden/edge_packet_pins.json holds
R.digest of every such packet, recorded from the nested builders before they were lifted."""
import json
import os

import pytest

import edge_packets as E
import rtjlib as R

PINS = json.load(open(os.path.join(R.GOLDEN, "edge_packet_pins.json")))


@pytest.fixture(scope="module")
def sets():
    return E.pinned_sets()


def test_the_pins_name_every_lifted_set(sets):
    assert set(PINS) == set(sets)
    assert {k: len(v) for k, v in PINS.items()} == dict(low4x4=16, budget=6, chunks=6, dc_spellings=4, adversarial=16)


@pytest.mark.parametrize("name", sorted(PINS))
def test_lifted_builders_build_the_pinned_packets(sets, name):
    got = [R.digest(p) for p in sets[name]]
    assert len(got) == len(PINS[name])
    for i, (g, w) in enumerate(zip(got, PINS[name])):
        assert g == w, f"{name}: packet {i} is not the packet the test built before its builder was lifted"


def test_budget_packets_populate_both_sides_of_the_budget():
    """the census of the packed passes' test stays with that test (tests/test_gpu_parity.py); here the same numbers
    without a device, and what the split form's bounds on parts_listed are computed from"""
    pkts, seen, meta = E.budget_packets()
    assert seen["in"] > 1000 and seen["out"] > 300 and seen["near"] > 300, seen
    for p, m in zip(pkts, meta):
        nblk = (m["w"] // 16) * (m["h"] // 16) * 6
        assert m["sums"].size == nblk and m["beyond_low4"].size == nblk and E.packet_size(p) == (m["w"], m["h"])
        assert ((m["sums"] > m["budget"]) & m["beyond_low4"]).any()
    # stepping one token does not always reach the inside of the budget: the pinned "all_in" packets hold a few
    # blocks above it (so parts of them go to the split form's list); built strictly they hold none, and still the
    # just-inside blocks
    over = [int((m["sums"] > m["budget"]).sum()) for m in meta if m["mix"] == "all_in"]
    assert over == [12, 37], over
    _, _, smeta = E.budget_packets(mixes=((512, 32, "all_in"),), strict_in=True)
    assert len(smeta) == 2 and all((m["sums"] <= m["budget"]).all() for m in smeta)
    assert sum(int((m["budget"] - m["sums"] < m["budget"] // 50).sum()) for m in smeta) > 100
