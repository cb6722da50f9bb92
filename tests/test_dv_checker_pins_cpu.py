"""The DV test statement (tests/dvsys.py) pinned to what the three modules it replaced computed:
tests/golden/dv_checker_pins.json holds SHA-256 of their maps, synthetic pictures, encoded frames, decoded pictures and
headers for every system (tests/golden/make_dv_checker_pins.py).  The committed float bounds are measured on these
pictures and frames, so a change here is a change of the reference."""
import json
import os
import sys

from pkg import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_dv_checker_pins as M  # noqa: E402


def test_the_statement_reproduces_every_pinned_hash():
    with open(M.PINS) as f:
        want = json.load(f)
    got = M.pins()
    assert sorted(want) == ["0", "1", "3", "4", "5"] == sorted(got)
    for system, pinned in want.items():
        assert sorted(pinned) == sorted(got[system]), system
        for what, digest in pinned.items():
            assert got[system][what] == digest, (system, what)
        assert len(pinned) == {"0": 4, "3": 12}.get(system, 9), system


def test_the_maker_reproduces_the_committed_pins_byte_for_byte():
    with open(M.PINS) as f:
        assert M.text() == f.read()
