"""mi_rtj_encode_bound and mi_rtj_encode_bound_fmt (pure host code: the library loads without a device) against
tests/golden/rtj_format_pins.json, which was written from the per-format arithmetic the format table replaced
(tests/golden/make_rtj_format_pins.py).  The refusals of the same file need a device: tests/test_gpu_rtj420_encode.py."""
import json
import os
import sys

from pkg import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_rtj_format_pins as M  # noqa: E402


def test_encode_bounds_are_the_pinned_ones():
    with open(M.PINS) as f:
        want = json.load(f)["bound"]
    got = M.bounds()
    grid = len(M.SIZES) ** 2 * len(M.COUNTS) * len(M.ALIGNS)
    assert len(want["plain"]) == grid and len(want["fmt"]) == grid * len(M.FMTS)
    for key in ("plain", "fmt"):
        assert len(got[key]) == len(want[key])
        for a, b in zip(want[key], got[key]):
            assert a == b, (key, a, b)
    # the grid holds sizes that are no multiple of a macroblock, unknown formats, and real pictures
    assert [1, 1920, 1088, 1, 64, 12 + 64 * 4 * 120 * 136 + 52 + 64] in want["fmt"]
    assert all(r[-1] == 0 for r in want["fmt"] if r[0] in (-1, 3))
