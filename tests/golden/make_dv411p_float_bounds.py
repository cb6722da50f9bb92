#!/usr/bin/env python3
"""Writes tests/golden/dv411p_float_bounds.json: how far the fixed-point DV statement (oracle/dv_oracle.c, dvo_*) is
from the floating-point one (oracle/dv_float.c, dvf_*) on whole frames of DVCPRO 625/50 4:1:1 (system 3), both through
the segment moves of tests/dvsys.py — on exactly the seeded frames this module builds for tests/test_dv411p_cpu.py and
tests/test_gpu_dv411p.py.  The rule is make_dv_float_bounds.py's: deviation = oracle pixel minus
float pixel clipped to 0..255, unrounded; a bound is the measured worst case rounded up to the next 0.25 level
(absolute) or 0.01 level (mean signed deviation of a frame), with no margin; the reference is the float statement,
never the kernel, and the GPU test uses the same numbers because the kernel has to equal the oracle bit for bit.
(PARITY UNPINNED: the file says how well the fixed-point code realises the closed form in this layout, nothing about
the standard.)

The families are section 9.2's: a the oracle's encoder, b the plain encoder, on the same synthetic pictures; c the two
symbol-written frames of tests/dvfloat.py carried as the segments of a 625/50 4:1:1 frame, in both orders.
tests/dvfloat.py is hard-wired to 525/60 and 625/50 4:2:0 where it builds frames and decodes them, so those few lines
are restated here for system 3; everything else is imported from it."""
import functools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dvfloat as F  # noqa: E402
import dvsys as S  # noqa: E402

SYSTEM = S.SYS_625_50_411
BOUNDS = os.path.join(HERE, "dv411p_float_bounds.json")
STEP = {"abs": 0.25, "mean": 0.01}
# (noise amplitude, encoder flags) of the pictures: those of 625/50 4:2:0 in tests/dvfloat.py
PICTURES = [(0, 0), (4, 1), (8, 3), (16, 2), (40, 3), (90, 3)]
FAMILIES = "abc"


@functools.lru_cache(None)
def picture(amp):
    return S.synth(SYSTEM, 0, F.SEEDS["picture_seed"] + amp, amp)


COUNT = {"a": len(PICTURES), "b": len(PICTURES), "c": 2}


@functools.lru_cache(None)
def frame(family, i):
    """frame i of a family (tests/dvfloat.py: frames), for system 3"""
    if family in ("a", "b"):
        amp, flags = PICTURES[i]
        return S.encode(SYSTEM, picture(amp), flags, encode525=None if family == "a" else F.encode)
    assert family == "c"
    a, b = (F.symbol_frame(seed)[0] for seed in F.SEEDS["symbol_frames"])
    return S.pack(SYSTEM, np.concatenate([a, b] if i == 0 else [b, a]))


def float_decode_info(frame):
    """(unrounded picture, blocks outside the fixed-point range, blocks that ended in pass 1/2/3/never) of the float
    statement behind tests/dvsys.py's segment moves (tests/dvfloat.py: decode625_info)"""
    outs, fins = [], []

    def one(host):
        pic, out, fin = F.decode_info(host)
        outs.append(out)
        fins.append(fin)
        return pic
    pic = S.decode(SYSTEM, frame, decode525=one)
    return pic, sum(outs), tuple(int(x) for x in np.sum(fins, axis=0))


@functools.lru_cache(None)
def reference(family, i):
    """(frame i of a family, the oracle's picture, the float statement's picture, blocks out of range), computed once"""
    fr = frame(family, i)
    pic, n_out, _ = float_decode_info(fr)
    return fr, S.decode(SYSTEM, fr), pic, n_out


def references(family):
    return [reference(family, i) for i in range(COUNT[family])]


def bounds():
    with open(BOUNDS) as f:
        return json.load(f)


def r4(x):
    return round(float(x), 4)


def text():
    out = {"system": SYSTEM, "seeds": F.SEEDS, "pictures": PICTURES, "step": STEP,
           "measured": {"frames": {}}, "bounds": {"frames": {}}}
    for fam in FAMILIES:
        worst, mean, n_out = 0.0, 0.0, 0
        for _, got, pic, o in references(fam):
            d = F.deviation(got, pic)
            worst, mean, n_out = max(worst, float(np.abs(d).max())), max(mean, abs(float(d.mean()))), n_out + o
        assert n_out == 0, (fam, n_out)
        out["measured"]["frames"][fam] = {"abs": r4(worst), "mean": r4(mean)}
        out["bounds"]["frames"][fam] = {"abs": F.up(worst, STEP["abs"]), "mean": F.up(mean, STEP["mean"])}
    return json.dumps(out, indent=1, sort_keys=True) + "\n"


def main():
    t = text()
    with open(BOUNDS, "w") as f:
        f.write(t)
    print(t)


if __name__ == "__main__":
    main()
