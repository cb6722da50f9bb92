#!/usr/bin/env python3
"""Writes tests/golden/dv_checker_pins.json: SHA-256 of what the DV test statement (tests/dvsys.py) computes for each of
the five systems — the four arrays of maps(), one synthetic picture, its encoded frame, that frame's picture, the picture
of seeded arbitrary bytes, header() on an empty frame; for 625/50 4:1:1 also the two regional pictures and a frame that
announces APT 5.  System 0 is the oracle itself and has no maps and no header of the statement's.  The file was first
written from the three modules tests/dvsys.py replaced (dv625.py, dv422.py, dv411p.py), so it pins the statement to
them; the float bounds under tests/golden/ are measured on these pictures and frames.  (An array is hashed behind its
dtype and shape.)"""
import functools
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dvsys as S  # noqa: E402

PINS = os.path.join(HERE, "dv_checker_pins.json")


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256((a.dtype.str + str(a.shape)).encode() + a.tobytes()).hexdigest()


@functools.lru_cache(None)
def pins():
    out = {}
    for s in S.SYSTEMS:
        g, r = S.geometry(s), {}
        pic = S.synth(s, 1, 2, 6)
        frame = S.encode(s, pic, 3)
        r["synth"], r["encode"], r["decode"] = sha(pic), sha(frame), sha(S.decode(s, frame))
        r["decode_random"] = sha(S.decode(s, np.random.default_rng(8 + s).integers(0, 256, g.frame_bytes, dtype=np.uint8)))
        if s != S.SYS_525_60:
            r.update({"maps_%d" % i: sha(a) for i, a in enumerate(S.maps(s))})
            r["header_zero"] = sha(S.header(s, np.zeros(g.frame_bytes, np.uint8)))
        if s == S.SYS_625_50_411:
            r["synth_bottom"], r["synth_right"] = sha(S.synth(s, 1, 2, 6, region="bottom")), sha(S.synth(s, 1, 2, 6, region="right"))
            r["encode_apt5"] = sha(S.encode(s, pic, 3, apt=5))
        out[str(s)] = r
    return out


def text():
    return json.dumps(pins(), indent=1, sort_keys=True) + "\n"


def main():
    with open(PINS, "w") as f:
        f.write(text())
    print(text())


if __name__ == "__main__":
    main()
