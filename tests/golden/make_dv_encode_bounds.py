#!/usr/bin/env python3
"""Writes tests/golden/dv_encode_bounds.json: what the integer statement of the DV encoder (tests/dvenc.py) measures on the
pictures of tests/dvenc_check.py.  Nothing here is a tolerance somebody chose:
  deviation   per picture and flags, the largest |level - F W / 2^s| (numpy double orthonormal transform, dvf_weight,
              dvf_shift), rounded up to 0.01.  The test's condition is "below 1" whatever this file says; the figure
              pinned here is what the arithmetic actually reaches.
  psnr        per picture, the oracle decoder's PSNR of the statement's, the oracle encoder's and the float encoder's frame,
              and the statement's shortfall against the lower of the other two, rounded up to 0.1 dB (0.0: none).
  systems     the same for one picture of each of the other four systems through tests/dvsys.py."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dvenc_check as K  # noqa: E402
import dvfloat as F  # noqa: E402
import dvsys as S  # noqa: E402


def psnr_entry(p):
    return {"statement": round(p[0], 3), "oracle": round(p[1], 3), "float": round(p[2], 3), "shortfall": K.shortfall(p)}


def main():
    out = {"step": {"deviation": K.STEP_DEVIATION, "db": K.STEP_DB},
           "deviation": {f"{name}/{flags}": F.up(K.deviation(name, flags), K.STEP_DEVIATION) for name, flags in K.FRAMES},
           "psnr": {name: psnr_entry(K.psnr_525(name)) for name in K.NAMES},
           "systems": {str(s): psnr_entry(K.psnr_system(s)) for s in S.SYSTEMS if s != S.SYS_525_60}}
    with open(K.BOUNDS, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
