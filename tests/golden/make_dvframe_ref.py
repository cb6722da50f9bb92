#!/usr/bin/env python3
"""Writes tests/golden/dvframe_ref.json: what the reference's own lib/dvframe.c (oracle/_ref/libdvframe_ref.so, built by
oracle/Makefile where the reference tree is present) answers for the seeded frames of tests/dvref.py that the device
launches of tests/test_gpu_dv_reference.py use — per system the 16 sound frames into 1, 2 and 4 pairs and the 9 metadata
frames.  Kept: the SHA-256 of every input frame (a drifting generator is caught), dv_extract_audio's return values and the
15 metadata ints of every frame in clear, the SHA-256 of every frame's PCM (pairs x 8192 bytes, written into zeroed
buffers), and the PCM itself of one 16-bit and one 12-bit 525/60 frame.  tests/test_dvframe_fixtures_cpu.py holds the
file to the live reference where there is one, and to the host reader and the statements everywhere."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dvref as R  # noqa: E402

if __name__ == "__main__":
    if not R.have_reference():
        sys.exit("oracle/_ref/libdvframe_ref.so is not built: run make -C oracle where the reference tree is present")
    with open(R.FIXTURE, "w") as f:
        json.dump(R.ref_records(), f, indent=0, sort_keys=True)
        f.write("\n")
    print(R.FIXTURE, os.path.getsize(R.FIXTURE), "bytes")
