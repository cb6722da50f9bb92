#!/usr/bin/env python3
"""Writes tests/golden/yuv_ref.json: what the reference's own lib/video_yuv.c (oracle/_ref/libvideo_yuv_ref.so, built by
oracle/Makefile where the reference tree is present) makes of the three seeded packets (tests/yuvref.py) of every case of
the GPU suite's CASES.  Kept: the SHA-256 of every packet (a drifting generator is caught) and every picture — its planes
back to back, each plane's rows at its own width — as bytes where it has at most 2048 of them, else as its SHA-256.
tests/test_yuv_fixtures_cpu.py holds the file to the live reference where there is one and to the statement everywhere;
tests/test_gpu_yuv_reference.py holds the kernels to it."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import yuvref as R  # noqa: E402

if __name__ == "__main__":
    if not R.have_reference():
        sys.exit("oracle/_ref/libvideo_yuv_ref.so is not built: run make -C oracle where the reference tree is present")
    with open(R.FIXTURE, "w") as f:
        json.dump(R.ref_records(), f, indent=0, sort_keys=True)
        f.write("\n")
    print(R.FIXTURE, os.path.getsize(R.FIXTURE), "bytes")
