"""Kernel throughput of the DV25 decoder for one system on one MI355X, 625/50 (IEC 4:2:0) or 525/60.

    python tools/bench_dv625.py --system 625|525 [--frames 1024] [--steps 20] [--warmup 3] [--distinct 16]

`--frames` DIF frames resident in HBM (`--distinct` different ones, made by the checker's encoder from synthetic
pictures and tiled) are decoded into as many pictures in HBM by mi_dv_decode_batch_sys, once per step.  The time is the
HIP-event time of the kernel launches (mi_dv_kernel_times).  Prints one JSON line: frames/s, ms per launch, GB/s where
the bytes are the frames read plus the pictures written, the fraction of 8 TB/s, and a bit-exact check of every
distinct frame against the checker (tests/dvsys.py; for 525/60 that is oracle/dv_oracle.c itself).  PARITY UNPINNED.
Run both systems in one session to compare them per block (a 625/50 frame has 1.2 x the blocks of a 525/60 one)."""
import argparse
import hashlib
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--system", choices=["625", "525"], default="625")
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=16)
    a = ap.parse_args()
    dv = importlib.import_module("gmerlin-avdecoder_amd.dv")
    import dvsys as S
    system = dv.SYS_625_50 if a.system == "625" else dv.SYS_525_60
    fb, pb, _ = dv.geometry(system)
    n, k = a.frames, max(1, min(a.distinct, a.frames))
    distinct = [S.encode(system, S.synth(system, i, 7, 2 + 3 * (i % 12)), 3) for i in range(k)]
    want = [hashlib.sha256(S.decode(system, f).tobytes()).hexdigest() for f in distinct]
    frames = np.stack([distinct[i % k] for i in range(n)])
    dev = dv.MiDv(0)
    df, dp = dev.alloc(n * fb), dev.alloc(n * pb)
    try:
        dev.h2d(df, frames)
        for _ in range(a.warmup):
            dev.decode_batch_sys(system, df, n, dp)
        dev.sync()
        dev.kernel_times()  # forget the warm-up launches
        for _ in range(a.steps):
            dev.decode_batch_sys(system, df, n, dp)
        ms, launches = dev.kernel_times()
        got = dev.d2h(dp, k * pb).reshape(k, pb)
        exact = all(hashlib.sha256(got[i].tobytes()).hexdigest() == want[i] for i in range(k))
    finally:
        dev.free(df)
        dev.free(dp)
        dev.close()
    per = ms / launches
    gbs = n * (fb + pb) / (per * 1e-3) / 1e9
    print(json.dumps({"tool": "bench_dv625", "system": a.system, "frames": n, "steps": launches, "warmup": a.warmup,
                      "ms_per_launch": round(per, 4), "frames_per_s": round(n / (per * 1e-3), 1), "gb_per_s": round(gbs, 1),
                      "hbm_fraction": round(gbs / HBM_PEAK_GBS, 4), "bytes_per_launch": n * (fb + pb),
                      "distinct_frames": k, "bit_exact": exact, "parity": "unpinned"}))
    return 0 if exact else 1


if __name__ == "__main__":
    sys.exit(main())
