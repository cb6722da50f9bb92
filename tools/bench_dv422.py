"""Kernel throughput of the DV decoder for one of its five systems on one MI355X: the 50 Mbit/s 4:2:2 systems,
DVCPRO 625/50 4:1:1 and, as their yardsticks in the same session, the two older 25 Mbit/s systems.

    python tools/bench_dv422.py --system 525_422|625_422|625_411|525|625 [--frames 1024] [--steps 20] [--warmup 3] [--distinct 16]
                                [--content own|dv25]

`--frames` DIF frames resident in HBM (`--distinct` different ones, made by the checker's encoder from synthetic
pictures and tiled) are decoded into as many pictures in HBM by mi_dv_decode_batch_sys, once per step.  The time is the
HIP-event time of the kernel launches (mi_dv_kernel_times).  Prints one JSON line: frames/s, ms per launch, GB/s where
the bytes are the frames read plus the pictures written, the fraction of 8 TB/s, and a bit-exact check of every
distinct frame against the checker (tests/dvsys.py; for 525/60 that is oracle/dv_oracle.c itself).
PARITY UNPINNED.  The method and the line are tools/bench_dv625.py's, plus the video segments per frame and the time per
segment: a 4:2:2 frame has twice the segments of the 25 Mbit/s frame of its line system, the same parse per segment and
fewer transforms and stores, so it is compared with that system per segment, in one session.  The checker's encoder
spends a segment's bits on four blocks per macroblock instead of six, so its 4:2:2 frames hold more code words per
segment, and more of them in the space areas 1 and 3 leave (pass 2, where one lane per macroblock works).
`--content dv25` (4:2:2 systems only) takes that difference out: the frames' segments are those of the 525/60 bench's
frames, byte for byte (areas 1 and 3 then hold ordinary blocks, which the decoder parses and drops), so the parse per
segment IS the yardstick's.  625/50 4:1:1 (`--system 625_411`) takes both contents too: its own is the checker's encoder
on tests/dvsys.py's pictures, `dv25` the 525/60 bench's segments byte for byte (324 of two such frames); its store forms
are 525/60's, so with that content the time per segment is to be compared with the 525/60 yardstick's."""
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
    ap.add_argument("--system", choices=["525_422", "625_422", "625_411", "525", "625"], default="525_422")
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--content", choices=["own", "dv25"], default="own")
    a = ap.parse_args()
    dv = importlib.import_module("gmerlin-avdecoder_amd.dv")
    import dvlib as D
    import dvsys as S
    system = {"525": dv.SYS_525_60, "625": dv.SYS_625_50, "625_411": dv.SYS_625_50_411, "525_422": dv.SYS_525_60_422, "625_422": dv.SYS_625_50_422}[a.system]
    segments = S.geometry(system).segments
    fb, pb, _ = dv.geometry(system)
    n, k = a.frames, max(1, min(a.distinct, a.frames))
    if a.content == "dv25" and system not in (dv.SYS_525_60_422, dv.SYS_625_50_422, dv.SYS_625_50_411):
        ap.error("--content dv25 is for the 4:2:2 systems and 625/50 4:1:1")
    if a.content == "dv25":
        hosts = S.geometry(system).hosts
        distinct = [S.pack(system, np.concatenate([D.encode(D.synth(hosts * i + h, 7, 2 + 3 * (i % 12)), 3) for h in range(hosts)]))
                    for i in range(k)]
    else:
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
    print(json.dumps({"tool": "bench_dv422", "system": a.system, "content": a.content, "frames": n, "steps": launches, "warmup": a.warmup,
                      "ms_per_launch": round(per, 4), "frames_per_s": round(n / (per * 1e-3), 1), "gb_per_s": round(gbs, 1),
                      "hbm_fraction": round(gbs / HBM_PEAK_GBS, 4), "bytes_per_launch": n * (fb + pb),
                      "segments_per_frame": segments, "ns_per_segment": round(per * 1e6 / (n * segments), 4),
                      "distinct_frames": k, "bit_exact": exact, "parity": "unpinned"}))
    return 0 if exact else 1


if __name__ == "__main__":
    sys.exit(main())
