"""What the DV encoder does on one MI355X: frames per second of k_dv_encode for pictures resident in HBM, next to the
scalar encoder of the test suite on one core.

    python tools/bench_dv_encode.py [--systems 525,625,625_411,525_422,625_422] [--pictures 1024] [--noise 0,8,32]
                                    [--steps 7] [--warmup 2] [--cpu-pictures 2] [--out profiles/dv_encode/bench_dv_encode.json]

Per system and noise amplitude: `--pictures` pictures resident in HBM — eight distinct dvsys.synth pictures repeated — are
one mi_dv_encode_batch per step.  The kernel's time is read after every step (mi_dv_encode_times: HIP events around the
launch) and the median over the steps is reported as frames per second, with the chosen-qno histogram and the dropped
levels of the last step (mi_dv_encode_stats), a byte-exact check of the first frame against the statement
(tests/dvenc.py), and the frames per second of dvo_encode_frame (through tests/dvsys.py for the systems it carries) on one
core for the first `--cpu-pictures` of the same pictures.  There is no pass mark.  One JSON line per case on stdout; `--out`
keeps them all in one file.  PARITY UNPINNED."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
DISTINCT = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", default="525,625,625_411,525_422,625_422")
    ap.add_argument("--pictures", type=int, default=1024)
    ap.add_argument("--noise", default="0,8,32")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cpu-pictures", type=int, default=2)
    ap.add_argument("--flags", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.steps < 5:
        ap.error("--steps: a median of at least 5 launches")
    dv = importlib.import_module("gmerlin-avdecoder_amd.dv")
    import dvenc as E
    import dvsys as S
    names = {"525": dv.SYS_525_60, "625": dv.SYS_625_50, "625_411": dv.SYS_625_50_411, "525_422": dv.SYS_525_60_422,
             "625_422": dv.SYS_625_50_422}
    dev = dv.MiDv(0)
    lines, ok = [], True
    try:
        for name in a.systems.split(","):
            system = names[name]
            fb, pb, _ = dv.geometry(system)
            n = a.pictures
            dp, df = dev.alloc(n * pb), dev.alloc(n * fb)
            try:
                for amp in [int(s) for s in a.noise.split(",")]:
                    distinct = np.stack([S.synth(system, i, 11, amp) for i in range(DISTINCT)])
                    for k in range(0, n, DISTINCT):
                        dev.h2d(dp, distinct[:min(DISTINCT, n - k)], offset=k * pb)
                    for _ in range(a.warmup):
                        dev.encode_batch(system, dp, n, df, a.flags)
                    dev.sync()
                    dev.encode_times()  # forget the warm-up launches
                    ms = []
                    for _ in range(a.steps):
                        dev.encode_batch(system, dp, n, df, a.flags)
                        ms.append(dev.encode_times()[0])
                    hist, dropped = dev.encode_stats()
                    exact = bool(np.array_equal(dev.d2h(df, fb), E.encode(system, distinct[0], a.flags)))
                    ok &= exact
                    t0 = time.perf_counter()
                    for i in range(a.cpu_pictures):
                        S.encode(system, distinct[i % DISTINCT], a.flags)
                    cpu = (time.perf_counter() - t0) / max(a.cpu_pictures, 1)
                    m = statistics.median(ms)
                    line = {"tool": "bench_dv_encode", "system": name, "pictures": n, "noise": amp, "flags": a.flags,
                            "steps": a.steps, "warmup": a.warmup, "encode_ms_median": round(m, 4), "encode_ms_min": round(min(ms), 4),
                            "encode_ms_max": round(max(ms), 4), "frames_per_s": round(n / (m / 1e3), 1),
                            "mbytes_per_s_out": round(n * fb / (m / 1e3) / 1e6, 1),
                            "cpu_one_core_frames_per_s": round(1.0 / cpu, 2) if a.cpu_pictures else None,
                            "qno_hist": [int(x) for x in hist], "levels_dropped": int(dropped), "byte_exact_first_frame": exact,
                            "parity": "unpinned"}
                    print(json.dumps(line), flush=True)
                    lines.append(line)
            finally:
                dev.free(dp)
                dev.free(df)
    finally:
        dev.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
