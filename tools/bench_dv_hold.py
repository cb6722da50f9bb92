"""What holding flagged macroblocks costs on one MI355X: the hold pass of mi_dv_decode_batch_held (k_dv_hold_mask,
k_dv_hold_carry, k_dv_hold_copy) next to k_dv_decode of the same launches.

    python tools/bench_dv_hold.py [--systems 525,625_422] [--frames 1024] [--shares 0,0.01,0.1] [--steps 7] [--warmup 2]
                                  [--out profiles/dv_hold/bench_dv_hold.json]

Per system and share: `--frames` DIF frames resident in HBM — four encoded ones (the checker's encoder on synthetic
pictures) repeated, each copy with its own STA nibbles: the share of its macroblocks carries an error nibble (0111 or
1111) at seeded random places, the rest any of the 14 other values — are one run of one stream without a picture
before it.  Every step is one mi_dv_decode_batch_held; its two HIP-event times are read after it (mi_dv_kernel_times:
k_dv_decode, unchanged by the hold pass and so the yardstick; mi_dv_hold_times: the three hold kernels), and the
medians over the steps are reported, with the hold pass as a fraction of the decode, the macroblocks copied, and a
bit-exact check of the first eight pictures against the test statement (tests/dvhold.py).  One JSON line per case on
stdout; `--out` keeps them all in one file.  PARITY UNPINNED."""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", default="525,625_422")
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--shares", default="0,0.01,0.1")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.steps < 5:
        ap.error("--steps: a median of at least 5 launches")
    dv = importlib.import_module("gmerlin-avdecoder_amd.dv")
    import dvhold as H
    import dvsys as S
    names = {"525": dv.SYS_525_60, "625": dv.SYS_625_50, "625_411": dv.SYS_625_50_411, "525_422": dv.SYS_525_60_422,
             "625_422": dv.SYS_625_50_422}
    dev = dv.MiDv(0)
    lines, ok = [], True
    try:
        for name in a.systems.split(","):
            system = names[name]
            fb, pb, _ = dv.geometry(system)
            nmb = S.geometry(system).macroblocks
            distinct = [S.encode(system, S.synth(system, i, 7, 4 + 3 * i), 3) for i in range(4)]
            n = a.frames
            df, dp = dev.alloc(n * fb), dev.alloc(n * pb)
            try:
                for share in [float(s) for s in a.shares.split(",")]:
                    rng = np.random.default_rng(int(share * 1000) + system)
                    frames = np.stack([H.stamp(system, distinct[k % 4], H.nibbles(system, rng, rng.random(nmb) < share))
                                       for k in range(n)])
                    flagged = sum(dv.held_macroblocks(f, system) for f in frames)
                    dev.h2d(df, frames)
                    for _ in range(a.warmup):
                        dev.decode_batch_held(system, df, n, dp)
                    dev.sync()
                    dev.kernel_times(), dev.hold_times()  # forget the warm-up launches
                    dec, hold = [], []
                    for _ in range(a.steps):
                        dev.decode_batch_held(system, df, n, dp)
                        dec.append(dev.kernel_times()[0])
                        hold.append(dev.hold_times()[0])
                    held = dev.hold_stats()
                    k = min(8, n)
                    want, _ = H.hold(system, frames[:k])
                    exact = bool(np.array_equal(dev.d2h(dp, k * pb).reshape(k, pb), want))
                    ok &= exact
                    d, h = statistics.median(dec), statistics.median(hold)
                    line = {"tool": "bench_dv_hold", "system": name, "frames": n, "share_flagged": share, "steps": a.steps,
                            "warmup": a.warmup, "macroblocks_flagged": int(flagged), "macroblocks_copied": int(held),
                            "decode_ms_median": round(d, 4), "decode_ms_min": round(min(dec), 4), "decode_ms_max": round(max(dec), 4),
                            "hold_ms_median": round(h, 4), "hold_ms_min": round(min(hold), 4), "hold_ms_max": round(max(hold), 4),
                            "hold_over_decode": round(h / d, 4), "bit_exact_first_pictures": exact, "parity": "unpinned"}
                    print(json.dumps(line), flush=True)
                    lines.append(line)
            finally:
                dev.free(df)
                dev.free(dp)
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
