"""What the unpack kernels of libmi_yuv.so do on one MI355X: every codec of lib/video_yuv.c over packets resident in HBM.

    python tools/bench_yuv.py [--codecs yuv2,2vuy,...] [--width 1920] [--height 1080] [--packets 1024] [--steps 7]
                              [--warmup 2] [--out profiles/yuv/bench_yuv.json]

Per codec: `--packets` packets resident in HBM — eight distinct packets of random bytes, repeated — are one
mi_yuv_unpack_batch per step into as many tightly packed pictures (both strides the sizes rounded up to 16 bytes).  The
kernel's time is read after every step (mi_yuv_times: HIP events around the launch); the median over the steps is
reported with the bytes the launch reads plus the bytes it writes (packets and pictures, whole, counted from the layout)
per second, against 8 TB/s and against mi_rtj_copy_ceiling (k_copy16, read plus write, 1 GiB to 1 GiB between the same two
buffers) measured next to it in the same run.  The first and the last picture are checked against the statement
(tests/yuvraw.py).  There is no pass mark.  One JSON line per codec on stdout; `--out` keeps them all in one file."""
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
DISTINCT = 8
HBM_BYTES_PER_S = 8e12


def main():
    import yuvraw as Y
    ap = argparse.ArgumentParser()
    ap.add_argument("--codecs", default=",".join(Y.CODECS))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--packets", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.steps < 5:
        ap.error("--steps: a median of at least 5 launches")
    yuv = importlib.import_module("gmerlin-avdecoder_amd.yuv")
    P = importlib.import_module("gmerlin-avdecoder_amd")
    w, h, n = a.width, a.height, a.packets
    dev, rtj = yuv.MiYuv(0), P.MiRtj(0)
    lines, ok = [], True
    try:
        for name in a.codecs.split(","):
            lay = Y.layout(name, w, h)
            assert yuv.layout_of(name, w, h) == lay
            ps, qs = yuv.up16(lay.packet_bytes), yuv.up16(lay.picture_bytes)
            rng = np.random.default_rng(1000 + Y.CODECS.index(name))
            block = np.zeros((DISTINCT, ps), np.uint8)
            for i in range(DISTINCT):
                block[i, :lay.packet_bytes] = Y.random_packet(name, w, h, rng)
            dp, dq = dev.alloc(n * ps), dev.alloc(n * qs)
            try:
                for k in range(0, n, DISTINCT):
                    dev.h2d(dp, block[:min(DISTINCT, n - k)], offset=k * ps)
                dev.sync()
                dev.times()
                ms = []
                for step in range(a.warmup + a.steps):
                    dev.unpack_batch(name, w, h, dp, ps, n, dq, qs)
                    t, launches = dev.times()
                    assert launches == 1
                    if step >= a.warmup:
                        ms.append(t)
                exact = all(np.array_equal(dev.d2h(dq, lay.picture_bytes, offset=k * qs),
                                           Y.unpack(name, w, h, block[k % DISTINCT, :lay.packet_bytes])) for k in (0, n - 1))
                ok &= exact
                ceiling = min(n * ps, n * qs, 1 << 30) // 16 * 16
                copy_gbs = rtj.copy_ceiling(dp, dq, ceiling)
            finally:
                dev.free(dp)
                dev.free(dq)
            med = statistics.median(ms)
            moved = n * (lay.packet_bytes + lay.picture_bytes)
            gbs = moved / (med / 1e3) / 1e9
            line = {"tool": "bench_yuv", "codec": name, "kernel": "k_yuv_move" if name in ("2vuy", "VYUY", "yv12", "YV12", "YVU9")
                    else "k_yuv_unpack", "width": w, "height": h, "packets": n, "steps": a.steps, "warmup": a.warmup,
                    "packet_bytes": lay.packet_bytes, "picture_bytes": lay.picture_bytes,
                    "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                    "us_per_packet": round(med * 1e3 / n, 4), "bytes_read_plus_written": moved,
                    "gbytes_per_s": round(gbs, 1), "share_of_8tb_s": round(gbs * 1e9 / HBM_BYTES_PER_S, 4),
                    "copy_ceiling_gbytes_per_s": round(copy_gbs, 1), "share_of_copy_ceiling": round(gbs / copy_gbs, 4),
                    "exact_first_and_last_picture": bool(exact)}
            print(json.dumps(line), flush=True)
            lines.append(line)
    finally:
        dev.close()
        rtj.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
