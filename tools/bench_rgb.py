"""What the unpack kernels of libmi_rgb.so do on one MI355X: every codec of lib/video_qtraw.c and lib/video_aviraw.c over
packets resident in HBM, with the `2vuy` row of libmi_yuv.so (k_yuv_move) in the same run as the yardstick for the movers.

    python tools/bench_rgb.py [--codecs QT1,QT2,...,2vuy] [--width 1920] [--height 1080] [--packets 1024] [--steps 7]
                              [--warmup 2] [--out profiles/rgb/bench_rgb.json]

Per codec: `--packets` packets resident in HBM — eight distinct packets of random bytes, repeated — are one
mi_rgb_unpack_batch per step into as many tightly packed pictures (both strides the sizes rounded up to 16 bytes); the
palettised codecs get two palettes that alternate from packet to packet.  The kernel's time is read after every step
(mi_rgb_times: HIP events around the launch; the palettes' upload lies in front of them); the median over the steps is
reported with the bytes the launch reads plus the bytes it writes (packets and pictures, whole, counted from the layout)
per second, against 8 TB/s and against mi_rtj_copy_ceiling (k_copy16, read plus write, 1 GiB to 1 GiB between the same two
buffers) measured next to it in the same run.  The first and the last picture are checked against the statement
(tests/rgbraw.py; `2vuy`: tests/yuvraw.py).  There is no pass mark.  One JSON line per codec on stdout; `--out` keeps them
all in one file."""
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
YARDSTICK = "2vuy"
KERNELS = {"QT1": "k_rgb_palette<1>", "QT2": "k_rgb_palette<2>", "QT4": "k_rgb_palette<4>", "QT8": "k_rgb_palette<8>",
           "AVI8": "k_rgb_palette<8>", "QT16": "k_rgb_move<Swap16>", "MTV16": "k_rgb_move<Swap16>", "QT32": "k_rgb_move<Rot32>",
           "QT24": "k_rgb_move<None>", "AVI8_GRAY": "k_rgb_move<None>", "AVI16": "k_rgb_move<None>", "AVI24": "k_rgb_move<None>",
           "AVI32": "k_rgb_move<None>", YARDSTICK: "k_yuv_move"}


def main():
    import rgbraw as R
    import yuvraw as Y
    ap = argparse.ArgumentParser()
    ap.add_argument("--codecs", default=",".join(R.CODECS + (YARDSTICK,)))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--packets", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.steps < 5:
        ap.error("--steps: a median of at least 5 launches")
    rgb = importlib.import_module("gmerlin-avdecoder_amd.rgb")
    yuv = importlib.import_module("gmerlin-avdecoder_amd.yuv")
    P = importlib.import_module("gmerlin-avdecoder_amd")
    w, h, n = a.width, a.height, a.packets
    devs = {"rgb": rgb.MiRgb(0), "yuv": yuv.MiYuv(0)}
    rtj = P.MiRtj(0)
    lines, ok = [], True
    try:
        for name in a.codecs.split(","):
            yard = name == YARDSTICK
            S, view, dev = (Y, yuv, devs["yuv"]) if yard else (R, rgb, devs["rgb"])
            lay = S.layout(name, w, h)
            got = view.layout_of(name, w, h)
            assert (got.packet_bytes, got.picture_bytes) == (lay.packet_bytes, lay.picture_bytes)
            ps, qs = view.up16(lay.packet_bytes), view.up16(lay.picture_bytes)
            rng = np.random.default_rng(2000 + len(lines))
            block = np.zeros((DISTINCT, ps), np.uint8)
            for i in range(DISTINCT):
                block[i, :lay.packet_bytes] = S.random_packet(name, w, h, rng)
            extra, palettes = (), None
            if not yard and lay.palette_entries:
                palettes = np.stack([R.random_palette(name, rng) for _ in range(2)])
                extra = (palettes, (np.arange(n) % 2).astype(np.uint16))
            dp, dq = dev.alloc(n * ps), dev.alloc(n * qs)
            try:
                for k in range(0, n, DISTINCT):
                    dev.h2d(dp, block[:min(DISTINCT, n - k)], offset=k * ps)
                dev.sync()
                dev.times()
                ms = []
                for step in range(a.warmup + a.steps):
                    dev.unpack_batch(name, w, h, dp, ps, n, dq, qs, *extra)
                    t, launches = dev.times()
                    assert launches == 1
                    if step >= a.warmup:
                        ms.append(t)

                def want(k):
                    packet = block[k % DISTINCT, :lay.packet_bytes]
                    if yard:
                        return Y.unpack(name, w, h, packet)
                    return R.unpack(name, w, h, packet, None if palettes is None else palettes[k % 2])
                exact = all(np.array_equal(dev.d2h(dq, lay.picture_bytes, offset=k * qs), want(k)) for k in (0, n - 1))
                ok &= exact
                ceiling = min(n * ps, n * qs, 1 << 30) // 16 * 16
                copy_gbs = rtj.copy_ceiling(dp, dq, ceiling)
            finally:
                dev.free(dp)
                dev.free(dq)
            med = statistics.median(ms)
            moved = n * (lay.packet_bytes + lay.picture_bytes)
            gbs = moved / (med / 1e3) / 1e9
            line = {"tool": "bench_rgb", "codec": name, "library": "libmi_yuv.so" if yard else "libmi_rgb.so", "kernel": KERNELS[name],
                    "width": w, "height": h, "packets": n, "steps": a.steps, "warmup": a.warmup,
                    "packet_bytes": lay.packet_bytes, "picture_bytes": lay.picture_bytes,
                    "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                    "us_per_packet": round(med * 1e3 / n, 4), "bytes_read_plus_written": moved,
                    "gbytes_per_s": round(gbs, 1), "share_of_8tb_s": round(gbs * 1e9 / HBM_BYTES_PER_S, 4),
                    "copy_ceiling_bytes": ceiling, "copy_ceiling_gbytes_per_s": round(copy_gbs, 1),
                    "share_of_copy_ceiling": round(gbs / copy_gbs, 4), "exact_first_and_last_picture": bool(exact)}
            print(json.dumps(line), flush=True)
            lines.append(line)
    finally:
        for d in devs.values():
            d.close()
        rtj.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
