"""What the three kernels of libmi_tga.so do on one MI355X: Targa packets resident in HBM to tightly packed pictures.

    python tools/bench_tga.py [--width 1920] [--height 1080] [--packets 1024] [--steps 5] [--warmup 1]
                              [--rows plain,flat,mixed,noise,worst] [--out profiles/tga/bench_tga.json]

Rows: the plain types (2 at depths 24 and 32) once each, and the run-length kinds (type 10 at depths 24 and 32, type 9 with
a 24-bit map) over four contents:
  flat    runs of 128: one header and one pixel for 128 pixels
  mixed   the greedy encoder (tests/tgaraw.py) on a synthetic picture: bars of 2 to 128 equal pixels in the upper half, noise
          in the lower
  noise   raw packets of 128
  worst   alternating run and raw packets of one pixel: a header a pixel
`--packets` packets, two distinct ones repeated, lie in one stream at odd byte offsets, each copy in memory of its own; one
mi_tga_decode_batch per step.  The times of the three kernels are read after every step (mi_tga_times: HIP events around
each launch); the medians over the steps are reported with the picture bytes written per second and the stream plus
picture bytes per second, against mi_rtj_copy_ceiling (k_copy16, read plus write, between the same two buffers) measured
next to it.  The first and the last picture and every status are checked against the statement.  There is no pass mark.
One JSON line per row on stdout; `--out` keeps them all in one file."""
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
DISTINCT = 2
KINDS = {"type2-24": (2, 24, 0), "type2-32": (2, 32, 0), "type10-24": (10, 24, 0), "type10-32": (10, 32, 0), "type9-map24": (9, 8, 24)}


def stored_pixels(content, rng, w, h, sb, mapped):
    """the stored pixels of a picture of the content, (npix, sb) uint8 (map indices below 200 for a mapped kind)"""
    npix, top = w * h, 200 if mapped else 256
    if content == "flat":
        return np.repeat(rng.integers(0, top, (-(-npix // 128), sb), dtype=np.uint8), 128, axis=0)[:npix]
    if content == "mixed":
        half = npix // 2
        lens = rng.integers(2, 129, half // 40 + 1)  # (65 on average: more than the half needs)
        bars = np.repeat(rng.integers(0, top, (lens.size, sb), dtype=np.uint8), lens, axis=0)[:half]
        return np.concatenate([bars, rng.integers(0, top, (npix - half, sb), dtype=np.uint8)])
    return rng.integers(0, top, (npix, sb), dtype=np.uint8)


def data_of(content, px, T):
    """the image data of the content over the stored pixels"""
    npix, sb = px.shape
    if content == "plain":
        return px.tobytes()
    if content == "mixed":
        return T.rle(px, T.greedy(px))
    if content == "worst":  # run, raw, run, raw, ... of one pixel each
        out = np.zeros((npix, 1 + sb), np.uint8)
        out[::2, 0] = 0x80
        out[:, 1:] = px
        return out.tobytes()
    full, rest = npix // 128, npix % 128
    head = 0xFF if content == "flat" else 0x7F
    body = px[:full * 128].reshape(full, 128, sb)
    body = body[:, 0] if content == "flat" else body.reshape(full, 128 * sb)
    out = np.concatenate([np.full((full, 1), head, np.uint8), body], axis=1).tobytes()
    if rest:
        out += T.rle(px[full * 128:], [("run" if content == "flat" else "raw", rest)])
    return out


def main():
    import tgaraw as T
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--packets", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", default="plain,flat,mixed,noise,worst")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.steps < 5:
        ap.error("--steps: a median of at least 5 launches")
    tga = importlib.import_module("gmerlin-avdecoder_amd.tga")
    P = importlib.import_module("gmerlin-avdecoder_amd")
    w, h, n = a.width, a.height, a.packets
    dev, rtj = tga.MiTga(0), P.MiRtj(0)
    lines, ok = [], True
    try:
        for content in a.rows.split(","):
            for kind, (image_type, depth, map_depth) in KINDS.items():
                if (content == "plain") != (image_type == 2):
                    continue
                fmt = T.FORMATS[(map_depth or depth) // 8 - 1]
                lay = T.layout(fmt, w, h)
                rng = np.random.default_rng(3000 + len(lines))
                packets = []
                for _ in range(DISTINCT):
                    px = stored_pixels(content, rng, w, h, depth // 8, bool(map_depth))
                    kw = dict(map_type=1, map_length=200, map_depth=map_depth, cmap=rng.integers(0, 256, 200 * map_depth // 8, dtype=np.uint8).tobytes()) if map_depth else {}
                    packets.append(T.packet(image_type, w, h, depth, data_of(content, px, T), 0x20, **kw))
                offsets, cur = np.zeros(n, np.uint64), 1
                for k in range(n):
                    offsets[k] = cur
                    cur += packets[k % DISTINCT].size + 2 * (k % 3)
                    cur += 1 - cur % 2
                lengths = np.array([packets[k % DISTINCT].size for k in range(n)], np.uint32)
                qs = tga.up16(lay.picture_bytes)
                ds, dq, dst = dev.alloc(cur + 16), dev.alloc(n * qs), dev.alloc(4 * n)
                try:
                    for k in range(n):
                        dev.h2d(ds, packets[k % DISTINCT], offset=int(offsets[k]))
                    dev.sync()
                    dev.times()
                    ms = []
                    for step in range(a.warmup + a.steps):
                        dev.decode_batch(ds, offsets, lengths, w, h, fmt, dq, qs, dst)
                        t, launches = dev.times()
                        assert launches == 3
                        if step >= a.warmup:
                            ms.append(t)
                    exact = not dev.d2h(dst, 4 * n, dtype=np.int32).any()
                    for k in (0, n - 1):
                        st, want, _ = T.decode_fast(packets[k % DISTINCT], None, (w, h, fmt))
                        exact &= st == 0 and np.array_equal(dev.d2h(dq, lay.picture_bytes, offset=k * qs), want)
                    ok &= exact
                    ceiling = min(cur, n * qs, 1 << 30) // 16 * 16
                    copy_gbs = rtj.copy_ceiling(ds, dq, ceiling)
                finally:
                    dev.free(ds), dev.free(dq), dev.free(dst)
                scan, index, expand = (statistics.median(m[i] for m in ms) for i in range(3))
                total = statistics.median(sum(m) for m in ms)
                stream_bytes, picture_bytes = int(lengths.astype(np.int64).sum()), n * lay.picture_bytes
                line = {"tool": "bench_tga", "kind": kind, "content": content, "format": fmt, "width": w, "height": h, "packets": n,
                        "steps": a.steps, "warmup": a.warmup, "tile_pixels": tga.tile_pixels(),
                        "packet_bytes": [int(p.size) for p in packets], "picture_bytes": lay.picture_bytes,
                        "ms_scan": round(scan, 4), "ms_index": round(index, 4), "ms_expand": round(expand, 4), "ms_total": round(total, 4),
                        "us_per_packet": round(total * 1e3 / n, 4),
                        "picture_gbytes_per_s": round(picture_bytes / (total / 1e3) / 1e9, 1),
                        "stream_plus_picture_gbytes_per_s": round((stream_bytes + picture_bytes) / (total / 1e3) / 1e9, 1),
                        "expand_only_picture_gbytes_per_s": round(picture_bytes / (expand / 1e3) / 1e9, 1),
                        "copy_ceiling_bytes": ceiling, "copy_ceiling_gbytes_per_s": round(copy_gbs, 1),
                        "picture_share_of_copy_ceiling": round(picture_bytes / (total / 1e3) / 1e9 / copy_gbs, 4),
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
