"""Throughput of plans with runs (mi_rtj_plan_set_runs) on one MI355X, next to an intra-only plan and a session.

    python tools/bench_runs.py [--frames 1024] [--steps 10] [--warmup 2] [--key-rate 255] [--lmask 4] [--cmask 4]
                               [--out profiles/runs/bench_runs.json]

A 1080p stream of --frames pictures is made on the device by mi_rtj_encode_stream (key_rate / lmask / cmask as
RTjpeg_set_intra) from synthetic content: a static gradient background, a 256x256 square that moves 8 pixels per
picture and a 192x192 patch of fresh noise in every picture.  The share of unchanged blocks is read from the plan's
block index and printed.  Three cases, each a number of pictures per second from wall time over --steps launches:
  runs     the stream through one plan cut into one run (one launch per step: the transform, then phase 2)
  intra    the same pictures encoded intra-only (key_rate 0) through a plain plan
  session  the stream through a pipelined session (mi_rtj_pipe_*, host packets in, host pictures out)
Phase 2's device time (mi_rtj_plan_run_times) and its copy rate (128 bytes per copied block: 64 read, 64 written)
are printed next to mi_rtj_copy_ceiling, with the per-kernel times of both plans.  Prints one JSON line."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def content(w, h, n, seed=7):
    """Yield n pictures (contiguous Y, U, V) of the synthetic scene."""
    yy, xx = np.mgrid[0:h, 0:w]
    bg_y = ((xx * 255) // w // 2 + (yy * 255) // h // 2).astype(np.uint8)
    cy, cx = np.mgrid[0:h // 2, 0:w // 2]
    bg_u = ((cx * 255) // (w // 2)).astype(np.uint8)
    bg_v = ((cy * 255) // (h // 2)).astype(np.uint8)
    rng = np.random.default_rng(seed)
    for i in range(n):
        y, u, v = bg_y.copy(), bg_u.copy(), bg_v.copy()
        x0, y0 = (64 + 8 * i) % (w - 256), 400
        y[y0:y0 + 256, x0:x0 + 256] = 235 - (yy[:256, :256] % 64)
        u[y0 // 2:y0 // 2 + 128, x0 // 2:x0 // 2 + 128] = 90
        v[y0 // 2:y0 // 2 + 128, x0 // 2:x0 // 2 + 128] = 200
        y[96:288, 1536:1728] = rng.integers(0, 256, (192, 192), dtype=np.uint8)
        yield np.concatenate([y.ravel(), u.ravel(), v.ravel()])


def timed(fn, steps, warmup, sync):
    for _ in range(warmup):
        fn()
    sync()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    sync()
    return (time.perf_counter() - t) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quality", type=int, default=200)
    ap.add_argument("--key-rate", type=int, default=255)
    ap.add_argument("--lmask", type=int, default=4)
    ap.add_argument("--cmask", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    P = importlib.import_module("gmerlin-avdecoder_amd")
    dev = P.MiRtj()
    w, h, n, Q = 1920, 1088, a.frames, a.quality
    fsz = w * h * 3 // 2
    d_fr = dev.alloc(fsz * n)
    for i, pic in enumerate(content(w, h, n)):
        dev.h2d(d_fr, pic, offset=i * fsz)
    d_inter, po_i, pl_i = dev.encode(w, h, Q, n, d_fr, align=64, key_rate=a.key_rate, lmask=a.lmask, cmask=a.cmask)
    d_intra, po_k, pl_k = dev.encode(w, h, Q, n, d_fr, align=64)
    dev.sync()
    dev.free(d_fr)
    oo = np.arange(n, dtype=np.uint64) * fsz
    d_out = dev.alloc(fsz * n)
    dev.memset(d_out, 0, fsz * n)
    res = {"tool": "bench_runs", "w": w, "h": h, "frames": n, "quality": Q, "key_rate": a.key_rate, "lmask": a.lmask,
           "cmask": a.cmask, "steps": a.steps}

    def plan_of(d_st, po, pl):
        hdrs = np.stack([dev.d2h(d_st, 12, offset=int(po[j])) for j in range(n)])
        return dev.plan(hdrs, po, pl, oo)

    # ---- runs: the stream as one run ----
    pr = plan_of(d_inter, po_i, pl_i)
    pr.set_runs([n])
    pr.decode(d_inter, d_out)
    dev.sync()
    idx = pr.read_index().astype(np.int64)
    nb = pr.info()["blocks"]
    per = nb // n
    lens = np.diff(idx.reshape(n, per + 1), axis=1)
    res["unchanged_share"] = round(float((lens == 1).mean()), 4)
    res["copied_blocks"] = pr.run_copied()
    res["stream_bytes_runs"] = int(pl_i.sum())
    res["stream_bytes_intra"] = int(pl_k.sum())
    t = timed(lambda: pr.decode(d_inter, d_out), a.steps, a.warmup, dev.sync)
    res["runs_pictures_per_s"] = round(n / t)
    res["runs_ms_per_launch"] = round(t * 1e3, 3)
    pr.profile(True)
    for _ in range(a.steps):
        pr.decode(d_inter, d_out)
    dev.sync()
    kt, launches = pr.times()
    ms2, l2 = pr.run_times()
    steps = pr.step_times()
    pr.profile(False)
    res["runs_kernel_ms"] = {k: round(v / launches, 4) for k, v in kt.items() if v}
    res["phase2_ms"] = round(ms2 / max(l2, 1), 4)
    res["runs_device_ms"] = round(float(np.median(steps)), 4)
    res["phase2_copy_gbs"] = round(res["copied_blocks"] * 128 / (res["phase2_ms"] * 1e-3) / 1e9, 1)
    res["phase2_index_gbs"] = round(nb * 4 / (res["phase2_ms"] * 1e-3) / 1e9, 1)
    pr.close()
    # ---- intra: the same pictures, intra-only, plain plan ----
    pk = plan_of(d_intra, po_k, pl_k)
    pk.decode(d_intra, d_out)
    t = timed(lambda: pk.decode(d_intra, d_out), a.steps, a.warmup, dev.sync)
    res["intra_pictures_per_s"] = round(n / t)
    res["intra_ms_per_launch"] = round(t * 1e3, 3)
    pk.profile(True)
    for _ in range(a.steps):
        pk.decode(d_intra, d_out)
    dev.sync()
    kt, launches = pk.times()
    res["intra_kernel_ms"] = {k: round(v / launches, 4) for k, v in kt.items() if v}
    res["intra_device_ms"] = round(float(np.median(pk.step_times())), 4)
    pk.profile(False)
    pk.close()
    # ---- session: the stream, host packets in order ----
    pkts = [dev.d2h(d_inter, int(pl_i[j]), offset=int(po_i[j])) for j in range(n)]
    s = P.MiRtj()
    pipe = s.pipe(depth=16, coded_w=w, coded_h=h)

    def session():
        for p in pkts:
            if pipe.room() == 0:
                pipe.next(drop=True)
            pipe.submit(p)
        while pipe.pending():
            pipe.next(drop=True)

    session()
    t0 = time.perf_counter()
    for _ in range(max(1, a.steps // 5)):
        session()
    t = (time.perf_counter() - t0) / max(1, a.steps // 5)
    res["session_pictures_per_s"] = round(n / t)
    pipe.close()
    s.close()
    # ---- copy ceiling ----
    half = (fsz * n // 2) // 16 * 16
    res["copy_ceiling_gbs"] = round(dev.copy_ceiling(d_out, d_out + half, min(half, 1 << 30)), 1)
    dev.free(d_out)
    dev.free(d_inter)
    dev.free(d_intra)
    dev.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
