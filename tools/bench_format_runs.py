"""Throughput of plans with runs in the three picture formats (mi_rtj_plan_set_runs_fmt) on one MI355X.

    python tools/bench_format_runs.py [--frames 1024] [--steps 50] [--warmup 3] [--reps 3]
                                      [--out profiles/format_runs/bench_format_runs.json]

Per format (4:2:0, 4:2:2, greyscale): one stream of --frames resident pictures of 1920 x 1088, made on the device by
mi_rtj_encode_stream_fmt (quality 200, key_rate 255, masks 4 / 4) from the content of tools/bench_runs.py in the
format's plane layout — a static gradient, a 256 x 256 square that moves 8 pixels per picture and a 192 x 192 patch of
fresh noise in every picture — and decoded as ONE plan with ONE run; next to it the same pictures encoded intra-only
through a plain plan.  Before anything is timed, the first and the last picture of each plan are compared with the
checker (tests/rtjlib.py's oracle for 4:2:0, the restatement of tests/rtjfmt.py for the other two; the last picture of
the run is the in-order decode of the whole stream, decode_in_order below).
Printed per format, each case --reps times (the lists) with the median: the share of unchanged blocks (from the plan's
block index), copied blocks per launch, ms per launch from wall time over --steps launches after --warmup, phase 2's
device time (mi_rtj_plan_run_times, a profiled lap of its own), its copy rate (128 bytes per copied block: 64 read,
64 written) and that rate's share of mi_rtj_copy_ceiling measured in the same session.  The 4:2:0 row is the yardstick
for the other two; there is no pass mark.  Prints one JSON line."""
import argparse
import ctypes as C
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

NAMES = {0: "yuv420", 1: "yuv422", 2: "grey"}


def content(fmt, w, h, n, seed=7):
    """Yield n pictures of the scene of tools/bench_runs.py as contiguous planes of `fmt` (0 4:2:0, 1 4:2:2, 2 grey)."""
    sy = 1 if fmt == 0 else 0  # chroma planes are w / 2 x (h >> sy)
    yy, xx = np.mgrid[0:h, 0:w]
    bg_y = ((xx * 255) // w // 2 + (yy * 255) // h // 2).astype(np.uint8)
    cy, cx = np.mgrid[0:h >> sy, 0:w // 2]
    bg_u = ((cx * 255) // (w // 2)).astype(np.uint8)
    bg_v = ((cy * 255) // (h >> sy)).astype(np.uint8)
    square = (235 - (yy[:256, :256] % 64)).astype(np.uint8)
    rng = np.random.default_rng(seed)
    for i in range(n):
        y = bg_y.copy()
        x0, y0 = (64 + 8 * i) % (w - 256), 400
        y[y0:y0 + 256, x0:x0 + 256] = square
        y[96:288, 1536:1728] = rng.integers(0, 256, (192, 192), dtype=np.uint8)
        if fmt == 2:
            yield y.ravel()
            continue
        u, v = bg_u.copy(), bg_v.copy()
        u[y0 >> sy:(y0 + 256) >> sy, x0 // 2:x0 // 2 + 128] = 90
        v[y0 >> sy:(y0 + 256) >> sy, x0 // 2:x0 // 2 + 128] = 200
        yield np.concatenate([y.ravel(), u.ravel(), v.ravel()])


def decode_in_order(fmt, pkts, frame):
    """The block loop of rtjfmt.Restated over the packets of one stream into ONE picture (`frame`, updated in place), with
    one shortcut that makes a thousand pictures of 1080p affordable in Python: at a block start a stretch of k bytes 0xFF
    is k unchanged blocks — each is one byte and leaves its rectangle as it was — and is stepped over at once.  For whole
    packets, as an encoder makes them.
    tests/test_fmt_runs_cpu.py holds this to the restatement's own loop."""
    import rtjfmt as F
    import rtjlib as R
    import runlib_fmt as RF
    L, t, q_now = R.oracle(), R.RtjoTables(), 0
    liqt, ciqt = C.cast(t.liqt, F.i32p), C.cast(t.ciqt, F.i32p)
    coef = (C.c_int16 * 64)()
    for pkt in pkts:
        w, h, q = F.header_of(pkt)
        if q != q_now:
            q_now = max(q, 1)
            L.rtjo_make_tables(q_now, C.byref(t))
        nb = F.nblocks(fmt, w, h)
        plane, y0, x0 = RF.block_rects(fmt, w, h)
        views = RF.plane_views(fmt, frame, w, h)
        base_of = [v.ctypes.data for v in views]
        stride_of = [v.shape[1] for v in views]
        pad = np.zeros(pkt.size + 128, np.uint8)  # (whole packets only: no block may begin past the packet's end)
        pad[:pkt.size] = pkt
        # nxt[i]: the first byte at or behind i that is not 0xFF (the zero padding ends every stretch)
        not_ff = np.flatnonzero(pad != 0xFF)
        nxt = not_ff[np.searchsorted(not_ff, np.arange(pad.size))]
        sp, b = F.HEADER, 0
        while b < nb:
            skip = int(nxt[sp]) - sp
            if skip:
                skip = min(skip, nb - b)
                sp += skip
                b += skip
                continue
            luma = fmt == F.FMT_GREY or (b & 3) < 2
            sp += L.rtjo_s2b(C.cast(pad.ctypes.data + sp, R.u8p), pad.size - sp, t.lb8 if luma else t.cb8,
                             liqt if luma else ciqt, coef)
            pl = int(plane[b])
            L.rtjo_idct(coef, C.cast(base_of[pl] + int(y0[b]) * stride_of[pl] + int(x0[b]), R.u8p), stride_of[pl])
            b += 1
            if sp > pkt.size:
                raise ValueError("decode_in_order: a packet ends inside a block (rtjfmt.Restated decodes such packets)")
    return frame


def checker_pictures(fmt, pkts, fsz, in_order):
    """(first, last) picture of a plan whose slots started as zeros: of one stream decoded in order, or of independent
    packets"""
    import rtjfmt as F
    import rtjlib as R
    first = np.zeros(fsz, np.uint8)
    if fmt == F.FMT_420:
        dec = R.OracleDecoder()
        dec.decode(pkts[0], first)
        last = first.copy() if in_order else np.zeros(fsz, np.uint8)
        for p in (pkts[1:] if in_order else pkts[-1:]):
            dec.decode(p, last)
        return first, last
    decode_in_order(fmt, pkts[:1], first)
    last = first.copy() if in_order else np.zeros(fsz, np.uint8)
    decode_in_order(fmt, pkts[1:] if in_order else pkts[-1:], last)
    return first, last


def timed(fn, steps, warmup, sync):
    for _ in range(warmup):
        fn()
    sync()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    sync()
    return (time.perf_counter() - t) / steps


def med(xs):
    return float(np.median(xs))


def measure(P, fmt, a):
    import rtjfmt as F
    w, h, n, Q = 1920, 1088, a.frames, a.quality
    dev = P.MiRtj()
    dev.set_format(fmt)
    fsz = F.plane_bytes(fmt, w, h)
    d_fr = dev.alloc(fsz * n)
    for i, pic in enumerate(content(fmt, w, h, n)):
        dev.h2d(d_fr, pic, offset=i * fsz)
    d_inter, po_i, pl_i = dev.encode(w, h, Q, n, d_fr, align=64, key_rate=a.key_rate, lmask=a.lmask, cmask=a.cmask, fmt=fmt)
    d_intra, po_k, pl_k = dev.encode(w, h, Q, n, d_fr, align=64, fmt=fmt)
    dev.sync()
    dev.free(d_fr)
    oo = np.arange(n, dtype=np.uint64) * fsz
    d_out = dev.alloc(fsz * n)
    res = {"frames": n, "blocks_per_picture": F.nblocks(fmt, w, h), "stream_bytes_runs": int(pl_i.sum()),
           "stream_bytes_intra": int(pl_k.sum())}

    def plan_of(d_st, po, pl):
        hdrs = np.stack([dev.d2h(d_st, 12, offset=int(po[j])) for j in range(n)])
        return dev.plan(hdrs, po, pl, oo)

    def check(plan, d_st, po, pl, in_order, what):
        dev.memset(d_out, 0, fsz * n)
        plan.decode(d_st, d_out)
        dev.sync()
        pkts = [dev.d2h(d_st, int(pl[j]), offset=int(po[j])) for j in (range(n) if in_order else (0, n - 1))]
        for i, want in zip((0, n - 1), checker_pictures(fmt, pkts, fsz, in_order)):
            if not np.array_equal(dev.d2h(d_out, fsz, offset=int(oo[i])), want):
                raise SystemExit(f"{NAMES[fmt]}, {what}: picture {i} differs from the checker")

    # ---- the stream as one run ----
    pr = plan_of(d_inter, po_i, pl_i)
    pr.set_runs_fmt([n])
    check(pr, d_inter, po_i, pl_i, True, "one run")
    lens = np.diff(pr.read_index().astype(np.int64).reshape(n, res["blocks_per_picture"] + 1), axis=1)
    res["unchanged_share"] = round(float((lens == 1).mean()), 4)
    res["copied_blocks"] = pr.run_copied()
    # ---- the same pictures intra-only, plain plan ----
    pk = plan_of(d_intra, po_k, pl_k)
    check(pk, d_intra, po_k, pl_k, False, "intra")
    half = (fsz * n // 2) // 16 * 16
    lists = {k: [] for k in ("runs_ms_per_launch", "intra_ms_per_launch", "phase2_ms", "runs_device_ms", "copy_ceiling_gbs")}
    kernel_ms = {}
    for _ in range(a.reps):  # the cases in turn, so that a drift of the machine shows in every list
        lists["runs_ms_per_launch"].append(timed(lambda: pr.decode(d_inter, d_out), a.steps, a.warmup, dev.sync) * 1e3)
        lists["intra_ms_per_launch"].append(timed(lambda: pk.decode(d_intra, d_out), a.steps, a.warmup, dev.sync) * 1e3)
        pr.profile(True)
        for _ in range(a.steps):
            pr.decode(d_inter, d_out)
        dev.sync()
        kt, launches = pr.times()
        ms2, l2 = pr.run_times()
        lists["phase2_ms"].append(ms2 / max(l2, 1))
        lists["runs_device_ms"].append(med(pr.step_times()))
        kernel_ms = {k: round(v / launches, 4) for k, v in kt.items() if v}
        pr.profile(False)
        lists["copy_ceiling_gbs"].append(dev.copy_ceiling(d_out, d_out + half, min(half, 1 << 30)))
    res["runs_kernel_ms"] = kernel_ms
    for k, v in lists.items():
        res[k] = round(med(v), 4)
        res[k + "_reps"] = [round(x, 4) for x in v]
    gbs = [res["copied_blocks"] * 128 / (ms * 1e-3) / 1e9 for ms in lists["phase2_ms"]]
    share = [g / c for g, c in zip(gbs, lists["copy_ceiling_gbs"])]
    res["phase2_copy_gbs"] = round(med(gbs), 1)
    res["phase2_share_of_ceiling"] = round(med(share), 4)
    res["phase2_share_of_ceiling_reps"] = [round(x, 4) for x in share]
    res["runs_pictures_per_s"] = round(n / (res["runs_ms_per_launch"] * 1e-3))
    res["intra_pictures_per_s"] = round(n / (res["intra_ms_per_launch"] * 1e-3))
    pr.close()
    pk.close()
    for d in (d_out, d_inter, d_intra):
        dev.free(d)
    dev.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quality", type=int, default=200)
    ap.add_argument("--key-rate", type=int, default=255)
    ap.add_argument("--lmask", type=int, default=4)
    ap.add_argument("--cmask", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    P = importlib.import_module("gmerlin-avdecoder_amd")
    res = {"tool": "bench_format_runs", "w": 1920, "h": 1088, "quality": a.quality, "key_rate": a.key_rate,
           "lmask": a.lmask, "cmask": a.cmask, "steps": a.steps, "warmup": a.warmup, "reps": a.reps}
    for fmt in (0, 1, 2):
        res[NAMES[fmt]] = measure(P, fmt, a)
        print(NAMES[fmt], json.dumps(res[NAMES[fmt]]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
