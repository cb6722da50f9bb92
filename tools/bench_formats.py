"""Throughput of 4:2:2 and greyscale plans (mi_rtj_set_format) and of the encoder in those formats (mi_rtj_encode_frames_fmt)
on one MI355X, next to the 4:2:0 plan and the 4:2:0 encoder on the same pictures in the same run.

    python tools/bench_formats.py [--packets device|reference] [--frames 1024] [--enc-frames 4096] [--steps 20]
                                  [--warmup 3] [--out profiles/formats_encode/bench_formats.json]

Per format: --frames resident packets of 1920x1088 at quality 255 — 16 distinct pictures of the bench content (the
gradient + LCG noise of bench.py, amplitude 8, seed 12345: tests/rtjlib.py synth_frame_lcg), each packet its own copy in
the stream buffer — decoded by one plan, one output slot per packet.  4:2:2 pictures take the 4:2:0 chroma lines twice;
greyscale pictures are the luma plane.
--packets device (the default): the packets come from the device's own encoder, and the first and the last of each
format are compared with the checker's restatement (tests/rtjfmt_enc.py over the pinned oracle) before anything is timed;
nothing but the oracle is needed.  --packets reference: they come from the reference's own encoder (oracle/_ref/
librtjpeg_ref.so, RTjpeg_set_format + RTjpeg_compress), as in the table of DESIGN.md section 11; without that library the
tool says so and exits with status 2.  The reference's greyscale packets do not code the picture they are given: its
greyscale arm reads a block at a line stride of 8 w and moves on by one line per block row (lib/RTjpeg.c:2626, 2630), so
they code an interleaved excerpt of the top h / 8 + 56 lines (192 at 1088); the output says so.
Printed per format: pictures per second from wall time over --steps launches after --warmup, the index's and the
transform's device time per launch (mi_rtj_plan_times: MI_RTJ_K_EMIT, MI_RTJ_K_DECODE; for 4:2:0 every kernel of its
path), the algorithmic bytes (packets read once, planes written once) and the transform's share of 8 TB/s with them; and
"encoder": pictures and blocks per second of one intra call over --enc-frames resident pictures (wall time of the
synchronous call, the median of five after one warm-up call).  The encoder's yardstick is the 4:2:0 call of the same run
(mi_rtj_encode_frames): the formats run the same kernel and the same work per block on 4/3 and 2/3 of the blocks.
There is no pass mark: these formats have no earlier figure.  Prints one JSON line."""
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

HBM_PEAK = 8e12  # bytes per second, nominal
NAMES = {0: "yuv420", 1: "yuv422", 2: "grey"}


def pictures(fmt, w, h, count, F, R):
    """`count` distinct pictures of the bench content in the format's plane layout"""
    out = []
    for i in range(count):
        p = R.synth_frame_lcg(w, h, i, seed=12345, amp=8)
        y, u, v = R.split_planes(p, w, h)
        if fmt == F.FMT_GREY:
            out.append(y.copy())
        elif fmt == F.FMT_422:
            twice = lambda c: np.repeat(c.reshape(h // 2, w // 2), 2, axis=0).reshape(-1)
            out.append(np.concatenate([y, twice(u), twice(v)]))
        else:
            out.append(p)
    return out


def encode_on_device(dev, fmt, w, h, Q, pics, n, reps=0):
    """n pictures (the distinct ones in turn) resident on the device, encoded by one intra call.  Returns the first
    len(pics) packets and, with reps, the wall seconds of the median call."""
    fsz = pics[0].size
    d_fr = dev.alloc(fsz * n)
    for i in range(n):
        dev.h2d(d_fr, pics[i % len(pics)], offset=i * fsz)
    d_st = dev.alloc(dev.encode_bound(w, h, n, 64, fmt=fmt))
    _, po, pl = dev.encode(w, h, Q, n, d_fr, align=64, d_stream=d_st, fmt=fmt)  # (the warm-up call when timing)
    pkts = [dev.d2h(d_st, int(pl[i]), offset=int(po[i])) for i in range(min(n, len(pics)))]
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        dev.encode(w, h, Q, n, d_fr, align=64, d_stream=d_st, fmt=fmt)
        times.append(time.perf_counter() - t0)
    dev.free(d_fr)
    dev.free(d_st)
    return pkts, (float(np.median(times)) if times else None)


def restated_packet(F, R, fmt, w, h, Q, pic):
    if fmt == F.FMT_420:
        return R.OracleEncoder(w, h, Q).encode(pic)
    import rtjfmt_enc as E
    return E.encode_all(fmt, w, h, Q, [pic])[0]


def measure(P, F, R, fmt, w, h, n, distinct, steps, warmup, source, enc_frames):
    pics = pictures(fmt, w, h, distinct, F, R)
    encoder = None
    if source == "reference":
        enc = F.RefFmt(fmt)
        enc.setup_encoder(w, h, 255)
        distinct_pkts = [enc.encode(p) for p in pics]
    else:
        dev = P.MiRtj()
        distinct_pkts, _ = encode_on_device(dev, fmt, w, h, 255, pics, distinct)
        for i in (0, distinct - 1):  # the packets the figures are taken on are the checker's, byte for byte
            if not np.array_equal(distinct_pkts[i], restated_packet(F, R, fmt, w, h, 255, pics[i])):
                raise SystemExit(f"{NAMES[fmt]}: device packet {i} differs from the checker's restatement")
        dev.close()
    if enc_frames > 0:
        dev = P.MiRtj()
        _, sec = encode_on_device(dev, fmt, w, h, 255, pics, enc_frames, reps=5)
        dev.close()
        nb = F.nblocks(fmt, w, h)
        encoder = {"frames": enc_frames, "ms_per_call": round(sec * 1e3, 3), "pictures_per_s": round(enc_frames / sec, 1),
                   "blocks_per_picture": nb, "blocks_per_s": round(enc_frames * nb / sec, 1)}
    pkts = [distinct_pkts[i % distinct] for i in range(n)]
    dev = P.MiRtj()
    dev.set_format(fmt)
    d_st, po, pl, hdrs = dev.upload_packets(pkts, align=64)
    fsz = F.plane_bytes(fmt, w, h)
    oo = np.arange(n, dtype=np.uint64) * fsz
    d_out = dev.alloc(fsz * n)
    dev.memset(d_out, 0, fsz * n)
    plan = dev.plan(hdrs, po, pl, oo)
    for _ in range(warmup):
        plan.decode(d_st, d_out)
    dev.sync()
    # the first and the last picture against the checker, so that the figure is of pictures that are right
    for i in (0, n - 1):
        got = dev.d2h(d_out, fsz, offset=int(oo[i]))
        want = np.zeros(fsz, np.uint8)
        if fmt == F.FMT_420:
            R.OracleDecoder().decode(pkts[i], want)
        else:
            F.Restated(fmt).decode(pkts[i], want)
        if not np.array_equal(got, want):
            raise SystemExit(f"{NAMES[fmt]}: picture {i} differs from the checker")
    t0 = time.perf_counter()
    for _ in range(steps):
        plan.decode(d_st, d_out)
    dev.sync()
    dt = (time.perf_counter() - t0) / steps
    plan.profile(True)
    for _ in range(steps):
        plan.decode(d_st, d_out)
    dev.sync()
    kt, launches = plan.times()
    device_ms = float(np.median(plan.step_times()))
    plan.profile(False)
    info = plan.info()
    algo = info["bytes_in"] + info["bytes_out"]
    index_ms = sum(v for k, v in kt.items() if k != "k_decode") / launches
    decode_ms = kt["k_decode"] / launches
    res = {"frames": n, "distinct_pictures": distinct, "blocks": info["blocks"], "bytes_in": info["bytes_in"],
           "bytes_out": info["bytes_out"], "algorithmic_bytes": algo,
           "frames_per_s": round(n / dt, 1), "ms_per_launch_wall": round(dt * 1e3, 4),
           "device_ms_per_launch": round(device_ms, 4), "index_ms": round(index_ms, 4), "transform_ms": round(decode_ms, 4),
           "kernel_ms": {k: round(v / launches, 4) for k, v in kt.items() if v},
           "transform_share_of_8TBs": round(algo / (decode_ms * 1e-3) / HBM_PEAK, 4),
           "launch_share_of_8TBs": round(algo / (device_ms * 1e-3) / HBM_PEAK, 4),
           "packets": source, "encoder": encoder}
    plan.close()
    dev.free(d_st)
    dev.free(d_out)
    dev.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1088)
    ap.add_argument("--packets", choices=("device", "reference"), default="device", help="who encodes the packets")
    ap.add_argument("--enc-frames", type=int, default=4096, help="resident pictures of the timed encoder call (0: skip)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import rtjfmt as F
    import rtjlib as R
    if a.packets == "reference" and not R.have_reference():
        print("tools/bench_formats.py: oracle/_ref/librtjpeg_ref.so is missing — the packets of this measurement come from "
              "the reference's encoder; build the oracle where the reference tree is present", file=sys.stderr)
        return 2
    if a.steps < 20:
        print("tools/bench_formats.py: --steps below 20: not a measurement", file=sys.stderr)
    P = importlib.import_module("gmerlin-avdecoder_amd")
    res = {"tool": "bench_formats", "w": a.width, "h": a.height, "quality": 255, "steps": a.steps, "warmup": a.warmup,
           "packets": a.packets,
           "content": "bench content: gradient + LCG noise, amplitude 8, seed 12345; packets by " +
                      ("the device encoder, first and last of each format equal to the checker's restatement"
                       if a.packets == "device" else
                       "the reference encoder; its greyscale packets code an interleaved excerpt of the top lines (a block "
                       "read at a line stride of 8 w, lib/RTjpeg.c:2626, 2630), not the picture")}
    for fmt in (F.FMT_422, F.FMT_GREY, F.FMT_420):
        res[NAMES[fmt]] = measure(P, F, R, fmt, a.width, a.height, a.frames, a.distinct, a.steps, a.warmup, a.packets,
                                  a.enc_frames)
    base = res[NAMES[F.FMT_420]]["encoder"]
    for fmt in (F.FMT_422, F.FMT_GREY):  # the yardstick: the 4:2:0 call's rate per block in the same run
        e = res[NAMES[fmt]]["encoder"]
        if e and base:
            e["yuv420_pictures_per_s_same_run"] = base["pictures_per_s"]
            e["blocks_per_s_over_yuv420"] = round(e["blocks_per_s"] / base["blocks_per_s"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
