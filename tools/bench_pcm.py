"""What k_pcm_decode of libmi_pcm.so does on one MI355X: every codec of lib/audio_pcm.c over packets resident in HBM.

    python tools/bench_pcm.py [--codecs COPY8,...,ALAW] [--workloads small,large] [--steps 7] [--warmup 2]
                              [--out profiles/pcm/bench_pcm.json]

Per codec, stereo (the two mono codecs: one channel), two workloads: `small` is 4,096 packets of 64 KiB at byte phases
0..15 of a 16-byte word in turn, `large` is 16 packets of 16 MiB, phases likewise.  Eight distinct packets (tests/pcmraw.py's
content: any bytes, the float codecs' samples inside the defined domain), repeated, are one mi_pcm_decode_batch per step
into sample slots at multiples of 256; the float codecs are given counts, the others none.  The device time is read after
every step (mi_pcm_times: HIP events around each launch, k_pcm_zero's included where there are counts); the median over the
steps is reported with the bytes the launch reads plus the bytes it writes (the consumed bytes of the packets and the
samples, counted from the layout) per second, against 8 TB/s and against mi_rtj_copy_ceiling (k_copy16, read plus write,
between the same two buffers, over as many bytes as the smaller of them) measured next to it in the same run.  The first
and the last packet's samples are checked against the statement (tests/pcmraw.py).  There is no pass mark.  One JSON line
per codec and workload on stdout; `--out` keeps them all in one file."""
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
WORKLOADS = {"small": (4096, 64 << 10), "large": (16, 16 << 20)}


def main():
    import pcmraw as R
    ap = argparse.ArgumentParser()
    ap.add_argument("--codecs", default=",".join(R.CODECS))
    ap.add_argument("--workloads", default="small,large")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.steps < 5:
        ap.error("--steps: a median of at least 5 launches")
    pcm = importlib.import_module("gmerlin-avdecoder_amd.pcm")
    P = importlib.import_module("gmerlin-avdecoder_amd")
    dev, rtj = pcm.MiPcm(0), P.MiRtj(0)
    lines, ok = [], True
    try:
        for name in a.codecs.split(","):
            c = R.codec(name)
            ch = 1 if c in R.MONO else 2
            counted = c in R.FLOATS
            for wl in a.workloads.split(","):
                n, size = WORKLOADS[wl]
                frames, _, consumed, out_bytes = pcm.layout_of(c, ch, size)
                assert (frames, consumed, out_bytes) == (R.layout(c, ch, size)[0],) + R.layout(c, ch, size)[2:]
                stride_in, stride_out = size + 256, (out_bytes + 255) // 256 * 256
                distinct = [np.frombuffer(R.content(c, size, 3000 + 17 * c + i), np.uint8) for i in range(DISTINCT)]
                offsets = np.array([k * stride_in + k % 16 for k in range(n)], np.uint64)
                slots = np.array([k * stride_out for k in range(n)], np.uint64)
                dp, dq, dc = dev.alloc(n * stride_in + 16), dev.alloc(n * stride_out), dev.alloc(4 * n)
                try:
                    for k in range(n):
                        dev.h2d(dp, distinct[k % DISTINCT], offset=int(offsets[k]))
                    dev.sync()
                    dev.times()
                    ms = []
                    for step in range(a.warmup + a.steps):
                        dev.decode_batch(c, ch, dp, offsets, np.full(n, size, np.uint32), dq, slots, dc if counted else None)
                        t, launches = dev.times()
                        assert launches == (2 if counted else 1)
                        if step >= a.warmup:
                            ms.append(t)
                    exact = True
                    for k in (0, n - 1):
                        want, count = R.decode(c, ch, distinct[k % DISTINCT].tobytes())
                        exact &= np.array_equal(dev.d2h(dq, out_bytes, offset=int(slots[k])), want)
                        exact &= not counted or int(dev.d2h(dc, 4, offset=4 * k, dtype=np.uint32)[0]) == count
                    ok &= exact
                    ceiling = min(n * stride_in, n * stride_out, 1 << 30) // 16 * 16
                    copy_gbs = rtj.copy_ceiling(dp, dq, ceiling)
                finally:
                    dev.free(dp)
                    dev.free(dq)
                    dev.free(dc)
                med = statistics.median(ms)
                moved = n * (consumed + out_bytes)
                gbs = moved / (med / 1e3) / 1e9
                line = {"tool": "bench_pcm", "codec": name, "library": "libmi_pcm.so", "kernel": f"k_pcm_decode<{name}>", "workload": wl,
                        "channels": ch, "packets": n, "packet_bytes": size, "sample_bytes_a_packet": out_bytes, "counts": counted,
                        "launches_a_call": 2 if counted else 1, "steps": a.steps, "warmup": a.warmup,
                        "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                        "bytes_read_plus_written": moved, "gbytes_per_s": round(gbs, 1),
                        "gsamples_per_s": round(n * frames * ch / (med / 1e3) / 1e9, 2),
                        "share_of_8tb_s": round(gbs * 1e9 / HBM_BYTES_PER_S, 4), "copy_ceiling_bytes": ceiling,
                        "copy_ceiling_gbytes_per_s": round(copy_gbs, 1), "share_of_copy_ceiling": round(gbs / copy_gbs, 4),
                        "exact_first_and_last_packet": bool(exact)}
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
