"""What k_gsm_decode of libmi_gsm.so does on one MI355X: GSM 06.10 streams resident in HBM to their samples.

    python tools/bench_gsm.py [--steps 5] [--warmup 1] [--rows 65536x64,4096x1024,64x4096,1x4096,65536x64:1]
                              [--out profiles/gsm/bench_gsm.json]

A row is streams x frames, ":1" for the Microsoft framing (two frames a block).  The streams are the statement's packer
(tests/gsmraw.py) over seeded parameters: three distinct streams, repeated in turn, each copy in memory of its own at a
byte address of its own; one mi_gsm_decode_batch a step, every stream from a fresh state.  The kernel's time is read after
every step (mi_gsm_times: HIP events around the launch); the median over the steps is reported as frames a second, as a
multiple of real time (a frame is 20 ms of sound) and as output bytes a second.  Beside each row a hipMemsetAsync of the
same sample bytes is timed with HIP events in the same way: the output is write-only, so that fill is the ceiling.
ns_per_frame is the launch over the frames of one stream: in the row of one stream that is one lane's chain.
The first and the last stream of each row are checked against the statement.  There is no pass mark.  One JSON line per
row on stdout; `--out` keeps them all in one file."""
import argparse
import ctypes as C
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
DISTINCT = 3
FRAME_SECONDS = 0.02


class Hip:
    """the few calls of the HIP runtime the fill ceiling needs"""

    def __init__(self):
        self.L = C.CDLL("libamdhip64.so")
        self.start, self.stop = C.c_void_p(), C.c_void_p()
        self.chk(self.L.hipEventCreate(C.byref(self.start)))
        self.chk(self.L.hipEventCreate(C.byref(self.stop)))

    def chk(self, rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")

    def memset_ms(self, d, nbytes):
        self.chk(self.L.hipEventRecord(self.start, None))
        self.chk(self.L.hipMemsetAsync(C.c_void_p(d), 0, C.c_size_t(nbytes), None))
        self.chk(self.L.hipEventRecord(self.stop, None))
        self.chk(self.L.hipEventSynchronize(self.stop))
        ms = C.c_float()
        self.chk(self.L.hipEventElapsedTime(C.byref(ms), self.start, self.stop))
        return ms.value


class Content:
    """the distinct streams of a framing and what the statement makes of them; a shorter row uses a prefix of both"""

    def __init__(self, G, fmt, frames):
        rng = np.random.default_rng(6100 + fmt)
        units = frames >> fmt
        self.G, self.fmt, self.units = G, fmt, units
        self.streams = [b"".join(G.implode(G.random_params(rng, fmt), fmt) for _ in range(units)) for _ in range(DISTINCT)]
        self.pcm = {}

    def want(self, d):
        if d not in self.pcm:
            self.pcm[d] = self.G.decode_stream(self.streams[d], self.fmt)[0]
        return self.pcm[d]


def main():
    import gsmraw as G
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", default="65536x64,4096x1024,64x4096,1x4096,65536x64:1")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.steps < 5:
        ap.error("--steps: a median of at least 5 launches")
    gsm = importlib.import_module("gmerlin-avdecoder_amd.gsm")
    rows = []
    for text in a.rows.split(","):
        shape, _, fmt = text.partition(":")
        n, frames = (int(t) for t in shape.split("x"))
        rows.append((n, frames, int(fmt or 0)))
    content = {fmt: Content(G, fmt, max(f for _, f, m in rows if m == fmt)) for fmt in {m for _, _, m in rows}}
    dev = gsm.MiGsm(0)
    hip = Hip()
    lines, ok = [], True
    try:
        for n, frames, fmt in rows:
            c = content[fmt]
            units = frames >> fmt
            size = units * G.unit_bytes(fmt)
            stride = size + 1  # streams start at every byte phase
            host = np.zeros(1 + n * stride, np.uint8)
            table = host[1:].reshape(n, stride)
            for d in range(DISTINCT):
                table[d::DISTINCT, :size] = np.frombuffer(c.streams[d][:size], np.uint8)
            offsets = 1 + np.arange(n, dtype=np.uint64) * np.uint64(stride)
            sample_bytes = frames * 2 * G.FRAME_SAMPLES
            pcm_offsets = np.arange(n, dtype=np.uint64) * np.uint64(sample_bytes)
            ds, dp = dev.alloc(host.nbytes + 16), dev.alloc(n * sample_bytes)
            try:
                dev.h2d(ds, host)
                dev.sync()
                dev.times()
                ms, fill_ms = [], []
                for step in range(a.warmup + a.steps):
                    dev.decode_batch(ds, offsets, np.full(n, units, np.uint32), fmt, dp, pcm_offsets)
                    t, launches = dev.times()
                    assert launches == 1
                    if step >= a.warmup:
                        ms.append(t)
                exact = True
                for k in (0, n - 1):
                    got = dev.d2h(dp, sample_bytes, offset=k * sample_bytes, dtype=np.int16)
                    exact &= bool(np.array_equal(got, c.want(k % DISTINCT)[:got.size]))
                ok &= exact
                for step in range(a.warmup + a.steps):
                    t = hip.memset_ms(dp, n * sample_bytes)
                    if step >= a.warmup:
                        fill_ms.append(t)
            finally:
                dev.free(ds), dev.free(dp)
            t, fill = statistics.median(ms), statistics.median(fill_ms)
            per_s = n * frames / (t / 1e3)
            line = {"tool": "bench_gsm", "fmt": fmt, "streams": n, "frames_per_stream": frames, "steps": a.steps, "warmup": a.warmup,
                    "stream_bytes": size, "sample_bytes": n * sample_bytes, "ms_decode": round(t, 4),
                    "frames_per_s": round(per_s, 1), "times_real_time": round(per_s * FRAME_SECONDS, 1),
                    "sample_gbytes_per_s": round(n * sample_bytes / (t / 1e3) / 1e9, 2),
                    "ms_memset": round(fill, 4), "memset_gbytes_per_s": round(n * sample_bytes / (fill / 1e3) / 1e9, 1),
                    "share_of_fill_ceiling": round(fill / t, 4),
                    "ns_per_frame": round(t * 1e6 / frames, 1),
                    "exact_first_and_last_stream": bool(exact)}
            print(json.dumps(line), flush=True)
            lines.append(line)
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
