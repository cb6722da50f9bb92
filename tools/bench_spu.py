"""What the two kernels of libmi_spu.so do on one MI355X: DVD subpicture packets resident in HBM to full-frame YUVA overlays.

    python tools/bench_spu.py [--packets 1024] [--steps 5] [--warmup 1] [--frames 720x576,720x480]
                              [--rows empty,text,worst] [--out profiles/spu/bench_spu.json]

Rows, made by the statement's encoder (tests/spuraw.py):
  empty   a full-frame rectangle, every line one fill code
  text    a seeded bitmap of two rows of block glyphs with a one-pixel outline colour, 600 x 80
  worst   a 16-bit code a pixel across a full-width rectangle, as many lines as a packet's 16-bit offsets can hold (44)
`--packets` packets, two distinct ones repeated, lie in one stream at odd byte offsets, each copy in memory of its own; one
mi_spu_decode_batch per step.  The times of the two kernels are read after every step (mi_spu_times: HIP events around each
launch); the medians over the steps are reported.  Beside each row a hipMemsetAsync of the same picture bytes is timed with
HIP events in the same way: the output is write-only, so that fill is the ceiling.  ns_per_code is the decode launch over
the codes one wave walks (the longer field of one packet; the waves of a launch walk side by side): an upper bound of the
walk's time a code, since the launch stores the rows too.
The first and the last picture and every status are checked against the statement.  There is no pass mark.  One JSON line
per row on stdout; `--out` keeps them all in one file."""
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
DISTINCT = 2


def glyphs(rng, width=600, height=80):
    """colour indices of two rows of block glyphs: 0 background, 1 the glyph's body, 2 its one-pixel outline"""
    body = np.zeros((height, width), bool)
    for top in (6, 44):
        x = 8
        while x + 24 < width:
            gw = int(rng.integers(10, 22))
            cells = rng.integers(0, 2, (5, 3)).astype(bool)
            cells[2] = True  # a bar through every glyph
            body[top:top + 30, x:x + gw] = np.kron(cells, np.ones((6, -(-gw // 3)), bool))[:, :gw]
            x += gw + int(rng.integers(3, 9))
    grown = body.copy()
    grown[1:] |= body[:-1]
    grown[:-1] |= body[1:]
    grown[:, 1:] |= body[:, :-1]
    grown[:, :-1] |= body[:, 1:]
    return np.where(body, 1, np.where(grown, 2, 0)).astype(np.uint8)


def content_packet(S, content, rng, w, h):
    """(packet, codes the longer field holds)"""
    if content == "empty":
        idx = np.full((h, w), int(rng.integers(0, 4)), np.uint8)
        return S.encode(idx), h // 2
    if content == "text":
        idx = glyphs(rng)
        p = S.encode(idx, 60, h - 100)
        codes = max(sum(len(S.runs_of(r)) for r in idx[f::2]) for f in (0, 1))
        return p, codes
    lines = 44
    idx = ((np.arange(w)[None, :] + rng.integers(0, 4, (lines, 1))) % 4).astype(np.uint8)
    return S.encode(idx, fill_ends=False, wide=True), lines // 2 * w


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


def main():
    import spuraw as S
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--frames", default="720x576,720x480")
    ap.add_argument("--rows", default="empty,text,worst")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.steps < 5:
        ap.error("--steps: a median of at least 5 launches")
    spu = importlib.import_module("gmerlin-avdecoder_amd.spu")
    n = a.packets
    dev = spu.MiSpu(0)
    hip = Hip()
    lines, ok = [], True
    try:
        for frame in a.frames.split(","):
            w, h = (int(t) for t in frame.split("x"))
            size = w * h * 4
            qs = spu.up16(size)
            for content in a.rows.split(","):
                rng = np.random.default_rng(5000 + len(lines))
                pal = S.random_palette(rng)
                made = [content_packet(S, content, rng, w, h) for _ in range(DISTINCT)]
                packets, codes = [m[0] for m in made], max(m[1] for m in made)
                offsets, cur = np.zeros(n, np.uint64), 1
                for k in range(n):
                    offsets[k] = cur
                    cur += packets[k % DISTINCT].size + 2 * (k % 3)
                    cur += 1 - cur % 2
                lengths = np.array([packets[k % DISTINCT].size for k in range(n)], np.uint32)
                ds, dq, di = dev.alloc(cur + 16), dev.alloc(n * qs), dev.alloc(spu.INFO_BYTES * n)
                try:
                    for k in range(n):
                        dev.h2d(ds, packets[k % DISTINCT], offset=int(offsets[k]))
                    dev.sync()
                    dev.times()
                    ms, fill_ms = [], []
                    for step in range(a.warmup + a.steps):
                        dev.decode_batch(ds, offsets, lengths, w, h, dq, qs, pal, di)
                        t, launches = dev.times()
                        assert launches == 2
                        if step >= a.warmup:
                            ms.append(t)
                    exact = all(i.status == 0 for i in spu.infos(dev.d2h(di, spu.INFO_BYTES * n)))
                    for k in (0, n - 1):
                        st, want, _ = S.decode(packets[k % DISTINCT], w, h, pal)
                        exact &= st == 0 and np.array_equal(dev.d2h(dq, size, offset=k * qs), want.reshape(-1))
                    ok &= exact
                    for step in range(a.warmup + a.steps):
                        t = hip.memset_ms(dq, n * qs)
                        if step >= a.warmup:
                            fill_ms.append(t)
                finally:
                    dev.free(ds), dev.free(dq), dev.free(di)
                scan, decode = (statistics.median(m[i] for m in ms) for i in range(2))
                total, fill = statistics.median(sum(m) for m in ms), statistics.median(fill_ms)
                picture_bytes = n * size
                line = {"tool": "bench_spu", "content": content, "width": w, "height": h, "packets": n, "steps": a.steps, "warmup": a.warmup,
                        "packet_bytes": [int(p.size) for p in packets], "picture_bytes": size, "codes_per_wave": int(codes),
                        "ms_scan": round(scan, 4), "ms_decode": round(decode, 4), "ms_total": round(total, 4),
                        "us_per_packet": round(total * 1e3 / n, 4),
                        "picture_gbytes_per_s": round(picture_bytes / (total / 1e3) / 1e9, 1),
                        "ms_memset": round(fill, 4), "memset_gbytes_per_s": round(n * qs / (fill / 1e3) / 1e9, 1),
                        "share_of_fill_ceiling": round(fill / total, 4),
                        "ns_per_code": round(decode * 1e6 / codes, 2),
                        "exact_first_and_last_picture": bool(exact)}
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
