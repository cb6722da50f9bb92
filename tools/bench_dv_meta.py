"""What the DV timecode kernels do on one MI355X: k_dv_meta_extract and k_dv_meta_write over frames resident in HBM, next to
what the host route costs on the same box.

    python tools/bench_dv_meta.py [--systems 525,625,625_411,525_422,625_422] [--frames 1024] [--steps 7] [--warmup 2]
                                  [--out profiles/dv_meta/bench_dv_meta.json]

Per system: `--frames` frames resident in HBM — eight distinct frames of random bytes, repeated — are one
mi_dv_meta_write_batch and one mi_dv_meta_batch per step.  The kernels' times are read after every step
(mi_dv_meta_times: HIP events around the launch) and the medians over the steps are reported with the bytes each kernel
moves (extract: the 32-byte sectors its loads touch, and the rows; write: the five DIF blocks of every sequence) per second
and against 8 TB/s.  Beside them, on the same frames, the host route: the device-to-host copy of the whole frames
(mi_dv_d2h into pageable memory, wall clock), then mi_dv_timecode, mi_dv_date, mi_dv_time and mi_dv_pixel_aspect of
libmi_dvframe.so per frame on one core.  The first and the last frame are checked against the statement (tests/dvmeta.py).
There is no pass mark.  One JSON line per system on stdout; `--out` keeps them all in one file.  PARITY UNPINNED."""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
DISTINCT = 8
HBM_BYTES_PER_S = 8e12
PROFILE_OF = {0: 0, 1: 1, 3: 2, 4: 3, 5: 4}  # system -> index in include/mi_dvframe.h's table


def host_reader():
    L = C.CDLL(os.path.join(ROOT, "gmerlin-avdecoder_amd", "lib", "libmi_dvframe.so"))
    L.mi_dv_profile_at.restype = C.c_void_p
    ip = C.POINTER(C.c_int)
    L.mi_dv_timecode.argtypes = [C.c_void_p, C.c_void_p, ip, ip, ip, ip]
    L.mi_dv_date.argtypes = L.mi_dv_time.argtypes = [C.c_void_p, C.c_void_p, ip, ip, ip]
    L.mi_dv_pixel_aspect.argtypes = [C.c_void_p, C.c_void_p, ip, ip]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", default="525,625,625_411,525_422,625_422")
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.steps < 5:
        ap.error("--steps: a median of at least 5 launches")
    dv = importlib.import_module("gmerlin-avdecoder_amd.dv")
    import dvmeta as M
    names = {"525": dv.SYS_525_60, "625": dv.SYS_625_50, "625_411": dv.SYS_625_50_411, "525_422": dv.SYS_525_60_422,
             "625_422": dv.SYS_625_50_422}
    H = host_reader()
    dev = dv.MiDv(0)
    lines, ok = [], True
    try:
        for name in a.systems.split(","):
            system = names[name]
            m = M.META[system]
            fb, n = m.frame_bytes, a.frames
            drop, first, rec = 0 if m.dsf else 1, 1700, 1709251199 - 20
            distinct = np.stack([M.noise_frame(system, 90 + i, wiped=False) for i in range(DISTINCT)])
            df, dm = dev.alloc(n * fb), dev.alloc(n * 64)
            try:
                for k in range(0, n, DISTINCT):
                    dev.h2d(df, distinct[:min(DISTINCT, n - k)], offset=k * fb)
                dev.sync()
                dev.meta_times()
                ex, wr, copy = [], [], []
                for step in range(a.warmup + a.steps):
                    dev.write_meta_batch(system, df, n, first, drop, rec, 1)
                    t = dev.meta_times()[0]
                    dev.meta_batch(system, df, n, dm)
                    u = dev.meta_times()[0]
                    if step >= a.warmup:
                        wr.append(t)
                        ex.append(u)
                rows = dev.d2h(dm, n * 64).view(np.int32).reshape(n, M.INTS)
                exact = True
                for k in (0, n - 1):
                    want = M.write_one(system, distinct[k % DISTINCT], first + k, drop, M.rec_of(system, rec, k), 1)
                    exact &= bool(np.array_equal(dev.d2h(df, fb, offset=k * fb), want))
                    exact &= rows[k].tolist() == M.extract(system, want).tolist()
                ok &= exact
                for _ in range(3):
                    t0 = time.perf_counter()
                    host = dev.d2h(df, n * fb)
                    copy.append((time.perf_counter() - t0) * 1e3)
                prof = H.mi_dv_profile_at(PROFILE_OF[system])
                v = [C.c_int() for _ in range(4)]
                r = [C.byref(x) for x in v]
                base = host.ctypes.data
                t0 = time.perf_counter()
                for i in range(n):
                    f = base + i * fb
                    H.mi_dv_timecode(prof, f, r[0], r[1], r[2], r[3])
                    H.mi_dv_date(prof, f, r[0], r[1], r[2])
                    H.mi_dv_time(prof, f, r[0], r[1], r[2])
                    H.mi_dv_pixel_aspect(prof, f, r[0], r[1])
                cpu_ms = (time.perf_counter() - t0) * 1e3
            finally:
                dev.free(df)
                dev.free(dm)
            # extract: a lane reads 8 bytes of its packet: six packets lie in 48 consecutive bytes of a subcode block
            # (two 32-byte sectors, or three where they straddle), so about 3 sectors a block; + the header and the
            # control pack; + the row.  write: the five blocks of every sequence, whole
            ex_bytes = n * (m.seqs * 2 * 96 + 64 + 64)
            wr_bytes = n * m.chans * m.seqs * 400
            em, wm = statistics.median(ex), statistics.median(wr)
            host_ms = statistics.median(copy) + cpu_ms
            line = {"tool": "bench_dv_meta", "system": name, "frames": n, "steps": a.steps, "warmup": a.warmup,
                    "extract_ms_median": round(em, 4), "extract_ms_min": round(min(ex), 4), "extract_ms_max": round(max(ex), 4),
                    "extract_us_per_frame": round(em * 1e3 / n, 4), "extract_bytes": ex_bytes,
                    "extract_gbytes_per_s": round(ex_bytes / (em / 1e3) / 1e9, 1),
                    "extract_share_of_8tb_s": round(ex_bytes / (em / 1e3) / HBM_BYTES_PER_S, 5),
                    "write_ms_median": round(wm, 4), "write_ms_min": round(min(wr), 4), "write_ms_max": round(max(wr), 4),
                    "write_us_per_frame": round(wm * 1e3 / n, 4), "write_bytes": wr_bytes,
                    "write_gbytes_per_s": round(wr_bytes / (wm / 1e3) / 1e9, 1),
                    "write_share_of_8tb_s": round(wr_bytes / (wm / 1e3) / HBM_BYTES_PER_S, 5),
                    "host_readers_one_core_ms": round(cpu_ms, 3), "frames_d2h_ms_median": round(statistics.median(copy), 3),
                    "host_route_us_per_frame": round(host_ms * 1e3 / n, 3),
                    "extract_beats_host_route": bool(em < host_ms), "exact_first_and_last_frame": exact, "parity": "unpinned"}
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
