"""What the DV sound kernels do on one MI355X: k_dv_audio_extract and k_dv_audio_write over frames resident in HBM, next
to what the host route costs on the same box.

    python tools/bench_dv_audio.py [--systems 525,625,625_411,525_422,625_422] [--frames 1024] [--steps 7] [--warmup 2]
                                   [--out profiles/dv_audio/bench_dv_audio.json]

Per system: `--frames` frames resident in HBM — eight distinct frames of random bytes with 16-bit 48 kHz sound, repeated —
are one mi_dv_audio_batch and one mi_dv_audio_write_batch per step.  The kernels' times are read after every step
(mi_dv_audio_times: HIP events around the launch) and the medians over the steps are reported with the bytes each kernel
moves (the sample bytes of the audio blocks, the pairs' buffers, the info rows) per second and against 8 TB/s.  Beside
them, on the same frames: mi_dv_extract_audio of libmi_dvframe.so on one core; the device-to-host copy of the whole frames
that the host route needs first (mi_dv_d2h into pageable memory, wall clock); and k_dv_decode of the batch
(mi_dv_kernel_times).  The first frame's sound is checked byte for byte against the statement (tests/dvaudio.py).  There is
no pass mark.  One JSON line per system on stdout; `--out` keeps them all in one file.  PARITY UNPINNED."""
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
    L.mi_dv_extract_audio.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
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
    import dvaudio as A
    names = {"525": dv.SYS_525_60, "625": dv.SYS_625_50, "625_411": dv.SYS_625_50_411, "525_422": dv.SYS_525_60_422,
             "625_422": dv.SYS_625_50_422}
    H = host_reader()
    dev = dv.MiDv(0)
    lines, ok = [], True
    try:
        for name in a.systems.split(","):
            system = names[name]
            s = A.SOUND[system]
            fb, pb, _ = dv.geometry(system)
            n, pairs = a.frames, s.chans
            counts = [dv.audio_samples(system, 48000, i) for i in range(n)]
            distinct = np.stack([A.noise_frame(system, 90 + i, counts[i] - s.min_samples[0], 0, 0) for i in range(DISTINCT)])
            df, dp, ds, di = dev.alloc(n * fb), dev.alloc(n * pb), dev.alloc(n * pairs * A.PAIR_BYTES), dev.alloc(n * 16)
            try:
                for k in range(0, n, DISTINCT):
                    dev.h2d(df, distinct[:min(DISTINCT, n - k)], offset=k * fb)
                for _ in range(a.warmup):
                    dev.audio_batch(system, df, n, ds, pairs, di)
                    dev.decode_batch_sys(system, df, n, dp)
                dev.sync()
                dev.audio_times()
                dev.kernel_times()
                ex, wr, dec, copy = [], [], [], []
                for _ in range(a.steps):
                    dev.audio_batch(system, df, n, ds, pairs, di)
                    ex.append(dev.audio_times()[0])
                    dev.decode_batch_sys(system, df, n, dp)
                    dec.append(dev.kernel_times()[0])
                exact = bool(np.array_equal(dev.d2h(ds, pairs * A.PAIR_BYTES).reshape(pairs, -1), A.extract(system, distinct[0], pairs)[1]))
                for step in range(a.warmup + a.steps):  # (the sound just read goes back into the frames: they stay what they were
                    dev.write_audio_batch(system, df, n, ds, pairs, 48000, counts)  # but for ids and packs)
                    t = dev.audio_times()[0]
                    if step >= a.warmup:
                        wr.append(t)
                exact &= bool(np.array_equal(dev.d2h(df, fb), A.write(system, distinct[0], A.extract(system, distinct[0], pairs)[1],
                                                                     48000, counts[0])))
                ok &= exact
                for _ in range(3):
                    t0 = time.perf_counter()
                    host = dev.d2h(df, n * fb)
                    copy.append((time.perf_counter() - t0) * 1e3)
                prof = H.mi_dv_profile_at(PROFILE_OF[system])
                bufs = np.zeros((4, A.PAIR_BYTES), np.uint8)
                arr = (C.c_void_p * 4)(*[bufs[k].ctypes.data if k < pairs else None for k in range(4)])
                t0 = time.perf_counter()
                for i in range(n):
                    H.mi_dv_extract_audio(prof, host[i * fb:].ctypes.data, arr)
                cpu_ms = (time.perf_counter() - t0) * 1e3
            finally:
                for d in (df, dp, ds, di):
                    dev.free(d)
            payload = s.chans * s.seqs * 9
            ex_bytes, wr_bytes = n * (payload * 72 + pairs * A.PAIR_BYTES + 16), n * (payload * 80 + s.chans * A.PAIR_BYTES + 4)
            em, wm = statistics.median(ex), statistics.median(wr)
            line = {"tool": "bench_dv_audio", "system": name, "frames": n, "pairs": pairs, "steps": a.steps, "warmup": a.warmup,
                    "extract_ms_median": round(em, 4), "extract_ms_min": round(min(ex), 4), "extract_ms_max": round(max(ex), 4),
                    "extract_gbytes_per_s": round(ex_bytes / (em / 1e3) / 1e9, 1),
                    "extract_share_of_8tb_s": round(ex_bytes / (em / 1e3) / HBM_BYTES_PER_S, 4),
                    "write_ms_median": round(wm, 4), "write_ms_min": round(min(wr), 4), "write_ms_max": round(max(wr), 4),
                    "write_gbytes_per_s": round(wr_bytes / (wm / 1e3) / 1e9, 1),
                    "write_share_of_8tb_s": round(wr_bytes / (wm / 1e3) / HBM_BYTES_PER_S, 4),
                    "host_extract_one_core_ms": round(cpu_ms, 3), "frames_d2h_ms_median": round(statistics.median(copy), 3),
                    "decode_ms_median": round(statistics.median(dec), 4), "byte_exact_first_frame": exact, "parity": "unpinned"}
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
