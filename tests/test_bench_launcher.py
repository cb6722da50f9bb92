"""bench.py --gpus N starts its own ranks when no launcher did, and refuses to report a run whose world size is not
N (round 1's bench.py silently ran one rank for --gpus 8).  The CPU tests use --selftest-ranks (every rank sends a
dummy shard through the real reduction, gloo, no GPU); the gpu tests run the real workloads with two ranks sharing
the box's one device (MI_RTJ_SHARE_DEVICE=1, reduction over gloo) and the other two bench configurations at small
sizes.  The frames1080 line carries its parity and CPU fields only with --full; a plain run is the headline alone."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from pkg import ROOT

BENCH = os.path.join(ROOT, "bench.py")


def run_bench(args, env=None, timeout=600):
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, env=e, timeout=timeout)


def last_json(r):
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert lines, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(lines[-1])


def test_gpus_2_without_a_launcher_starts_two_ranks():
    r = run_bench(["--gpus", "2", "--selftest-ranks"])
    assert r.returncode == 0, r.stderr[-3000:]
    d = last_json(r)
    assert d["n_gpus"] == 2 and d["frames"] == 10 + 11 and abs(d["elapsed"] - 2.0) < 1e-9  # SUM of frames, MAX of elapsed


def test_world_size_that_differs_from_gpus_is_an_error():
    r = run_bench(["--gpus", "2", "--selftest-ranks"], env={"WORLD_SIZE": "1", "RANK": "0"})
    assert r.returncode != 0 and "refusing" in (r.stderr + r.stdout)
    r = run_bench(["--gpus", "1", "--selftest-ranks"], env={"WORLD_SIZE": "2", "RANK": "0", "MASTER_ADDR": "127.0.0.1",
                                                             "MASTER_PORT": "29999"})
    assert r.returncode != 0 and "refusing" in (r.stderr + r.stdout)


SHARE = {"MI_RTJ_DIST_BACKEND": "gloo", "MI_RTJ_SHARE_DEVICE": "1"}


@pytest.mark.gpu
def test_two_ranks_on_one_box_report_two_gpus():
    """the N > 1 line carries its own evidence: every rank compares a sample of its own output with the CPU decoder
    (parity_checked = N x sample, through the path's one reduction), rank 0 times the CPU baseline"""
    r = run_bench(["--full", "--gpus", "2", "--frames", "128", "--steps", "3", "--warmup", "1", "--verify-frames", "32",
                   "--cpu-seconds", "1", "--no-stress", "--no-e2e"], env=SHARE)
    assert r.returncode == 0, r.stderr[-3000:]
    d = last_json(r)
    assert d["n_gpus"] == 2 and d["config"]["frames_per_gpu"] == 128 and d["value"] > 0
    assert d["parity_checked"] == 2 * 32 and d["parity_sample_per_rank"] == 32 and d["parity_mismatches"] == 0
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["cores"] == 1
    assert d["cpu_baseline_all_cores"]["value"] > 0
    assert d["roofline"]["frac"] > 0


def test_selftest_reduction_carries_the_frames_compared():
    """(CPU, gloo) the reduction sums what every rank compared"""
    sys.path.insert(0, ROOT)
    import importlib
    shard = importlib.import_module("gmerlin-avdecoder_amd.shard")
    rep = shard.reduce_report(shard.Report(10, 1000, 1, 2.0, 32))
    assert (rep.frames, rep.pixels, rep.mismatches, rep.elapsed, rep.checked) == (10, 1000, 1, 2.0, 32)


@pytest.mark.gpu
def test_one_rank_line_checks_every_sampled_frame_and_carries_the_extras():
    r = run_bench(["--full", "--frames", "512", "--steps", "3", "--warmup", "1", "--cpu-seconds", "1", "--verify-frames", "64"])
    assert r.returncode == 0, r.stderr[-3000:]
    d = last_json(r)
    assert d["parity_checked"] == 64 and d["parity_mismatches"] == 0
    assert set(d["by_batch"]) >= {"256", "512"} and d["by_batch"]["256"]["frames_per_s"] > 0
    assert "k_synth" in d["config"]["workload"]
    assert d["cpu_baseline"]["cores"] == 1 and d["cpu_baseline_all_cores"]["cores"] >= 1
    assert d["median_step"]["device_ms"] > 0 and d["roofline"]["frac"] > 0
    assert d["kernels"]["k_decode"]["gbs"] > 0
    for k, v in d["kernels"].items():  # kernels that served an empty to-do list claim no bandwidth
        assert v["gbs"] is None or v["ms"] > 0.05, k
    assert d["end_to_end"].get("fps", 0) > 0 and d["stress_amp64"]["frames_per_s"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,extra", [("streams4k", ["--frames", "8", "--steps", "2", "--warmup", "1"]),
                                        ("mixed", ["--frames", "1", "--steps", "2", "--warmup", "1"])])
def test_other_bench_configurations(cfg, extra):
    for gpus in (1, 2):
        r = run_bench(["--gpus", str(gpus), "--config", cfg] + extra, env=SHARE if gpus > 1 else None)
        assert r.returncode == 0, r.stderr[-3000:]
        d = last_json(r)
        assert d["n_gpus"] == gpus and d["parity_mismatches"] == 0 and d["parity_checked"] > 0 and d["value"] > 0
        assert d["roofline"]["frac"] >= 0 and d["roofline"]["kernel"] and d["cpu_baseline"]["value"] > 0
        if cfg == "streams4k":  # the whole first lap of every stream is compared (8 packets here)
            assert d["parity_checked"] == 8 * gpus
        assert cfg.replace("streams4k", "3840x2160").replace("mixed", "mixed") in d["metric"] or cfg == "mixed"


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _HostOutputs:
    """stands in for MiRtj.d2h over an output buffer of n pictures (no GPU)"""

    def __init__(self, buf):
        self.buf = buf

    def d2h(self, dptr, nbytes, offset=0):
        return self.buf[dptr + offset:dptr + offset + nbytes].copy()


def _dump(bench, tmp, buf, n, w, h, stride):
    bench.dump_outputs(str(tmp), _HostOutputs(buf), 0, n, w, h, stride)
    return {f: np.load(os.path.join(tmp, f)) for f in sorted(os.listdir(tmp))}


def test_dump_outputs_writes_a_fixed_sample_of_whole_pictures(tmp_path):
    """(CPU) --dump-outputs: float32 planes of seeded pictures, the same ones every run, inside the size budget"""
    bench = _bench_module()
    n, w, h, pad = 40, 64, 32, 16
    fsz = w * h * 3 // 2
    buf = np.random.default_rng(1).integers(0, 256, n * (fsz + pad), dtype=np.uint8)
    got = _dump(bench, tmp_path / "a", buf, n, w, h, fsz + pad)
    assert len(got) == 3 * bench.DUMP_PICTURES
    for name, arr in got.items():
        i, plane = int(name[3:8]), name[9]
        assert arr.dtype == np.float32 and name.endswith(".npy")
        pic = buf[i * (fsz + pad):i * (fsz + pad) + fsz]
        want = {"y": pic[:w * h].reshape(h, w), "u": pic[w * h:w * h * 5 // 4].reshape(h // 2, w // 2),
                "v": pic[w * h * 5 // 4:].reshape(h // 2, w // 2)}[plane]
        assert np.array_equal(arr, want.astype(np.float32)), name
    again = _dump(bench, tmp_path / "b", buf, n, w, h, fsz + pad)
    assert sorted(again) == sorted(got) and all(np.array_equal(again[k], got[k]) for k in got)


def test_dump_outputs_stays_inside_its_budget(tmp_path):
    """(CPU) pictures larger than the budget keep their top rows, whole rows of every plane"""
    bench = _bench_module()
    bench.DUMP_BYTES = 1 << 16
    n, w, h = 3, 128, 128
    fsz = w * h * 3 // 2
    buf = np.arange(n * fsz, dtype=np.uint64).astype(np.uint8)
    got = _dump(bench, tmp_path, buf, n, w, h, fsz)
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_BYTES
    ys = [a for k, a in got.items() if k.endswith("_y.npy")]
    assert len(ys) == 1 and 0 < ys[0].shape[0] < h and ys[0].shape[1] == w
    assert np.array_equal(ys[0], buf[int(next(iter(got))[3:8]) * fsz:][:ys[0].size].reshape(-1, w).astype(np.float32))


def test_dump_outputs_is_refused_where_it_is_not_implemented():
    r = run_bench(["--config", "dv", "--dump-outputs", "unused"])
    assert r.returncode != 0 and "frames1080" in r.stderr


@pytest.mark.gpu
def test_plain_line_is_the_headline_and_dumps_the_last_step(tmp_path):
    """a plain run times exactly --steps steps, leaves the --full fields out, and --dump-outputs writes the pictures
    of the last step: equal from run to run, and equal to the CPU decoder's planes of the same packets"""
    args = ["--frames", "64", "--steps", "4", "--warmup", "1"]
    r = run_bench(args + ["--dump-outputs", str(tmp_path / "a")])
    assert r.returncode == 0, r.stderr[-3000:]
    d = last_json(r)
    assert d["steps"] == 4 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "frames/s"
    for k in ("cpu_baseline", "parity_checked", "by_batch", "end_to_end", "stress_amp64", "copy_ceiling_gbs"):
        assert k not in d, k
    a = sorted(os.listdir(tmp_path / "a"))
    assert len(a) == 12 and all(f.endswith(".npy") for f in a)
    r = run_bench(args + ["--dump-outputs", str(tmp_path / "b")])
    assert r.returncode == 0, r.stderr[-3000:]
    assert sorted(os.listdir(tmp_path / "b")) == a
    for f in a:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float32 and np.array_equal(x, y), f
    # the pictures are the CPU decoder's: the dumped frames re-made on the host, encoded and decoded by the oracle
    import rtjlib as R
    w, h = 1920, 1088
    for i in sorted({int(f[3:8]) for f in a}):
        pkt = R.OracleEncoder(w, h, 255).encode(R.synth_frame_lcg(w, h, i, seed=12345, amp=8))
        want = np.zeros(w * h * 3 // 2, np.uint8)
        R.OracleDecoder().decode(pkt, want)
        y, u, v = R.split_planes(want, w, h)
        assert np.array_equal(np.load(tmp_path / "a" / f"pic{i:05d}_y.npy"), y.reshape(h, w).astype(np.float32))
        assert np.array_equal(np.load(tmp_path / "a" / f"pic{i:05d}_u.npy"), u.reshape(h // 2, w // 2).astype(np.float32))
        assert np.array_equal(np.load(tmp_path / "a" / f"pic{i:05d}_v.npy"), v.reshape(h // 2, w // 2).astype(np.float32))
