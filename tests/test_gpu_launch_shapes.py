"""The launch shapes of the batch transform against the oracle: how k_decode_split, k_decode (span 3 and span 1) and
k_decode_list divide a picture among waves is computed per plan from its macroblock-group count
(tests/launch_shapes.py restates it, tests/test_launch_shapes_cpu.py pins that to the headers); a rounding slip there
leaves a group, a part of one or the tail of a partial one undecoded, or decoded by two waves, and nothing crashes.
Every picture of every launch here is compared with the oracle byte for byte, in outputs prefilled with two different
bytes, with guard bytes between the pictures.  Integer work: equality, no tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest

import launch_shapes as LS
import rtjlib as R
import test_gpu_parity as T
from pkg import P

pytestmark = pytest.mark.gpu

S = LS.Shapes()
CLASSES = S.geometry_classes()
GUARD = 256
PREFILLS = (0x00, 0xA5)


def forms(groups):
    """name -> (environment of the plan, what plan.decode_form() must say ran)"""
    return {
        "split": (dict(MI_RTJ_ROTATE="1", MI_RTJ_SPLIT="1"), 0),
        "classic": (dict(MI_RTJ_ROTATE="1", MI_RTJ_SPLIT="0"), 1),
        "span1": (dict(MI_RTJ_ROTATE="0"), -1),
        # small batches get a wave per group; the fewest waves the kernel allows make every wave run kDecIters rounds
        "classic-fewest-slots": (dict(MI_RTJ_ROTATE="1", MI_RTJ_SPLIT="0",
                                      MI_RTJ_DEC_SLOTS=str((groups + S.kDecIters - 1) // S.kDecIters)), 1),
    }


def header(w, h, Q, total):
    return np.array([total & 255, (total >> 8) & 255, (total >> 16) & 255, (total >> 24) & 255, 12, 0,
                     w & 255, w >> 8, h & 255, h >> 8, Q, 0], np.uint8)


KINDS = ("quiet", "noisy", "quiet", "noisy", "arbitrary", "quiet", "noisy", "truncated", "quiet")  # nine: every stripe rotation


def make_packets(w, h, kinds=KINDS, seed=0):
    """quiet: amplitude 8 at Q 255 (the pooling chroma waves' content); noisy: amplitude 48 at Q 255 (most chroma parts
    go to k_decode_list); one packet of arbitrary bytes; one cut short."""
    def one(ik):
        i, kind = ik
        if kind == "arbitrary":
            rng = np.random.default_rng(1000 * seed + i)
            n = (w // 16) * (h // 16) * 6 * 24
            return np.concatenate([header(w, h, 255, 12 + n), rng.integers(0, 256, n, dtype=np.uint8)])
        amp = 48 if kind == "noisy" else 8
        p = R.OracleEncoder(w, h, 255).encode(R.synth_frame(w, h, i, seed=40 + seed, amp=amp))
        return p[: 12 + (p.size - 12) * 3 // 5].copy() if kind == "truncated" else p
    return T.pmap(one, enumerate(kinds))


def oracle_pictures(pkts, prefill):
    def one(p):
        want = np.full(T.frame_bytes(*T.packet_size(p)), prefill, np.uint8)
        R.OracleDecoder().decode(p, want)
        return want
    return T.pmap(one, pkts)


def compare(outs, wants, pkts, cls, form, prefill, kinds=None, max_groups=None, **model):
    for i, (got, want) in enumerate(zip(outs, wants)):
        if np.array_equal(got, want):
            continue
        w, h = T.packet_size(pkts[i])
        d = np.nonzero(got != want)[0]
        off = int(d[0])
        where = S.describe_byte(w, h, off, "split" if form.startswith("split") else "classic" if form.startswith("classic") else "span1",
                                frame=i, frames=len(pkts), max_groups=max_groups, **model)
        raise AssertionError(f"class {cls} ({w}x{h}, {S.groups(w, h)} groups), form {form}, prefill {prefill:#04x}, picture {i}"
                             f"{' (' + kinds[i] + ')' if kinds else ''}: {d.size} bytes differ from the oracle, first at byte {off}: "
                             f"got {int(got[off])} want {int(want[off])}; {where}")


def run_form(dev, monkeypatch, pkts, wants, cls, form, env, expect_form, prefill, kinds=None, max_groups=None, launches=1):
    with monkeypatch.context() as m:
        for k in ("MI_RTJ_ROTATE", "MI_RTJ_SPLIT", "MI_RTJ_DEC_SLOTS"):
            m.delenv(k, raising=False)
        for k, v in env.items():
            m.setenv(k, v)
        rep = {}
        outs = T.batch_decode(dev, pkts, prefill=prefill, align=1, guard=GUARD, odd16=True, report=rep, launches=launches)
    assert rep["form"] == expect_form, f"class {cls}, form {form}: the plan ran form {rep['form']}, not {expect_form}"
    assert any(int(o) % 256 for o in rep["out_offsets"]) and all(int(o) % 16 == 0 for o in rep["out_offsets"])
    compare(outs, wants, pkts, cls, form, prefill, kinds, max_groups, slots=int(env.get("MI_RTJ_DEC_SLOTS", 0)) or None)
    return rep


@pytest.fixture(scope="module")
def dev():
    d = P.MiRtj()
    yield d
    d.close()


# --------------------------------------------------------------------------- 2. the geometry sweep
@pytest.mark.parametrize("cls,w,h", CLASSES, ids=[c[0] for c in CLASSES])
def test_geometry_class(dev, monkeypatch, cls, w, h):
    groups = S.groups(w, h)
    pkts = make_packets(w, h)
    noisy = [p for p, k in zip(pkts, KINDS) if k == "noisy"]
    for prefill in PREFILLS:
        wants = oracle_pictures(pkts, prefill)
        for form, (env, expect) in forms(groups).items():
            rep = run_form(dev, monkeypatch, pkts, wants, cls, form, env, expect, prefill, KINDS)
            if form == "split":
                # some chroma parts take the pooling waves' short forms, some go to the list
                assert 0 < rep["parts_listed"] < 3 * groups * len(pkts), (cls, rep)
        # the noisy pictures alone: their chroma is what k_decode_list is for
        nw = [wt for wt, k in zip(wants, KINDS) if k == "noisy"]
        rep = run_form(dev, monkeypatch, noisy, nw, cls, "split (noisy pictures alone)", *forms(groups)["split"], prefill)
        assert rep["parts_listed"] > 0, (cls, rep)


def mixed_plan():
    """24 pictures of six classes in one plan; the largest, which sets the launch's max_groups, first, in the middle
    and last, so that every other picture leaves surplus waves idle"""
    by = {}
    for n, w, h in CLASSES:
        for part in n.split("__"):
            by[part] = (w, h)
    big = by["per-xcd-pool-iters-max+1"]
    small = [by["1-group"], by["2-super-groups"], by[f"{S.kXcds + 1}-super-groups"],
             by[f"groups-{S.kPoolGroups}k+1-last-{S.kMbPerGroup - 1}mb"], by["640x368"], by["strip-narrow"], by["strip-wide"]]
    dims, kinds = [], []
    for i in range(24):
        dims.append(big if i in (0, 12, 23) else small[i % len(small)])
        kinds.append(("quiet", "noisy", "quiet", "arbitrary", "noisy", "truncated")[i % 6])
    assert len(set(dims)) >= 4 and S.groups(*big) == max(S.groups(*d) for d in dims)
    pkts = [None] * len(dims)
    for d in set(dims):  # (one encoder run per geometry)
        idx = [i for i in range(len(dims)) if dims[i] == d]
        made = make_packets(d[0], d[1], [kinds[i] for i in idx], seed=7)
        for i, p in zip(idx, made):
            pkts[i] = p
    return dims, kinds, pkts


def test_mixed_plan_leaves_surplus_waves_idle(dev, monkeypatch):
    dims, kinds, pkts = mixed_plan()
    mg = max(S.groups(*d) for d in dims)
    for prefill in PREFILLS:
        wants = oracle_pictures(pkts, prefill)
        for form in ("split", "classic", "span1"):
            env, expect = forms(mg)[form]
            run_form(dev, monkeypatch, pkts, wants, "mixed plan", form, env, expect, prefill, kinds, max_groups=mg)


# --------------------------------------------------------------------------- 3. the headline geometries, every picture
def device_batch(dev, w, h, n, amp=8, seed=12345):
    """n pictures generated and encoded on the device (the encoder is pinned to the oracle's bytes by
    tests/test_gpu_parity.py): stream buffer, packet offsets and lengths, headers, and the packets on the host"""
    d_fr = dev.synth(w, h, 0, n, seed=seed, amp=amp)
    d_st, po, pl = dev.encode(w, h, 255, n, d_fr)
    dev.sync()
    dev.free(d_fr)
    end = int(po[-1]) + int(pl[-1])
    host = dev.d2h(d_st, end)
    pkts = [host[int(po[i]):int(po[i]) + int(pl[i])] for i in range(n)]
    hdrs = np.stack([p[:12] for p in pkts])
    return d_st, po, pl, hdrs, pkts


@pytest.mark.parametrize("w,h", [(3840, 2176), (3840, 2160)])
def test_4k_batches_every_picture(dev, monkeypatch, w, h):
    """the bench's 4K coded size and 3840x2160 (four chroma waves per XCD), 40 pictures: span 3 by the size of the batch"""
    n = 40
    groups = S.groups(w, h)
    assert S.span(n, groups) == 3
    fsz = T.frame_bytes(w, h)
    d_st, po, pl, hdrs, pkts = device_batch(dev, w, h, n)
    want = T.oracle_digests(pkts)
    d_out = dev.alloc(fsz * n)
    oo = np.arange(n, dtype=np.uint64) * np.uint64(fsz)
    for form, split, expect in (("split", "1", 0), ("classic", "0", 1)):
        with monkeypatch.context() as m:
            m.delenv("MI_RTJ_ROTATE", raising=False)
            m.setenv("MI_RTJ_SPLIT", split)
            plan = dev.plan(hdrs, po, pl, oo)
        for fill in PREFILLS:
            dev.memset(d_out, fill, fsz * n)
            plan.decode(d_st, d_out)
            dev.sync()
            assert plan.decode_form()[0] == expect, (form, plan.decode_form())
            got = T.device_digests(dev, d_out, fsz, n)
            for k in range(n):
                assert got[k] == want[k], T.explain_picture(dev, d_out, fsz, k, pkts[k], f"{w}x{h}", form, n, form == "split")
        plan.close()
    dev.free(d_st)
    dev.free(d_out)


def test_1080p_overlapped_launches_back_to_back_every_picture(dev, monkeypatch):
    """129 pictures of 1080p: the smallest plan whose index runs on the plan's own stream next to the previous launch's
    transform.  Three launches without a sync in between; every picture of the last one is compared."""
    w, h = 1920, 1088
    groups = S.groups(w, h)
    n = (S.kDecRotateMinGroups + groups - 1) // groups
    for k in ("MI_RTJ_ROTATE", "MI_RTJ_SPLIT", "MI_RTJ_OVERLAP"):
        monkeypatch.delenv(k, raising=False)
    fsz = T.frame_bytes(w, h)
    d_st, po, pl, hdrs, pkts = device_batch(dev, w, h, n, seed=777)
    want = T.oracle_digests(pkts)
    d_out = dev.alloc(fsz * n)
    plan = dev.plan(hdrs, po, pl, np.arange(n, dtype=np.uint64) * np.uint64(fsz))
    dev.memset(d_out, 0xA5, fsz * n)
    for _ in range(3):
        plan.decode(d_st, d_out)
    assert plan.overlapped()
    dev.sync()
    form = plan.decode_form()[0]
    assert form in (0, 1)
    got = T.device_digests(dev, d_out, fsz, n)
    for k in range(n):
        assert got[k] == want[k], T.explain_picture(dev, d_out, fsz, k, pkts[k], "1080p x %d overlapped" % n, "policy", n, form == 0)
    plan.close()
    dev.free(d_st)
    dev.free(d_out)


# --------------------------------------------------------------------------- 4. wave counts and rotation do not matter
EXPERIMENT_CLASSES = ("640x368", "per-xcd-pool-iters-max", "per-xcd-pool-iters-max+1")


def experiments_child(names):
    """Runs in a process of its own with MI_RTJ_LIB naming the experiments build: the classes `names` of the sweep in the
    split form under every stripe rotation and under every pair of wave counts from 1 to one more than the computed
    ones.  Both kinds of wave loop over their stripe until the picture ends (tests/test_launch_shapes_cpu.py), so every
    pair covers the picture and every pair is compared."""
    import ctypes as C
    lib = P.binding.load()
    assert hasattr(lib, "mi_rtj_debug_pool_stamps"), "not the experiments build: MI_RTJ_LUMA_WAVES and its kin would be ignored"
    lib.mi_rtj_debug_pool_stamps.argtypes = [C.POINTER(C.c_ulonglong)]
    stamps = (C.c_ulonglong * 16)()
    by = {}
    for n, w, h in CLASSES:
        for part in n.split("__"):
            by[part] = (w, h)
    os.environ["MI_RTJ_ROTATE"], os.environ["MI_RTJ_SPLIT"] = "1", "1"
    dev = P.MiRtj()
    prefill, runs = 0xA5, 0
    for cls in names:
        w, h = by[cls]
        g = S.groups(w, h)
        nsg, lw0, cw0 = S.super_groups(g), S.split_luma_waves(g), S.split_chroma_waves(g)
        pkts = make_packets(w, h, seed=3)
        wants = oracle_pictures(pkts, prefill)
        cases = [(None, None, rot) for rot in range(8)]
        cases += [(lw, cw, None) for lw in range(1, lw0 + 2) for cw in range(1, cw0 + 2)]
        cases += [(lw0 + 1, cw0 + 1, 3), (1, 1, 7)]
        for lw, cw, rot in cases:
            for k, v in (("MI_RTJ_LUMA_WAVES", lw), ("MI_RTJ_CHROMA_WAVES", cw), ("MI_RTJ_XCD_ROT", rot)):
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = str(v)
            assert lib.mi_rtj_debug_pool_stamps(stamps) == 0  # (clears the counters)
            rep = {}
            outs = T.batch_decode(dev, pkts, prefill=prefill, align=1, guard=GUARD, odd16=True, report=rep, check_index=False)
            assert rep["form"] == 0, rep
            # the switch was honoured: stamp 7 counts the pooling chroma waves that had a stripe to work on
            assert lib.mi_rtj_debug_pool_stamps(stamps) == 0
            assert stamps[7] == len(pkts) * min(S.kXcds * (cw or cw0), nsg), (cls, lw, cw, rot, stamps[7])
            compare(outs, wants, pkts, cls, f"split lw={lw or lw0} cw={cw or cw0} rot={S.kSplitXcdRot if rot is None else rot}",
                    prefill, KINDS, rot=rot, lw=lw, cw=cw)
            runs += 1
    dev.close()
    print(f"experiments ok {runs} launches")


def test_wave_counts_and_rotation_do_not_matter():
    bld = __import__("importlib").import_module("gmerlin-avdecoder_amd.build")
    try:
        lib = bld.build_experiments()  # built by __graft_entry__.build(); rebuilt here only if missing or stale
    except (RuntimeError, OSError) as e:
        pytest.skip(f"the experiments build cannot be built here: {str(e)[:200]}")
    env = dict(os.environ, MI_RTJ_LIB=lib)
    for k in ("MI_RTJ_SPLIT_ONLY", "MI_RTJ_DEC_SLOTS", "MI_RTJ_OVERLAP"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--experiments", *EXPERIMENT_CLASSES], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "experiments ok" in r.stdout, r.stdout[-2000:] + r.stderr[-6000:]


if __name__ == "__main__":
    assert sys.argv[1] == "--experiments"
    experiments_child(sys.argv[2:])
