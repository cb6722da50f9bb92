"""Runs on 4:2:2 and greyscale plans on the device (mi_rtj_plan_set_runs_fmt): one launch decodes streams with
unchanged blocks, bit for bit the in-order decode of the restatement (tests/runlib_fmt.py, which
tests/test_fmt_runs_cpu.py holds to the reference), and the copied-block count is the restatement's.  Slots of pictures
k > 0 start as 0x5A, so a block nobody copied shows.  Run on the GPU box with `pytest -m gpu`."""
import numpy as np
import pytest

import rtjfmt as F
import runlib as RL
import runlib_fmt as RF
from pkg import P

pytestmark = pytest.mark.gpu

FMTS = (F.FMT_422, F.FMT_GREY)
FILL = RF.FILL
SMALL = {F.FMT_422: (48, 24), F.FMT_GREY: (24, 8)}     # less than one copy tile
WRAP = {F.FMT_422: (176, 40), F.FMT_GREY: (136, 72)}   # tiles that wrap picture rows, a partial last tile
QK = [(200, 4), (90, 1), (255, 255)]


@pytest.fixture(scope="module")
def devs():
    d = {}
    for fmt in FMTS:
        d[fmt] = P.MiRtj()
        d[fmt].set_format(fmt)
    yield d
    for x in d.values():
        x.close()


def first_diff(a, b):
    d = np.nonzero(a != b)[0]
    return None if d.size == 0 else (int(d[0]), int(a[d[0]]), int(b[d[0]]), int(d.size))


def check(got, want, what=""):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert first_diff(a, b) is None, (what, i, first_diff(a, b))


class Batch:
    """Packets uploaded once, one output slot each; picture 0 of every run prefilled with prev[r], the rest with FILL."""

    def __init__(self, dev, fmt, pkts, runs, prev, align=1, pad=256):
        self.dev, self.pkts, self.runs, self.prev = dev, pkts, runs, prev
        self.d_stream, po, pl, hdrs = dev.upload_packets(pkts, align=align)
        self.sizes = [F.plane_bytes(fmt, *RF.dims(p)) for p in pkts]
        self.oo = np.zeros(len(pkts), np.uint64)
        cur = 0
        for i, s in enumerate(self.sizes):
            self.oo[i] = cur
            cur += (s + pad - 1) // pad * pad
        self.total = cur
        self.d_out = dev.alloc(cur)
        self.plan = dev.plan(hdrs, po, pl, self.oo)
        assert self.plan.fmt == fmt

    def prefill(self):
        self.dev.memset(self.d_out, FILL, self.total)
        i = 0
        for r, n in enumerate(self.runs):
            self.dev.h2d(self.d_out, self.prev[r], offset=int(self.oo[i]))
            i += n

    def decode(self, prefill=True):
        if prefill:
            self.prefill()
        self.plan.decode(self.d_stream, self.d_out)
        self.dev.sync()
        whole = self.dev.d2h(self.d_out, self.total)
        pics = [whole[int(self.oo[i]):int(self.oo[i]) + s] for i, s in enumerate(self.sizes)]
        gaps = [whole[int(self.oo[i]) + s:int(self.oo[i + 1]) if i + 1 < len(self.sizes) else self.total]
                for i, s in enumerate(self.sizes)]
        assert all(np.all(g == FILL) for g in gaps), "bytes between the output slots were written"
        return pics

    def close(self):
        self.plan.close()
        self.dev.free(self.d_stream)
        self.dev.free(self.d_out)


def decode_runs(dev, fmt, pkts, runs, prev, **kw):
    b = Batch(dev, fmt, pkts, runs, prev, **kw)
    b.plan.set_runs_fmt(runs)
    got = b.decode()
    copied = b.plan.run_copied()
    b.close()
    return got, copied


def against_restatement(dev, fmt, pkts, runs, prev, what="", **kw):
    """the device's pictures and copied-block count against the in-order decode and the rule's count"""
    got, copied = decode_runs(dev, fmt, pkts, runs, prev, **kw)
    check(got, RF.in_order(fmt, pkts, runs, prev), what)
    want, n = RF.by_rule(fmt, pkts, runs, prev)
    check(got, want, ("rule", what))
    assert copied == n, (what, copied, n)
    return got


@pytest.mark.parametrize("fmt", FMTS)
def test_golden_key_rate_sequences_as_one_run(devs, fmt):
    cases = [c for c in F.golden_cases(F.load_golden()) if c[0] == fmt and c[4] > 0]
    assert cases
    for _, w, h, Q, key, pkts, outs in cases:
        n = len(pkts)
        assert RF.has_both_kinds(fmt, pkts, [n])
        prev = [np.full(F.plane_bytes(fmt, w, h), 77, np.uint8)]
        got, copied = decode_runs(devs[fmt], fmt, pkts, [n], prev)
        check(got, outs, (w, h, Q, key))
        assert copied == RF.by_rule(fmt, pkts, [n], prev)[1] > 0


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("shape", ("small", "wrap"))
@pytest.mark.parametrize("Q,kr", QK)
def test_encoder_streams(devs, fmt, shape, Q, kr):
    w, h = (SMALL if shape == "small" else WRAP)[fmt]
    pkts = F.make_packets(fmt, w, h, Q, 9, seed=3, key_rate=kr, lmask=2, cmask=2)
    assert RF.has_both_kinds(fmt, pkts, [9])
    against_restatement(devs[fmt], fmt, pkts, [9], [RF.rand_pic(fmt, w, h, Q)], (w, h, Q, kr))


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 128, 129])
def test_runs_around_the_scan_chunk(devs, fmt, n):
    w, h = SMALL[fmt]
    pkts = RF.crafted_run(fmt, n, w, h, seed=n)
    assert n == 1 or RF.has_both_kinds(fmt, pkts, [n])  # (a run of one picture has no picture k > 0)
    against_restatement(devs[fmt], fmt, pkts, [n], [RF.rand_pic(fmt, w, h, n)], n)


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("align", [1, 64])
def test_several_runs_sizes_and_qualities(devs, fmt, align):
    a, b = SMALL[fmt], WRAP[fmt]
    c = (320, 88)
    pkts, runs, prev = [], [], []
    for j, ((w, h), Q, n, kr) in enumerate([(b, 200, 5, 4), (a, 90, 1, 1), (c, 255, 7, 255), (a, 30, 1, 3),
                                            (b, 120, 3, 2), (a, 90, 4, 1)]):
        pkts += F.make_packets(fmt, w, h, Q, n, seed=3 + j, key_rate=kr, lmask=2, cmask=2)
        runs.append(n)
        prev.append(RF.rand_pic(fmt, w, h, j))
    assert RF.has_both_kinds(fmt, pkts, runs)
    against_restatement(devs[fmt], fmt, pkts, runs, prev, align=align, pad=256)


@pytest.mark.parametrize("fmt", FMTS)
def test_quality_change_inside_a_run(devs, fmt):
    w, h = WRAP[fmt]
    pkts = F.make_packets(fmt, w, h, 200, 4, seed=3, key_rate=4) + F.make_packets(fmt, w, h, 60, 4, seed=3, key_rate=4) + \
        F.make_packets(fmt, w, h, 255, 3, seed=4, key_rate=2, lmask=8, cmask=8)
    assert RF.has_both_kinds(fmt, pkts, [len(pkts)])
    against_restatement(devs[fmt], fmt, pkts, [len(pkts)], [RF.rand_pic(fmt, w, h, 5)])


@pytest.mark.parametrize("fmt", FMTS)
def test_device_round_trip(devs, fmt):
    """pictures encoded on the device as one stream (mi_rtj_encode_stream_fmt), then decoded as one run"""
    dev = devs[fmt]
    w, h = WRAP[fmt]
    n = 8
    pics = F.make_stream(fmt, w, h, n, seed=9, amp=8)
    d_fr = dev.alloc(F.plane_bytes(fmt, w, h) * n)
    dev.h2d(d_fr, np.concatenate(pics))
    d_st, po, pl = dev.encode(w, h, 200, n, d_fr, align=1, key_rate=4, lmask=2, cmask=2, fmt=fmt)
    dev.sync()
    pkts = [dev.d2h(d_st, int(pl[i]), offset=int(po[i])) for i in range(n)]
    dev.free(d_fr)
    dev.free(d_st)
    assert RF.has_both_kinds(fmt, pkts, [n])
    against_restatement(dev, fmt, pkts, [n], [RF.rand_pic(fmt, w, h, 1)])


@pytest.mark.parametrize("fmt", FMTS)
def test_repeat_and_reset(devs, fmt):
    dev = devs[fmt]
    w, h = WRAP[fmt]
    pkts = F.make_packets(fmt, w, h, 200, 9, seed=3, key_rate=4)
    assert RF.has_both_kinds(fmt, pkts, [9])
    prev = [RF.rand_pic(fmt, w, h, 8)]
    b = Batch(dev, fmt, pkts, [9], prev)
    b.plan.set_runs_fmt([9])
    first = b.decode()
    n1 = b.plan.run_copied()
    again = b.decode()
    check(again, first, "repeat")
    assert b.plan.run_copied() == n1 > 0
    check(first, RF.in_order(fmt, pkts, [9], prev))
    # set_runs still refuses such a plan, and the plan keeps its runs
    with pytest.raises(P.MiRtjError, match="rc=-3: .*4:2:0"):
        b.plan.set_runs([9])
    check(b.decode(), first, "after set_runs' refusal")
    b.plan.set_runs_fmt([])
    plain = b.decode()
    assert b.plan.run_copied() == 0
    check(plain, RF.independent(fmt, pkts, prev, [9]), "independent pictures")
    b.close()


def test_set_runs_fmt_on_a_420_plan_is_set_runs():
    dev = P.MiRtj()
    w, h = 64, 48
    pkts = RL.stream_packets(w, h, 200, 9, 4, 2, 2, seed=8)
    prev = [np.random.default_rng(8).integers(0, 256, RL.frame_bytes(w, h), dtype=np.uint8)]
    d_st, po, pl, hdrs = dev.upload_packets(pkts)
    fsz = RL.frame_bytes(w, h)
    d_out = dev.alloc(9 * fsz)
    plan = dev.plan(hdrs, po, pl, np.arange(9, dtype=np.uint64) * fsz)
    res = []
    for setter in (plan.set_runs, plan.set_runs_fmt):
        plan.set_runs_fmt([])
        setter([9])
        dev.memset(d_out, FILL, 9 * fsz)
        dev.h2d(d_out, prev[0])
        plan.decode(d_st, d_out)
        dev.sync()
        res.append((dev.d2h(d_out, 9 * fsz), plan.run_copied()))
    assert first_diff(res[0][0], res[1][0]) is None and res[0][1] == res[1][1] > 0
    assert first_diff(res[1][0], np.concatenate(RL.oracle_in_order(pkts, [9], prev))) is None
    with pytest.raises(P.MiRtjError, match="mi_rtj_plan_set_runs_fmt"):
        plan.set_runs_fmt([4, 4])
    plan.close()
    dev.free(d_st)
    dev.free(d_out)
    dev.close()


@pytest.mark.parametrize("fmt", FMTS)
def test_refusals_leave_the_plan_decoding(devs, fmt):
    dev = devs[fmt]
    a, s = WRAP[fmt], SMALL[fmt]
    pkts = F.make_packets(fmt, *a, 90, 4, seed=2, key_rate=1) + F.make_packets(fmt, *s, 90, 3, seed=2, key_rate=1)
    prev = [RF.rand_pic(fmt, *a, 1), RF.rand_pic(fmt, *s, 2)]
    b = Batch(dev, fmt, pkts, [4, 3], prev)
    b.plan.set_runs_fmt([4, 3])
    for bad in ([4, 2], [4, 4], [4, 0, 3], [4, -1, 4], [3, 4], [7]):  # sums, lengths, size change inside a run
        with pytest.raises(P.MiRtjError, match="rc=-3: mi_rtj_plan_set_runs_fmt"):
            b.plan.set_runs_fmt(bad)
    check(b.decode(), RF.in_order(fmt, pkts, [4, 3], prev), "after refusals")
    b.close()
    # output pictures of a run that overlap one another (by the format's picture size)
    d_stream, po, pl, hdrs = dev.upload_packets(pkts[:4])
    fsz = F.plane_bytes(fmt, *a)
    d_out = dev.alloc(4 * fsz)
    for oo in ([0, fsz, fsz, 3 * fsz], [0, fsz - 16, 2 * fsz, 3 * fsz]):
        plan = dev.plan(hdrs, po, pl, np.array(oo, np.uint64))
        with pytest.raises(P.MiRtjError, match="overlap"):
            plan.set_runs_fmt([4])
        plan.set_runs_fmt([2, 2] if oo[1] == fsz else [1, 1, 2])  # runs that do not overlap themselves are taken
        plan.close()
    # pictures exactly back to back do not overlap
    plan = dev.plan(hdrs, po, pl, np.arange(4, dtype=np.uint64) * fsz)
    plan.set_runs_fmt([4])
    plan.close()
    dev.free(d_stream)
    dev.free(d_out)


@pytest.mark.parametrize("fmt", FMTS)
def test_profiling(devs, fmt):
    w, h = WRAP[fmt]
    pkts = F.make_packets(fmt, w, h, 200, 9, seed=3, key_rate=4)
    b = Batch(devs[fmt], fmt, pkts, [9], [RF.rand_pic(fmt, w, h, 3)])
    b.plan.set_runs_fmt([9])
    b.plan.profile(True)
    b.decode()
    ms, launches = b.plan.run_times()
    assert launches == 1 and ms > 0
    kt, n = b.plan.times()
    assert n == 1 and kt["k_index_emit"] > 0 and kt["k_decode"] > 0
    assert all(v == 0 for k, v in kt.items() if k not in ("k_index_emit", "k_decode"))
    steps = b.plan.step_times()
    assert len(steps) == 1 and steps[0] >= ms
    b.plan.profile(False)
    b.close()


@pytest.mark.parametrize("fmt", FMTS)
def test_one_larger_picture_size(devs, fmt):
    """640 x 368, 6 pictures, key_rate 255: 58 copy tiles of 4:2:2 (the last one partial), 3,680 greyscale blocks."""
    w, h, n = 640, 368, 6
    pkts = F.make_packets(fmt, w, h, 200, n, seed=3, key_rate=255, lmask=2, cmask=2)
    assert RF.has_both_kinds(fmt, pkts, [n])
    against_restatement(devs[fmt], fmt, pkts, [n], [RF.rand_pic(fmt, w, h, 6)], (w, h))


@pytest.mark.parametrize("fmt", FMTS)
def test_more_copy_items_than_a_grid_has_rows(devs, fmt):
    """8,200 runs of two pictures are 8,200 chunks and 65,600 copy items, past the 65,535 rows a grid may have: the
    kernels' loops over chunks, runs and items go round a second time.  16 distinct runs of 16 x 8 pictures, repeated,
    so that the restatement decodes 32 packets."""
    dev = devs[fmt]
    w, h, distinct, nruns = 16, 8, 16, 8200
    fsz = F.plane_bytes(fmt, w, h)
    runs_pk = [RF.crafted_run(fmt, 2, w, h, seed=r) for r in range(distinct)]
    prevs = [RF.rand_pic(fmt, w, h, r) for r in range(distinct)]
    want, copied = [], []
    for r in range(distinct):
        assert RF.has_both_kinds(fmt, runs_pk[r], [2])
        pics, c = RF.by_rule(fmt, runs_pk[r], [2], [prevs[r]])
        check(pics, RF.in_order(fmt, runs_pk[r], [2], [prevs[r]]), r)
        want.append(np.concatenate(pics))
        copied.append(c)
    pkts = [p for i in range(nruns) for p in runs_pk[i % distinct]]
    d_st, po, pl, hdrs = dev.upload_packets(pkts, align=1)
    host = np.full(2 * nruns * fsz, FILL, np.uint8)
    for i in range(nruns):
        host[2 * i * fsz:(2 * i + 1) * fsz] = prevs[i % distinct]
    d_out = dev.alloc(host.size)
    dev.h2d(d_out, host)
    plan = dev.plan(hdrs, po, pl, np.arange(2 * nruns, dtype=np.uint64) * fsz)
    plan.set_runs_fmt([2] * nruns)
    plan.decode(d_st, d_out)
    dev.sync()
    got = dev.d2h(d_out, host.size).reshape(nruns, 2 * fsz)
    for i in range(nruns):
        assert first_diff(got[i], want[i % distinct]) is None, (i, first_diff(got[i], want[i % distinct]))
    assert plan.run_copied() == sum(copied[i % distinct] for i in range(nruns)) > 0
    plan.close()
    dev.free(d_st)
    dev.free(d_out)
