"""The host layer's buffers when they have to grow (csrc/host_base.h, GrowBuf::grow): an instance, a plan and a session
are fed pictures that outgrow what they hold, then smaller ones that reuse it, then larger ones again — every picture
bit for bit against the oracle (4:2:2 and greyscale: the restatement of tests/rtjfmt.py), on the smallest pictures that
force a reallocation.  Every object is closed explicitly: a double free or a freed view would end the process there.

What no other test was found to reach: the one-packet picture, packet buffer and index growing, being reused and growing
again on ONE instance (all three formats), the one-packet plan's speculative buffers growing with the packet, and a
session without a fixed size whose slots grow.  Reached elsewhere too and repeated here on one object family, as cheap as it is: the
chunk scratch, the speculative buffers and split lists of a batch plan (tests/test_gpu_spec_index.py,
tests/test_gpu_decode_policy.py), runs replaced on a live plan (tests/test_gpu_plan_runs.py), a group plan's index after a
flush inside a group (tests/test_gpu_sessions.py).  Run on the GPU box with `pytest -m gpu`."""
import numpy as np
import pytest

import rtjfmt as F
import rtjlib as R
import runlib as RL
from pkg import P

pytestmark = pytest.mark.gpu


def first_diff(a, b):
    d = np.nonzero(a != b)[0]
    return None if d.size == 0 else (int(d[0]), int(a[d[0]]), int(b[d[0]]), int(d.size))


def intra_packet(w, h, i, Q=200, amp=8):
    """a packet that codes every block: its picture does not depend on what the buffer held"""
    return R.OracleEncoder(w, h, Q).encode(R.synth_frame(w, h, i, seed=31 + w, amp=amp))


def oracle_picture(pkt):
    w, h = RL.dims(pkt)
    pic = np.zeros(RL.frame_bytes(w, h), np.uint8)
    R.OracleDecoder().decode(pkt, pic)
    return pic


# ---- one instance, single packets: grows, reuses, grows again ----
@pytest.mark.parametrize("spec", [None, "1"])  # "1": the one-packet plan speculates, its walkers' buffers grow with the packet
def test_one_instance_decodes_packets_that_grow_shrink_and_grow(monkeypatch, spec):
    if spec:
        monkeypatch.setenv("MI_RTJ_SPEC", spec)
    else:
        monkeypatch.delenv("MI_RTJ_SPEC", raising=False)
    dev = P.MiRtj()
    for i, (w, h) in enumerate([(16, 16), (64, 48), (16, 16), (128, 64)]):
        # (amp 64: the 128x64 packet is also the longest by far — the packet buffer and the chunk scratch grow with it)
        pkt = intra_packet(w, h, i, Q=255, amp=64 if w == 128 else 8)
        want = oracle_picture(pkt)
        got = np.zeros(want.size, np.uint8)
        dev.decode(pkt, got)
        assert first_diff(got, want) is None, (w, h, "decode", first_diff(got, want))
        y, u, v = dev.decode_nocopy(pkt)  # the pinned host picture grows the same way
        assert first_diff(np.concatenate([y, u, v]), want) is None, (w, h, "nocopy")
    dev.close()


@pytest.mark.parametrize("fmt,sizes", [(F.FMT_422, [(16, 8), (48, 16)]), (F.FMT_GREY, [(8, 8), (24, 16)])])
def test_one_instance_of_the_other_formats_grows(fmt, sizes):
    dev = P.MiRtj()
    dev.set_format(fmt)
    for w, h in sizes:
        pkt = F.make_packets(fmt, w, h, 200, 1, seed=w, amp=8)[0]
        want = np.zeros(F.plane_bytes(fmt, w, h), np.uint8)
        assert F.Restated(fmt).decode(pkt, want) is not None
        got = np.zeros(want.size, np.uint8)
        dev.decode(pkt, got)
        assert first_diff(got, want) is None, (fmt, w, h, first_diff(got, want))
    dev.close()


# ---- one plan family: speculative buffers and split lists made and used, runs replaced on a live plan ----
class Batch:
    def __init__(self, dev, pkts):
        self.dev, self.n = dev, len(pkts)
        self.fsz = RL.frame_bytes(*RL.dims(pkts[0]))
        self.d_stream, po, pl, hdrs = dev.upload_packets(pkts)
        self.d_out = dev.alloc(self.fsz * self.n)
        self.plan = dev.plan(hdrs, po, pl, np.arange(self.n, dtype=np.uint64) * self.fsz)

    def decode(self):
        self.dev.memset(self.d_out, 0, self.fsz * self.n)
        self.plan.decode(self.d_stream, self.d_out)
        self.dev.sync()
        return [self.dev.d2h(self.d_out, self.fsz, offset=i * self.fsz) for i in range(self.n)]

    def close(self):
        self.plan.close()
        self.dev.free(self.d_stream)
        self.dev.free(self.d_out)


def test_two_plans_of_one_instance_and_runs_replaced_on_a_live_plan(monkeypatch):
    monkeypatch.setenv("MI_RTJ_SPEC", "1")
    monkeypatch.setenv("MI_RTJ_ROTATE", "1")
    monkeypatch.setenv("MI_RTJ_SPLIT", "1")
    w = h = 32
    pkts = RL.stream_packets(w, h, 200, 9, 255, 2, 2)  # one key frame, then unchanged blocks
    assert sum(int((p[12:] == 255).sum()) for p in pkts[1:]) > 0
    zero = np.zeros(RL.frame_bytes(w, h), np.uint8)

    def check(b, runs, what):
        want = RL.oracle_in_order(pkts[:b.n], runs, [zero] * len(runs))
        for launch in range(2):
            got = b.decode()
            for i in range(b.n):
                assert first_diff(got[i], want[i]) is None, (what, launch, i, first_diff(got[i], want[i]))

    dev = P.MiRtj()
    small, big = Batch(dev, pkts[:2]), Batch(dev, pkts)
    check(small, [1, 1], "2 packets")
    check(big, [1] * 9, "9 packets")
    assert big.plan.spec_stats()[1] > 0 and big.plan.decode_form()[0] == 0  # speculative index, split form: made and used
    for runs in ([9], [3, 3, 3], []):
        big.plan.set_runs(runs)
        check(big, runs or [1] * 9, f"runs {runs}")
        assert (big.plan.run_copied() > 0) == bool(runs), runs
    check(small, [1, 1], "2 packets again")
    big.close()
    small.close()
    dev.close()


# ---- sessions ----
def take(pipe):
    y, u, v, tag = pipe.next()
    return np.concatenate([y, u, v]), tag


def test_session_without_a_fixed_size_grows_its_slots():
    dev = P.MiRtj()
    pipe = dev.pipe(depth=4)
    pkts = [intra_packet(w, h, i) for i, (w, h) in enumerate([(16, 16)] * 5 + [(48, 32)] * 5 + [(16, 16)] * 5)]
    got = 0
    for i, pkt in enumerate(pkts):
        pipe.submit(pkt, i)
        if pipe.pending() == 3 or i == len(pkts) - 1:
            while pipe.pending() > (0 if i == len(pkts) - 1 else 1):
                pic, tag = take(pipe)
                assert tag == got and first_diff(pic, oracle_picture(pkts[got])) is None, (got, RL.dims(pkts[got]))
                got += 1
    assert got == len(pkts)
    pipe.close()
    dev.close()


def test_session_flushed_inside_an_index_group_and_refilled(monkeypatch):
    monkeypatch.setenv("MI_RTJ_IDX_GROUP", "4")
    monkeypatch.setenv("MI_RTJ_OUT_GROUP", "4")
    w = h = 32
    pkts = RL.stream_packets(w, h, 200, 14, 255, 2, 2)
    want = RL.oracle_in_order(pkts, [len(pkts)], [np.zeros(RL.frame_bytes(w, h), np.uint8)])
    dev = P.MiRtj()
    pipe = dev.pipe(depth=8, coded_w=w, coded_h=h)
    pipe.submit(pkts[0], 0)
    pipe.submit(pkts[1], 1)
    pipe.flush()  # two packets of a group of four: decoded and forgotten; the ring now stands inside the group
    assert pipe.pending() == 0
    got = 2
    for i in range(2, len(pkts)):
        pipe.submit(pkts[i], i)
        if pipe.room() == 0 or i == len(pkts) - 1:
            while pipe.pending() > 0:
                pic, tag = take(pipe)
                assert tag == got and first_diff(pic, want[got]) is None, (got, first_diff(pic, want[got]))
                got += 1
    assert got == len(pkts)
    pipe.close()
    dev.close()


# ---- mi_rtj_copy_ceiling: its two events are the call's own (csrc/host_base.h, EventPair); a refused call writes nothing ----
def test_copy_ceiling_copies_and_refuses_without_writing():
    dev = P.MiRtj()
    n = 4096
    src = (np.arange(n, dtype=np.uint32) * 2654435761 >> 13).astype(np.uint8)
    d_src, d_dst = dev.alloc(n + 16), dev.alloc(n + 16)
    dev.h2d(d_src, src)
    dev.memset(d_dst, 0xA5, n + 16)
    assert dev.copy_ceiling(d_src, d_dst, n, reps=2) > 0
    assert first_diff(dev.d2h(d_dst, n), src) is None
    assert (dev.d2h(d_dst, 16, offset=n) == 0xA5).all()  # nothing behind the bytes asked for
    dev.memset(d_dst, 0x5A, n + 16)
    for bad in (dict(nbytes=24), dict(nbytes=n, d_src=d_src + 4), dict(nbytes=n, d_dst=d_dst + 8), dict(nbytes=n, reps=0)):
        args = dict(dict(d_src=d_src, d_dst=d_dst, reps=2), **bad)
        with pytest.raises(P.MiRtjError, match=r"rc=-3: mi_rtj_copy_ceiling: bad argument"):
            dev.copy_ceiling(args["d_src"], args["d_dst"], args["nbytes"], reps=args["reps"])
        assert (dev.d2h(d_dst, n + 16) == 0x5A).all(), bad
    dev.free(d_src)
    dev.free(d_dst)
    dev.close()
