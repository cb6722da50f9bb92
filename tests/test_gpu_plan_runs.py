"""Plans with runs on the device (mi_rtj_plan_set_runs): one launch decodes streams with unchanged blocks, bit-exact
with the reference's in-order decode.  Run on the GPU box with `pytest -m gpu`."""
import numpy as np
import pytest

import rtjlib as R
import runlib as RL
from pkg import P

pytestmark = pytest.mark.gpu

FILL = 0x5A  # slots of pictures k > 0 start as this: every unchanged block there must be copied


@pytest.fixture(scope="module")
def dev():
    d = P.MiRtj()
    yield d
    d.close()


def first_diff(a, b):
    d = np.nonzero(a != b)[0]
    return None if d.size == 0 else (int(d[0]), int(a[d[0]]), int(b[d[0]]), int(d.size))


class Batch:
    """Packets uploaded once, one output slot each; picture 0 of every run prefilled with prev[r]."""

    def __init__(self, dev, pkts, runs, prev, align=1, pad=256):
        self.dev, self.pkts, self.runs, self.prev = dev, pkts, runs, prev
        self.d_stream, po, pl, hdrs = dev.upload_packets(pkts, align=align)
        self.sizes = [RL.frame_bytes(*RL.dims(p)) for p in pkts]
        self.oo = np.zeros(len(pkts), np.uint64)
        cur = 0
        for i, s in enumerate(self.sizes):
            self.oo[i] = cur
            cur += (s + pad - 1) // pad * pad
        self.total = cur
        self.d_out = dev.alloc(cur)
        self.plan = dev.plan(hdrs, po, pl, self.oo)

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
        return [self.dev.d2h(self.d_out, self.sizes[i], offset=int(self.oo[i])) for i in range(len(self.pkts))]

    def close(self):
        self.plan.close()
        self.dev.free(self.d_stream)
        self.dev.free(self.d_out)


def check(got, want, what=""):
    for i, (a, b) in enumerate(zip(got, want)):
        assert first_diff(a, b) is None, (what, i, first_diff(a, b))


def decode_runs(dev, pkts, runs, prev, **kw):
    b = Batch(dev, pkts, runs, prev, **kw)
    b.plan.set_runs(runs)
    got = b.decode()
    copied = b.plan.run_copied()
    b.close()
    return got, copied


def rand_pic(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, RL.frame_bytes(w, h), dtype=np.uint8)


def test_golden_inter_sequence_as_one_run(dev):
    G = np.load(R.GOLDEN + "/rtjpeg_golden.npz")
    w, h, Q, key, lm, cm, nfr = [int(x) for x in G["inter_meta"]]
    pkts = [G[f"inter_{n}_pkt"] for n in range(nfr)]
    got, copied = decode_runs(dev, pkts, [nfr], [np.zeros(RL.frame_bytes(w, h), np.uint8)])
    for n in range(nfr):
        assert first_diff(got[n], G[f"inter_{n}_planes"]) is None, n
    assert copied > 0


@pytest.mark.parametrize("w,h,Q,key_rate,lm,cm", [(320, 240, 200, 4, 2, 2), (640, 368, 255, 255, 16, 16),
                                                  (320, 240, 90, 1, 0, 0), (1920, 1088, 150, 8, 4, 4)])
def test_encoder_streams(dev, w, h, Q, key_rate, lm, cm):
    n = 12 if w < 1920 else 6
    frames = [R.synth_frame(w, h, i // 3, seed=13 + w, amp=3) for i in range(n)]
    d_fr = dev.alloc(RL.frame_bytes(w, h) * n)
    dev.h2d(d_fr, np.concatenate(frames))
    d_st, po, pl = dev.encode(w, h, Q, n, d_fr, align=1, key_rate=key_rate, lmask=lm, cmask=cm)
    dev.sync()
    pkts = [dev.d2h(d_st, int(pl[i]), offset=int(po[i])) for i in range(n)]
    dev.free(d_fr)
    dev.free(d_st)
    assert sum(int((p[12:] == 255).sum()) for p in pkts) > 0
    prev = [rand_pic(w, h, 1)]
    got, copied = decode_runs(dev, pkts, [n], prev)
    check(got, RL.oracle_in_order(pkts, [n], prev), (w, h))
    assert copied > 0


def test_several_runs_sizes_and_qualities(dev):
    pkts, runs, prev = [], [], []
    for j, (w, h, Q, n, kr) in enumerate([(320, 240, 200, 5, 4), (64, 48, 90, 1, 1), (160, 128, 255, 7, 255),
                                          (48, 32, 30, 1, 3), (320, 240, 120, 3, 2), (64, 48, 90, 4, 1)]):
        pkts += RL.stream_packets(w, h, Q, n, kr, 3, 3, seed=j)
        runs.append(n)
        prev.append(rand_pic(w, h, j))
    got, _ = decode_runs(dev, pkts, runs, prev)
    check(got, RL.oracle_in_order(pkts, runs, prev))


def test_quality_change_inside_a_run(dev):
    w, h = 160, 128
    pkts = RL.stream_packets(w, h, 200, 4, 4, 2, 2, seed=3) + RL.stream_packets(w, h, 60, 4, 4, 2, 2, seed=3) + \
        RL.stream_packets(w, h, 255, 3, 2, 8, 8, seed=4)
    prev = [rand_pic(w, h, 5)]
    got, _ = decode_runs(dev, pkts, [len(pkts)], prev)
    check(got, RL.oracle_in_order(pkts, [len(pkts)], prev))


def _crafted_run(n, w=48, h=32, Q=100, seed=0):
    """Packets of 0xFF and coded blocks by a pattern: block 0 coded only in picture 0, block 1 only in the last,
    block 2 never, block 3 every 64th picture, the rest at random."""
    rng = np.random.default_rng(seed)
    _, _, lb8, cb8, _, _ = R.oracle_tables(Q)
    nblk = (w // 16) * (h // 16) * 6
    pkts = []
    for k in range(n):
        body = bytearray()
        for b in range(nblk):
            coded = {0: k == 0, 1: k == n - 1, 2: False, 3: k % 64 == 0}.get(b, rng.random() < 0.3)
            if not coded:
                body.append(255)
                continue
            bt8 = lb8 if (b % 6) < 4 else cb8
            body += bytes([int(rng.integers(0, 255))] + [int(x) for x in rng.integers(0, 4, bt8)] + ([126 - bt8] if bt8 < 63 else []))
        pkts.append(np.concatenate([RL.header(w, h, Q, 12 + len(body)), np.frombuffer(bytes(body), np.uint8)]))
    return pkts


@pytest.mark.parametrize("n", [63, 64, 65, 3 * 64 + 5])
def test_runs_around_the_scan_chunk(dev, n):
    pkts = _crafted_run(n, seed=n)
    prev = [rand_pic(48, 32, n)]
    got, _ = decode_runs(dev, pkts, [n], prev)
    check(got, RL.oracle_in_order(pkts, [n], prev), n)
    check(got, RL.oracle_by_rule(pkts, [n], prev), n)


def test_adversarial_and_fuzz_packets_in_runs(dev):
    from golden.make_golden import adversarial_packet
    rng = np.random.default_rng(99)
    pkts, runs, prev = [], [], []
    for j, Q in enumerate((1, 3, 31, 129, 255)):
        _, _, lb8, cb8, _, _ = R.oracle_tables(Q)
        w, h = [(48, 32), (160, 16), (160, 64)][j % 3]
        run = [adversarial_packet(rng, w, h, Q, lb8, cb8, skip_prob=float(rng.choice([0.1, 0.5, 0.9])))
               for _ in range(4)]
        run += [RL.skip_heavy_packet(rng, w, h, Q) for _ in range(4)]
        run.append(RL.skip_heavy_packet(rng, w, h, Q, n=0))
        pkts += [run[i] for i in rng.permutation(len(run))]
        runs.append(len(run))
        prev.append(rand_pic(w, h, j))
    got, _ = decode_runs(dev, pkts, runs, prev)
    check(got, RL.oracle_in_order(pkts, runs, prev))


def test_repeat_and_reset(dev):
    w, h = 320, 240
    pkts = RL.stream_packets(w, h, 200, 10, 4, 2, 2, seed=8)
    prev = [rand_pic(w, h, 8)]
    b = Batch(dev, pkts, [10], prev)
    b.plan.set_runs([10])
    first = b.decode()
    n1 = b.plan.run_copied()
    again = b.decode()
    check(again, first, "repeat")
    assert b.plan.run_copied() == n1 > 0
    check(first, RL.oracle_in_order(pkts, [10], prev))
    b.plan.set_runs([])
    plain = b.decode()
    assert b.plan.run_copied() == 0
    # today's rule: an unchanged block leaves its slot as it was (picture 0: prev, the others: FILL)
    dec = R.OracleDecoder()
    for i, p in enumerate(pkts):
        want = prev[0].copy() if i == 0 else np.full(RL.frame_bytes(w, h), FILL, np.uint8)
        dec.decode(p, want)
        assert first_diff(plain[i], want) is None, i
    b.close()


def test_refusals_leave_the_plan_decoding(dev):
    pkts = RL.stream_packets(64, 48, 90, 4, 1, 0, 0, seed=2) + RL.stream_packets(48, 32, 90, 3, 1, 0, 0, seed=2)
    prev = [rand_pic(64, 48, 1), rand_pic(48, 32, 2)]
    b = Batch(dev, pkts, [4, 3], prev)
    b.plan.set_runs([4, 3])
    for bad in ([4, 2], [4, 4], [4, 0, 3], [4, -1, 4], [3, 4], [7]):  # sums, lengths, size change inside a run
        with pytest.raises(P.binding.MiRtjError):
            b.plan.set_runs(bad)
    check(b.decode(), RL.oracle_in_order(pkts, [4, 3], prev), "after refusals")
    b.close()
    # output pictures of a run that overlap one another
    d_stream, po, pl, hdrs = dev.upload_packets(pkts[:4])
    fsz = RL.frame_bytes(64, 48)
    d_out = dev.alloc(4 * fsz)
    for oo in ([0, fsz, fsz, 3 * fsz], [0, 16, 2 * fsz, 3 * fsz]):
        plan = dev.plan(hdrs, po, pl, np.array(oo, np.uint64))
        with pytest.raises(P.binding.MiRtjError):
            plan.set_runs([4])
        plan.set_runs([2, 2] if oo[1] == fsz else [1, 1, 2])  # runs that do not overlap themselves are taken
        plan.close()
    dev.free(d_stream)
    dev.free(d_out)


@pytest.mark.parametrize("overlap,split", [("0", "1"), ("1", "0")])
def test_large_1080p_against_a_session(dev, monkeypatch, overlap, split):
    """1,024 pictures of 1080p in runs, with the speculative index, the split or the classic transform form and an
    overlapped index or not.  Each run is one encoder stream (its picture 0 is a key picture), so a session decodes
    the same pictures from scratch: every picture must equal the session's, a sample the oracle's."""
    monkeypatch.setenv("MI_RTJ_OVERLAP", overlap)
    monkeypatch.setenv("MI_RTJ_SPLIT", split)
    w, h, n = 1920, 1088, 1024
    runs = [300, 1, 64, 659]
    fsz = RL.frame_bytes(w, h)
    d_fr = dev.alloc(fsz * n)
    dev.synth(w, h, 0, n, seed=21, amp=2, dptr=d_fr)
    d_st = dev.alloc(dev.encode_bound(w, h, n, 64))
    po, pl = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    i, base = 0, 0
    for r, m in enumerate(runs):
        _, a, l = dev.encode(w, h, 200, m, d_fr + i * fsz, align=64, key_rate=255 if r % 2 == 0 else 16, lmask=4,
                             cmask=4, d_stream=d_st + base)
        dev.sync()
        po[i:i + m] = a + base
        pl[i:i + m] = l
        base = int(po[i + m - 1] + pl[i + m - 1] + 63) // 64 * 64
        i += m
    dev.free(d_fr)
    hdrs = np.stack([dev.d2h(d_st, 12, offset=int(po[j])) for j in range(n)])
    oo = np.arange(n, dtype=np.uint64) * fsz
    d_out = dev.alloc(n * fsz)
    dev.memset(d_out, FILL, n * fsz)
    plan = dev.plan(hdrs, po, pl, oo)
    plan.set_runs(runs)
    plan.decode(d_st, d_out)
    dev.sync()
    copied = plan.run_copied()
    pkts = [dev.d2h(d_st, int(pl[j]), offset=int(po[j])) for j in range(n)]
    skipped = sum(int((RL.coded_blocks(R.OracleDecoder().block_offsets(p)) == 0).sum()) for p in pkts[1:8])
    assert skipped > 0 and copied > 0
    starts = np.cumsum([0] + runs[:-1])
    sample = set(np.random.default_rng(0).choice(n, 6, replace=False).tolist()) | {int(s) for s in starts} | {63, 64, n - 1}
    j = 0
    for r, m in enumerate(runs):
        s = P.MiRtj()
        pipe = s.pipe(depth=8, coded_w=w, coded_h=h)
        dec, frame = R.OracleDecoder(), np.zeros(fsz, np.uint8)
        k_out = 0
        for k in range(m):
            pipe.submit(pkts[j + k], tag=j + k)
            while pipe.room() == 0 or (k == m - 1 and pipe.pending()):
                y, u, v, tag = pipe.next()
                want = np.concatenate([y, u, v])
                got = dev.d2h(d_out, fsz, offset=int(oo[tag]))
                assert first_diff(got, want) is None, ("session", r, tag - j)
                k_out += 1
        assert k_out == m
        for k in range(m):
            dec.decode(pkts[j + k], frame)
            if j + k in sample:
                assert first_diff(dev.d2h(d_out, fsz, offset=int(oo[j + k])), frame) is None, ("oracle", r, k)
        pipe.close()
        s.close()
        j += m
    plan.close()
    dev.free(d_st)
    dev.free(d_out)
