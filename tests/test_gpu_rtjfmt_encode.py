"""The 4:2:2 and greyscale encoders on the device (mi_rtj_encode_frames_fmt / mi_rtj_encode_stream_fmt): packet bytes,
lengths and offsets byte for byte against the restatement of tests/rtjfmt_enc.py (which tests/test_rtjfmt_encode_cpu.py
holds to the reference's own encoder and to golden packets made by it), the golden 4:2:2 packets straight from the
device, and the device's packets back through the format decoders — the first real pictures those see.  No tolerance
anywhere.  Run on the GPU box with `pytest -m gpu`."""
import numpy as np
import pytest

import rtjfmt as F
import rtjfmt_enc as E
import rtjlib as R
from pkg import P

pytestmark = pytest.mark.gpu

B = P.binding
ERR_ARG = -3
PREFILL = 0x4D
INTRA_SHAPES = [
    (F.FMT_422, 16, 8),     # one macroblock: 62 idle lanes in the luma part, 30 + 30 in the chroma part
    (F.FMT_422, 48, 24),    # small picture of several rows
    (F.FMT_422, 176, 40),   # 11 macroblocks per row: groups wrap picture rows, the last group is partial
    (F.FMT_422, 528, 8),    # 33 per row: a group boundary inside a row
    (F.FMT_GREY, 8, 8),     # one block
    (F.FMT_GREY, 24, 8),    # one short block row
    (F.FMT_GREY, 136, 72),  # 17 blocks per row, 153 blocks: three groups, the last partial, rows wrap
    (F.FMT_GREY, 520, 8),   # 65 blocks: one full group plus one block
]
INTER_SHAPES = [(F.FMT_422, 48, 24), (F.FMT_422, 176, 40), (F.FMT_GREY, 24, 8), (F.FMT_GREY, 136, 72)]


def first_diff(a, b):
    if a.size != b.size:
        return ("size", a.size, b.size)
    d = np.nonzero(a != b)[0]
    return None if d.size == 0 else (int(d[0]), int(a[d[0]]), int(b[d[0]]), int(d.size))


def up(x, align):
    return (x + align - 1) // align * align


def upload(dev, pics):
    host = np.concatenate(pics)
    d = dev.alloc(host.size)
    dev.h2d(d, host)
    return d


def device_packets(dev, fmt, w, h, Q, pics, align=1, key=0, lmask=0, cmask=0, keep=False):
    """pictures -> (packets, pkt_offset, pkt_len[, device stream buffer]) through the binding"""
    n = len(pics)
    d_fr = upload(dev, pics)
    bound = dev.encode_bound(w, h, n, align, fmt=fmt)
    assert bound == n * up(12 + 64 * F.nblocks(fmt, w, h), align) + align
    d_st = dev.alloc(bound)
    dev.memset(d_st, PREFILL, bound)
    got_st, po, pl = dev.encode(w, h, Q, n, d_fr, align=align, key_rate=key, lmask=lmask, cmask=cmask, d_stream=d_st, fmt=fmt)
    assert got_st == d_st
    stream = dev.d2h(d_st, bound)
    dev.free(d_fr)
    pkts = [stream[int(po[i]):int(po[i]) + int(pl[i])].copy() for i in range(n)]
    if keep:
        return pkts, po, pl, d_st, stream
    dev.free(d_st)
    return pkts, po, pl, None, stream


def assert_stream_equals(what, want, pkts, po, pl, align, stream=None):
    """packet bytes, pkt_len and pkt_offset; with `stream`, also that the bytes between packets were left alone"""
    cur = 0
    assert len(want) == len(pkts) == po.size == pl.size
    for i, p in enumerate(want):
        start = up(cur, align)
        assert int(po[i]) == start and int(pl[i]) == p.size, (what, i, int(po[i]), start, int(pl[i]), p.size)
        assert first_diff(pkts[i], p) is None, (what, i, first_diff(pkts[i], p))
        if stream is not None:
            assert np.all(stream[cur:start] == PREFILL), (what, i)
        cur = start + p.size
    if stream is not None:
        assert np.all(stream[cur:] == PREFILL), what


def intra_pictures(fmt, w, h, Q):
    return [F.make_picture(fmt, w, h, i, seed=Q + amp, amp=amp) for i, amp in enumerate((0, 8, 64))] + \
        [E.extreme_picture(fmt, w, h, kind, seed=Q) for kind in E.EXTREMES]


def plan_decode(dev, fmt, w, h, d_st, po, pl, hdrs):
    """the packets where the encoder left them, through a plan of the instance's format: one slot per packet"""
    n, fsz = po.size, F.plane_bytes(fmt, w, h)
    slot = up(fsz, 256)
    d_out = dev.alloc(slot * n)
    dev.memset(d_out, PREFILL, slot * n)
    plan = dev.plan(hdrs, po, pl, np.arange(n, dtype=np.uint64) * slot)
    assert plan.fmt == fmt
    plan.decode(d_st, d_out)
    dev.sync()
    out = dev.d2h(d_out, slot * n)
    plan.close()
    dev.free(d_out)
    return [out[i * slot:i * slot + fsz] for i in range(n)]


# ---- intra, every launch shape; the device's packets back through a plan of the format ----
@pytest.mark.parametrize("fmt,w,h", INTRA_SHAPES)
def test_intra_against_the_restatement_and_back_through_a_plan(fmt, w, h):
    dev = P.MiRtj()
    dev.set_format(fmt)  # (for the plan below: encoding does not look at it)
    for Q, align in ((1, 1), (128, 64), (255, 1)):  # 128: lb8 == cb8; 255: the most raw bytes; 1: the coarsest tables
        pics = intra_pictures(fmt, w, h, Q)
        want = E.encode_all(fmt, w, h, Q, pics)
        pkts, po, pl, d_st, stream = device_packets(dev, fmt, w, h, Q, pics, align=align, keep=True)
        assert_stream_equals((fmt, w, h, Q), want, pkts, po, pl, align, stream)
        assert all(p[11] == 0 and p[10] == Q for p in pkts)
        hdrs = np.stack([p[:12] for p in pkts])
        got = plan_decode(dev, fmt, w, h, d_st, po, pl, hdrs)
        dec = F.Restated(fmt)
        for i, p in enumerate(pkts):
            back = np.full(F.plane_bytes(fmt, w, h), PREFILL, np.uint8)
            assert dec.decode(p, back)[0] == p.size
            assert first_diff(got[i], back) is None, (fmt, w, h, Q, i, first_diff(got[i], back))
        dev.free(d_st)
    dev.close()


def test_the_golden_422_packets_come_from_the_device():
    dev = P.MiRtj()
    total = 0
    for ci, w, h, Q, key, pics, want in E.golden_422():
        pkts, po, pl, _, _ = device_packets(dev, F.FMT_422, w, h, Q, pics, align=1, key=key, lmask=2, cmask=2)
        assert_stream_equals(("golden", ci), want, pkts, po, pl, 1)
        total += len(pkts)
    assert total == 8
    dev.close()


# ---- inter: one stream in order ----
def inter_pictures(fmt, w, h, seed):
    """six pictures: a new top third each time (rtjfmt_enc.make_stream), picture 3 the same as picture 2"""
    pics = E.make_stream(fmt, w, h, 6, seed=seed, amp=8)
    pics[3] = pics[2].copy()
    return pics


@pytest.mark.parametrize("fmt,w,h", INTER_SHAPES)
def test_inter_streams_against_the_restatement_and_back_in_order(fmt, w, h):
    dev = P.MiRtj()
    nb = F.nblocks(fmt, w, h)
    for key, Q in ((1, 255), (3, 128), (255, 224)):
        for lmask, cmask in ((0, 0), (2, 2), (16, 16), (2, 5)):
            what = (fmt, w, h, key, lmask, cmask)
            pics = inter_pictures(fmt, w, h, seed=key + lmask)
            want = E.encode_all(fmt, w, h, Q, pics, key, lmask, cmask)
            pkts, po, pl, _, stream = device_packets(dev, fmt, w, h, Q, pics, align=64 if key == 3 else 1, key=key,
                                                     lmask=lmask, cmask=cmask)
            assert_stream_equals(what, want, pkts, po, pl, 64 if key == 3 else 1, stream)
            assert [int(p[11]) for p in pkts] == [i % (key + 1) for i in range(6)], what  # the key byte counts and wraps
            # the same picture twice in a row (packet 3 is no key frame at any of these rates): nothing but 0xFF
            assert pkts[3].size == 12 + nb and np.all(pkts[3][12:] == 0xFF), what
            kinds = [E.block_kinds(fmt, p) for p in pkts]
            for i in range(1, 6):
                if i == 3:
                    assert kinds[i][1] == 0, (what, kinds)  # the repeated picture: no coded block
                elif pkts[i][11] == 0:
                    # a key frame: the store was cleared, and a block of these pictures has coefficients outside any mask
                    assert kinds[i][0] == 0, (what, i, kinds)
                elif h > 8:  # a new top third over an unchanged rest: both kinds in one packet
                    assert kinds[i][0] > 0 and kinds[i][1] > 0, (what, i, kinds)
                else:  # an 8-line picture has no block below the new third: every block is coded
                    assert kinds[i][1] > 0, (what, i, kinds)
            # back through the one-packet path of an instance of the format, in order
            back_dev, dec = P.MiRtj(), F.Restated(fmt)
            back_dev.set_format(fmt)
            back = np.zeros(F.plane_bytes(fmt, w, h), np.uint8)
            for i, p in enumerate(pkts):
                assert dec.decode(p, back)[0] == p.size
                got = np.zeros_like(back)
                back_dev.decode(p, got)
                assert first_diff(got, back) is None, (what, i, first_diff(got, back))
            back_dev.close()
    dev.close()


# ---- launch plumbing ----
def test_257_pictures_cross_the_pass_boundary():
    """an intra call takes 256 pictures per pass: picture 256 is the second pass's only one"""
    fmt, w, h, Q, n = F.FMT_422, 16, 8, 200, 257
    pics = [F.make_picture(fmt, w, h, i, seed=3, amp=(0, 8, 64)[i % 3]) for i in range(n)]
    want = E.encode_all(fmt, w, h, Q, pics)
    dev = P.MiRtj()
    pkts, po, pl, _, stream = device_packets(dev, fmt, w, h, Q, pics, align=64)
    assert_stream_equals("257", want, pkts, po, pl, 64, stream)
    assert len({p.tobytes() for p in pkts[250:]}) > 1
    dev.close()


def test_420_through_the_new_calls_is_the_old_encoder():
    dev = P.MiRtj()
    w, h, n, Q, align = 48, 32, 5, 224, 16
    d_fr = dev.synth(w, h, 0, n, seed=7, amp=8)
    bound = dev.encode_bound(w, h, n, align)
    assert dev.L.mi_rtj_encode_bound_fmt(B.FMT_YUV420, w, h, n, align) == bound
    for key, lmask, cmask in ((0, 0, 0), (2, 2, 5)):
        d_old, po_old, pl_old = dev.encode(w, h, Q, n, d_fr, align=align, key_rate=key, lmask=lmask, cmask=cmask)
        old = dev.d2h(d_old, bound)
        d_new = dev.alloc(bound)
        po, pl = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        pop, plp = po.ctypes.data_as(B.u64p), pl.ctypes.data_as(B.u32p)
        if key:
            rc = dev.L.mi_rtj_encode_stream_fmt(dev.h, B.FMT_YUV420, w, h, Q, key, lmask, cmask, n, d_fr, d_new, align, pop, plp)
        else:
            rc = dev.L.mi_rtj_encode_frames_fmt(dev.h, B.FMT_YUV420, w, h, Q, n, d_fr, d_new, align, pop, plp)
        assert rc == 0
        new = dev.d2h(d_new, bound)
        assert np.array_equal(po, po_old) and np.array_equal(pl, pl_old)
        for i in range(n):
            a, b = int(po[i]), int(po[i]) + int(pl[i])
            assert np.array_equal(new[a:b], old[a:b]), (key, i)
        assert first_diff(new[12:int(pl[0])], R.OracleEncoder(w, h, Q, key, lmask, cmask).encode(
            R.synth_frame(w, h, 0, seed=7, amp=8))[12:]) is None
        dev.free(d_old)
        dev.free(d_new)
    dev.free(d_fr)
    dev.close()


def test_the_format_is_the_calls_not_the_instances():
    """an instance in one format encodes another; encoding neither reads nor fixes mi_rtj_set_format's state"""
    dev = P.MiRtj()
    pic = F.make_picture(F.FMT_GREY, 24, 8, 0, seed=2, amp=8)
    want = E.encode_all(F.FMT_GREY, 24, 8, 192, [pic])
    pkts, po, pl, _, _ = device_packets(dev, F.FMT_GREY, 24, 8, 192, [pic])
    assert_stream_equals("grey on a fresh instance", want, pkts, po, pl, 1)
    assert dev.format == B.FMT_YUV420
    dev.set_format(B.FMT_YUV422)  # still free to change: encoding fixed nothing
    pkts, po, pl, _, _ = device_packets(dev, F.FMT_GREY, 24, 8, 192, [pic])
    assert_stream_equals("grey on a 4:2:2 instance", want, pkts, po, pl, 1)
    assert dev.format == B.FMT_YUV422
    dev.close()


# ---- refusals ----
def test_refusals_leave_the_instance_encoding():
    dev = P.MiRtj()
    d_fr, d_st = dev.alloc(4096), dev.alloc(8192)
    dev.memset(d_fr, 100, 4096)
    po, pl = np.zeros(1, np.uint64), np.zeros(1, np.uint32)
    pop, plp = po.ctypes.data_as(B.u64p), pl.ctypes.data_as(B.u32p)

    def refused(rc, *words):
        msg = dev.L.mi_rtj_last_error(dev.h).decode()
        assert rc == ERR_ARG and all(x in msg for x in words), (rc, msg)

    frames, stream = dev.L.mi_rtj_encode_frames_fmt, dev.L.mi_rtj_encode_stream_fmt
    for w, h in ((24, 8), (16, 12), (0, 8), (16, 0)):
        refused(frames(dev.h, B.FMT_YUV422, w, h, 128, 1, d_fr, d_st, 1, pop, plp), "4:2:2", "multiple of 16", "multiple of 8")
        refused(stream(dev.h, B.FMT_YUV422, w, h, 128, 3, 2, 2, 1, d_fr, d_st, 1, pop, plp), "4:2:2", "multiple of 16")
    for w, h in ((12, 8), (8, 12), (0, 8)):
        refused(frames(dev.h, B.FMT_GREY, w, h, 128, 1, d_fr, d_st, 1, pop, plp), "greyscale", "multiples of 8")
    for fmt in (3, -1):
        refused(frames(dev.h, fmt, 16, 16, 128, 1, d_fr, d_st, 1, pop, plp), "format")
        refused(stream(dev.h, fmt, 16, 16, 128, 3, 2, 2, 1, d_fr, d_st, 1, pop, plp), "format")
    for fmt in (B.FMT_YUV422, B.FMT_GREY):
        refused(frames(dev.h, fmt, 16, 8, 128, 1, None, d_st, 1, pop, plp), "argument")
        refused(frames(dev.h, fmt, 16, 8, 128, 1, d_fr, None, 1, pop, plp), "argument")
        refused(frames(dev.h, fmt, 16, 8, 128, 1, d_fr, d_st, 1, None, plp), "argument")
        refused(frames(dev.h, fmt, 16, 8, 128, 1, d_fr, d_st, 1, pop, None), "argument")
        refused(frames(dev.h, fmt, 16, 8, 128, 0, d_fr, d_st, 1, pop, plp), "argument")
        refused(frames(dev.h, fmt, 16, 8, 128, 1, d_fr, d_st, 3, pop, plp), "argument")
    assert frames(None, B.FMT_YUV422, 16, 8, 128, 1, d_fr, d_st, 1, pop, plp) == ERR_ARG
    with pytest.raises(P.MiRtjError, match="rc=-3: .*4:2:2"):  # the binding raises with the library's message
        dev.encode(24, 8, 128, 1, d_fr, fmt=B.FMT_YUV422)
    # ... and the instance still encodes
    for fmt, w, h in ((F.FMT_422, 16, 8), (F.FMT_GREY, 8, 8)):
        pic = F.make_picture(fmt, w, h, 0, seed=5, amp=8)
        pkts, po2, pl2, _, _ = device_packets(dev, fmt, w, h, 128, [pic])
        assert_stream_equals("after refusals", E.encode_all(fmt, w, h, 128, [pic]), pkts, po2, pl2, 1)
    dev.free(d_fr)
    dev.free(d_st)
    dev.close()


def test_quality_and_intra_settings_are_clamped():
    """Q to 1 .. 255, key_rate to 0 .. 255, masks to 0 .. 16 (RTjpeg_set_intra's clamps)"""
    dev = P.MiRtj()
    fmt, w, h = F.FMT_422, 48, 24
    pics = inter_pictures(fmt, w, h, seed=9)[:4]
    for (Q, key, lm, cm), (cq, ckey, clm, ccm) in (((0, 0, 0, 0), (1, 0, 0, 0)), ((999, 300, 40, -3), (255, 255, 16, 0)),
                                                   ((200, -5, 3, 3), (200, 0, 0, 0))):
        want = E.encode_all(fmt, w, h, cq, pics, ckey, clm, ccm)
        d_fr = upload(dev, pics)
        bound = dev.encode_bound(w, h, 4, 1, fmt=fmt)
        d_st = dev.alloc(bound)
        po, pl = np.zeros(4, np.uint64), np.zeros(4, np.uint32)
        rc = dev.L.mi_rtj_encode_stream_fmt(dev.h, fmt, w, h, Q, key, lm, cm, 4, d_fr, d_st, 1, po.ctypes.data_as(B.u64p),
                                            pl.ctypes.data_as(B.u32p))
        assert rc == 0
        stream = dev.d2h(d_st, bound)
        pkts = [stream[int(po[i]):int(po[i]) + int(pl[i])] for i in range(4)]
        assert_stream_equals((Q, key, lm, cm), want, pkts, po, pl, 1)
        dev.free(d_fr)
        dev.free(d_st)
    dev.close()
