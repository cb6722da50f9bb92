"""4:2:2 and greyscale RTjpeg streams on the device (mi_rtj_set_format): the one-packet path, plans, hostile input,
refusals and the 4:2:2 colour stage — bit for bit against the restatement of tests/rtjfmt.py (which tests/test_rtjfmt_cpu.py
holds to the reference's own code) and against golden vectors made by the reference.  No tolerance anywhere.
Run on the GPU box with `pytest -m gpu`."""
import numpy as np
import pytest

import edge_packets as E
import rtjfmt as F
import rtjlib as R
from pkg import P

pytestmark = pytest.mark.gpu

B = P.binding
ERR_ARG, ERR_GEOMETRY = -3, -4
SMALL = [(F.FMT_422, 48, 24), (F.FMT_422, 176, 40), (F.FMT_GREY, 24, 8), (F.FMT_GREY, 136, 72)]
SHAPES = SMALL + [(F.FMT_422, 640, 360), (F.FMT_GREY, 640, 360)]
QUALITIES = (1, 128, 192, 224, 255)  # lb8 = 0, 0, 4, 8, 9 (tab_b8 of the golden tables); cb8 is always 0
PREFILL = 0x4D


def first_diff(a, b):
    d = np.nonzero(a != b)[0]
    return None if d.size == 0 else (int(d[0]), int(a[d[0]]), int(b[d[0]]), int(d.size))


def instance(fmt):
    d = P.MiRtj()
    d.set_format(fmt)
    assert d.format == fmt
    return d


def rc_of(dev, call):
    """return code and message of a call that must be refused"""
    with pytest.raises(P.MiRtjError) as e:
        call()
    msg = str(e.value)
    assert msg.startswith("rc=") and len(msg.split(": ", 1)[1]) > 10, msg
    return int(msg[3:msg.index(":")]), msg


def decode_stream(fmt, pkts, via="decode"):
    """Packets in order through one instance and one restatement; the persistent picture of a fresh instance is zero."""
    dev, want_dec = instance(fmt), F.Restated(fmt)
    want = None
    for i, pkt in enumerate(pkts):
        w, h, _ = F.header_of(pkt)
        n = F.plane_bytes(fmt, w, h)
        if want is None or want.size != n:
            assert i == 0 or n > want.size  # (a smaller picture would reuse the larger one's bytes: not exercised)
            want = np.zeros(n, np.uint8)
        assert want_dec.decode(pkt, want) is not None
        if via == "decode":
            got = np.zeros(n, np.uint8)
            dev.decode(pkt, got)
        else:
            y, u, v = dev.decode_nocopy(pkt)
            got = y.copy() if fmt == F.FMT_GREY else np.concatenate([y, u, v])
            assert (u is None) == (fmt == F.FMT_GREY)
        assert first_diff(got, want) is None, (fmt, w, h, i, first_diff(got, want))
        assert dev.state() == (w, h, want_dec.Q)
    dev.close()


# ---- the default stays what it was ----
def test_fresh_instance_is_420_and_decodes_as_before():
    G = np.load(R.GOLDEN + "/rtjpeg_golden.npz")
    dev = P.MiRtj()
    assert dev.format == B.FMT_YUV420
    dev.set_format(B.FMT_YUV420)
    assert dev.format == B.FMT_YUV420
    pkt, want = G["intra0_0_pkt"], G["intra0_0_planes"]
    got = np.zeros(want.size, np.uint8)
    dev.decode(pkt, got)
    assert first_diff(got, want) is None
    dev.set_format(B.FMT_YUV420)  # the format it has: still accepted
    dev.close()


# ---- one-packet path ----
@pytest.mark.parametrize("fmt,w,h", SHAPES)
def test_intra_packets_of_every_quality_and_noise(fmt, w, h):
    big = w * h > 100000
    pkts = []
    for Q in QUALITIES:
        for amp in ((64,) if big and Q != 255 else (0, 8, 64)):
            pkts += F.make_packets(fmt, w, h, Q, 1, seed=Q + amp, amp=amp)
    decode_stream(fmt, pkts)


@pytest.mark.parametrize("fmt,w,h", SMALL)
def test_golden_streams_made_by_the_reference(fmt, w, h):
    cases = [c for c in F.golden_cases(F.load_golden()) if (c[0], c[1], c[2]) == (fmt, w, h)]
    assert cases
    for _, _, _, Q, key, pkts, outs in cases:
        # the golden decoder's planes started as 77; the device's persistent picture starts as 0: compare through a plan
        # whose slot is prefilled, one packet per launch into the same slot, as a stream is decoded
        dev = instance(fmt)
        n = F.plane_bytes(fmt, w, h)
        d_out = dev.alloc(n)
        dev.memset(d_out, 77, n)
        for i, (pkt, want) in enumerate(zip(pkts, outs)):
            d_st, po, pl, hdrs = dev.upload_packets([pkt])
            plan = dev.plan(hdrs, po, pl, np.zeros(1, np.uint64))
            plan.decode(d_st, d_out)
            dev.sync()
            got = dev.d2h(d_out, n)
            assert first_diff(got, want) is None, (Q, key, i, first_diff(got, want))
            plan.close()
            dev.free(d_st)
        dev.free(d_out)
        dev.close()


@pytest.mark.parametrize("fmt,w,h", SHAPES)
def test_stream_with_unchanged_blocks_in_order(fmt, w, h):
    pkts = F.make_packets(fmt, w, h, 224, 4, seed=3, amp=8, key_rate=3)
    assert any(np.count_nonzero(p[F.HEADER:] == 0xFF) for p in pkts[1:])
    decode_stream(fmt, pkts)
    decode_stream(fmt, pkts, via="nocopy")


@pytest.mark.parametrize("fmt", (F.FMT_422, F.FMT_GREY))
def test_first_packet_with_quality_byte_zero(fmt):
    """a fresh decoder's tables are all zero and stay so when the first header says quality 0 (lb8 = cb8 = 0)"""
    pkts = F.make_packets(fmt, 176, 40, 192, 2, seed=5, amp=8)
    pkts[0] = pkts[0].copy()
    pkts[0][10] = 0
    decode_stream(fmt, pkts)  # the second packet switches to quality 192


@pytest.mark.parametrize("fmt", (F.FMT_422, F.FMT_GREY))
def test_size_and_quality_change_mid_stream(fmt):
    small, large = ((48, 24), (176, 40)) if fmt == F.FMT_422 else ((24, 8), (136, 72))
    pkts = F.make_packets(fmt, *small, 255, 2, seed=6, amp=64) + F.make_packets(fmt, *small, 128, 1, seed=7) + \
        F.make_packets(fmt, *large, 128, 1, seed=8) + F.make_packets(fmt, *large, 224, 2, seed=9, amp=64)
    decode_stream(fmt, pkts)


@pytest.mark.parametrize("fmt,w,h", [(F.FMT_422, 176, 40), (F.FMT_GREY, 136, 72)])
def test_decode_with_crop_and_foreign_strides(fmt, w, h):
    pkt = F.make_packets(fmt, w, h, 224, 1, seed=11, amp=8)[0]
    want = np.zeros(F.plane_bytes(fmt, w, h), np.uint8)
    F.Restated(fmt).decode(pkt, want)
    cw, ch = w - 11, h - 3
    strides = (cw + 13, (cw + 1) // 2 + 5, (cw + 1) // 2 + 5)
    ccw, cch = (cw + 1) // 2, ch
    out = np.full(strides[0] * ch + 2 * strides[1] * cch, PREFILL, np.uint8)
    dev = instance(fmt)
    dev.decode(pkt, out, crop=(cw, ch), strides=strides)
    y, cb, cr = F.split(fmt, want, w, h)
    gy = out[:strides[0] * ch].reshape(ch, strides[0])
    assert np.array_equal(gy[:, :cw], y.reshape(h, w)[:ch, :cw])
    assert np.all(gy[:, cw:] == PREFILL)
    rest = out[strides[0] * ch:]
    if fmt == F.FMT_GREY:
        assert np.all(rest == PREFILL)  # the chroma arguments are not looked at: nothing is written there
    else:
        for k, plane in enumerate((cb, cr)):
            g = rest[k * strides[1] * cch:(k + 1) * strides[1] * cch].reshape(cch, strides[1])
            assert np.array_equal(g[:, :ccw], plane.reshape(h, w // 2)[:cch, :ccw]), k
            assert np.all(g[:, ccw:] == PREFILL)
    dev.close()


# ---- plans ----
def mixed_packets(fmt, count=70):
    shapes = [s[1:] for s in SMALL if s[0] == fmt]
    pkts = []
    for i in range(count):
        w, h = shapes[i % 2] if i % 7 else (320, 88)
        Q = QUALITIES[i % 5]
        key = 2 if i % 3 == 0 else 0
        got = F.make_packets(fmt, w, h, Q, 2 if key else 1, seed=100 + i, amp=(0, 8, 64)[i % 3], key_rate=key)
        pkts.append(got[-1])  # (with a key rate: the stream's second packet, the one with unchanged blocks)
    return pkts


@pytest.mark.parametrize("fmt", (F.FMT_422, F.FMT_GREY))
def test_one_plan_of_mixed_sizes_and_qualities(fmt):
    pkts = mixed_packets(fmt)
    dev = instance(fmt)
    d_st, po, pl, hdrs = dev.upload_packets(pkts, align=1)
    sizes = [F.plane_bytes(fmt, *F.header_of(p)[:2]) for p in pkts]
    oo = np.zeros(len(pkts), np.uint64)
    cur = 0
    for i, s in enumerate(sizes):
        oo[i] = cur
        cur += (s + 255) // 256 * 256
    d_out = dev.alloc(cur)
    plan = dev.plan(hdrs, po, pl, oo)
    assert plan.fmt == fmt
    # the restatement: one decoder sees the plan's headers in order (quality and size changes), every picture into a
    # slot of its own that starts as the prefill
    dec = F.Restated(fmt)
    want, want_idx, blocks = [], [], 0
    for p, s in zip(pkts, sizes):
        out = np.full(s, PREFILL, np.uint8)
        _, offs = dec.decode(p, out)
        want.append(out)
        want_idx.append(offs)
        blocks += offs.size - 1
    # a block of one byte is an unchanged (0xFF) block — any other has its DC and at least one token: those leave the prefill
    assert sum(int(np.count_nonzero(np.diff(o.astype(np.int64)) == 1)) for o in want_idx) > 100
    for launch in range(2):  # twice over the same buffers
        dev.memset(d_out, PREFILL, cur)
        plan.decode(d_st, d_out)
        dev.sync()
        whole = dev.d2h(d_out, cur)
        for i, s in enumerate(sizes):
            got = whole[int(oo[i]):int(oo[i]) + s]
            assert first_diff(got, want[i]) is None, (launch, i, F.header_of(pkts[i]), first_diff(got, want[i]))
            gap = whole[int(oo[i]) + s:int(oo[i + 1]) if i + 1 < len(sizes) else cur]
            assert np.all(gap == PREFILL), (launch, i)
        assert np.array_equal(plan.read_index(), np.concatenate(want_idx))
    info = plan.info()
    assert info == dict(frames=len(pkts), blocks=blocks, bytes_in=sum(p.size for p in pkts), bytes_out=sum(sizes))
    assert plan.spec_stats() == (0, 0)
    assert plan.decode_form() == (-1, 0, 0)
    assert plan.overlapped() is False
    # the index is MI_RTJ_K_EMIT's time, the transform MI_RTJ_K_DECODE's
    plan.profile(True)
    plan.decode(d_st, d_out)
    ms, n = plan.times()
    assert n == 1 and ms["k_index_emit"] > 0 and ms["k_decode"] > 0
    assert all(v == 0 for k, v in ms.items() if k not in ("k_index_emit", "k_decode"))
    assert len(plan.step_times()) == 1
    plan.profile(False)
    # runs are for 4:2:0 plans: refused, and the plan decodes as before
    rc, msg = rc_of(dev, lambda: plan.set_runs([len(pkts)]))
    assert rc == ERR_ARG and "4:2:0" in msg
    dev.memset(d_out, PREFILL, cur)
    plan.decode(d_st, d_out)
    dev.sync()
    whole = dev.d2h(d_out, cur)
    assert all(first_diff(whole[int(oo[i]):int(oo[i]) + s], want[i]) is None for i, s in enumerate(sizes))
    plan.close()
    dev.free(d_st)
    dev.free(d_out)
    dev.close()


# ---- hostile input ----
def plan_decode_each(fmt, pkts):
    """every packet alone through a fresh header state: a plan of one packet on a fresh instance"""
    for i, pkt in enumerate(pkts):
        w, h, _ = F.header_of(pkt)
        n = F.plane_bytes(fmt, w, h)
        want = np.full(n, PREFILL, np.uint8)
        used, offs = F.Restated(fmt).decode(pkt, want)
        dev = instance(fmt)
        d_st, po, pl, hdrs = dev.upload_packets([pkt])
        d_out = dev.alloc(n)
        dev.memset(d_out, PREFILL, n)
        plan = dev.plan(hdrs, po, pl, np.zeros(1, np.uint64))
        plan.decode(d_st, d_out)
        dev.sync()
        got = dev.d2h(d_out, n)
        assert first_diff(got, want) is None, (i, first_diff(got, want))
        assert np.array_equal(plan.read_index(), offs), i
        plan.close()
        dev.free(d_st)
        dev.free(d_out)
        dev.close()


@pytest.mark.parametrize("fmt,w,h", [(F.FMT_422, 176, 40), (F.FMT_GREY, 136, 72)])
def test_packets_cut_in_the_middle_of_a_block(fmt, w, h):
    pkt = F.make_packets(fmt, w, h, 255, 1, seed=21, amp=64)[0]
    offs = F.Restated(fmt).decode(pkt, np.zeros(F.plane_bytes(fmt, w, h), np.uint8))[1].astype(np.int64)
    cuts = [F.HEADER + int(offs[k]) + d for k, d in ((1, 0), (5, 1), (offs.size // 2, 7), (offs.size - 2, 3))] + [F.HEADER, 5]
    plan_decode_each(fmt, [pkt[:c].copy() for c in cuts if c >= F.HEADER])
    # (a packet shorter than its header is refused by the one-packet path and zero-padded by a plan's caller: not a stream)


@pytest.mark.parametrize("fmt", (F.FMT_422, F.FMT_GREY))
def test_packets_of_longest_and_shortest_blocks(fmt):
    """the serial walker's window slide and offset stores: 64-byte blocks, 1-byte blocks, run tokens and their mixtures
    in the format's block pattern (tests/edge_packets.py; tests/test_rtjfmt_cpu.py holds the expectation to the
    reference's own decoder)"""
    pkts = E.format_boundary_packets(fmt)
    assert len(pkts) == 6 and F.nblocks(fmt, *F.header_of(pkts[0])[:2]) in (132, 153)
    plan_decode_each(fmt, pkts)


@pytest.mark.parametrize("fmt,w,h", [(F.FMT_422, 176, 40), (F.FMT_GREY, 136, 72)])
def test_seeded_packets_of_random_bytes(fmt, w, h):
    rng = np.random.default_rng([31, fmt])
    dev, dec = instance(fmt), F.Restated(fmt)
    n = F.plane_bytes(fmt, w, h)
    want = np.zeros(n, np.uint8)
    for i in range(32):
        pkt = rng.integers(0, 256, int(rng.integers(F.HEADER, 6000)), dtype=np.uint8)
        if i % 4 == 1:
            pkt[F.HEADER:][rng.random(pkt.size - F.HEADER) < 0.3] = 0xFF  # many unchanged blocks
        if i % 4 == 2:
            pkt[F.HEADER:] &= 0x7F  # zero runs
        pkt[6], pkt[7], pkt[8], pkt[9] = w & 255, w >> 8, h & 255, h >> 8
        pkt[10] = (0, 1, 128, 192, 224, 255, 77, 200)[i % 8]
        assert dec.decode(pkt, want) is not None
        got = np.zeros(n, np.uint8)
        dev.decode(pkt, got)
        assert first_diff(got, want) is None, (i, first_diff(got, want))
    dev.close()


# ---- refusals ----
def header(w, h, q=128):
    p = np.zeros(64, np.uint8)
    p[6], p[7], p[8], p[9], p[10] = w & 255, w >> 8, h & 255, h >> 8, q
    return p


def test_geometry_per_format():
    pkt422 = F.make_packets(F.FMT_422, 48, 24, 224, 1)[0]
    d420 = P.MiRtj()
    rc, _ = rc_of(d420, lambda: d420.decode(pkt422))  # 48 x 24: not a 4:2:0 picture ...
    assert rc == ERR_GEOMETRY
    d420.close()
    decode_stream(F.FMT_422, [pkt422])  # ... and a legal 4:2:2 one
    for fmt, bad in ((F.FMT_422, [(40, 24), (48, 20), (0, 24), (48, 0)]), (F.FMT_GREY, [(20, 8), (24, 12), (0, 8), (24, 0)])):
        dev = instance(fmt)
        for w, h in bad:
            rc, _ = rc_of(dev, lambda: dev.decode(header(w, h)))
            assert rc == ERR_GEOMETRY, (fmt, w, h)
            hd = header(w, h)[:12].reshape(1, 12)
            with pytest.raises(P.MiRtjError, match="plan_create failed: packet header %dx%d: .*multiple" % (w, h)):
                dev.plan(hd, np.zeros(1, np.uint64), np.array([64], np.uint32), np.zeros(1, np.uint64))
        dev.close()
        good = (48, 24) if fmt == F.FMT_422 else (24, 8)
        decode_stream(fmt, F.make_packets(fmt, *good, 128, 1))  # an instance still works (a fresh one: see below)


@pytest.mark.parametrize("fmt", (F.FMT_422, F.FMT_GREY))
def test_an_instance_still_works_after_a_refused_packet(fmt):
    w, h = (48, 24) if fmt == F.FMT_422 else (24, 8)
    pkt = F.make_packets(fmt, w, h, 128, 1)[0]
    dev = instance(fmt)
    rc, _ = rc_of(dev, lambda: dev.decode(header(20, 20)))
    assert rc == ERR_GEOMETRY
    want = np.zeros(F.plane_bytes(fmt, w, h), np.uint8)
    F.Restated(fmt).decode(pkt, want)
    got = np.zeros_like(want)
    dev.decode(pkt, got)
    assert first_diff(got, want) is None
    dev.close()


def test_set_format_rules():
    dev = P.MiRtj()
    for bad in (3, -1, 99):
        rc, msg = rc_of(dev, lambda: dev.set_format(bad))
        assert rc == ERR_ARG and "format" in msg
    assert dev.format == B.FMT_YUV420
    dev.set_format(B.FMT_GREY)
    dev.set_format(B.FMT_YUV422)  # before the first decode: free to change
    pkt = F.make_packets(F.FMT_422, 48, 24, 128, 1)[0]
    want = np.zeros(F.plane_bytes(F.FMT_422, 48, 24), np.uint8)
    F.Restated(F.FMT_422).decode(pkt, want)
    got = np.zeros_like(want)
    dev.decode(pkt, got)
    for other in (B.FMT_YUV420, B.FMT_GREY):
        rc, msg = rc_of(dev, lambda: dev.set_format(other))
        assert rc == ERR_ARG and "format" in msg
    dev.set_format(B.FMT_YUV422)
    assert dev.format == B.FMT_YUV422
    got[:] = 0
    dev.decode(pkt, got)  # still works
    assert first_diff(got, want) is None
    dev.close()
    # a plan fixes the format as well
    dev = instance(F.FMT_GREY)
    pkt = F.make_packets(F.FMT_GREY, 24, 8, 128, 1)[0]
    d_st, po, pl, hdrs = dev.upload_packets([pkt])
    plan = dev.plan(hdrs, po, pl, np.zeros(1, np.uint64))
    rc, _ = rc_of(dev, lambda: dev.set_format(B.FMT_YUV420))
    assert rc == ERR_ARG
    plan.close()
    dev.free(d_st)
    dev.close()


@pytest.mark.parametrize("fmt", (F.FMT_422, F.FMT_GREY))
def test_sessions_are_refused_and_the_instance_goes_on(fmt):
    dev = instance(fmt)
    with pytest.raises(P.MiRtjError, match="4:2:0.*(4:2:2|greyscale)"):
        dev.pipe(depth=4)
    w, h = (48, 24) if fmt == F.FMT_422 else (24, 8)
    pkt = F.make_packets(fmt, w, h, 128, 1)[0]
    want = np.zeros(F.plane_bytes(fmt, w, h), np.uint8)
    F.Restated(fmt).decode(pkt, want)
    got = np.zeros_like(want)
    dev.decode(pkt, got)
    assert first_diff(got, want) is None
    dev.close()


# ---- colour ----
@pytest.mark.parametrize("w,h", [(48, 24), (640, 360)])
def test_yuv422_to_rgb24(w, h):
    n = 3
    fsz = F.plane_bytes(F.FMT_422, w, h)
    in_stride = (fsz + 255) // 256 * 256
    pitch = (3 * w + 16 + 15) // 16 * 16
    out_stride = pitch * h + 32
    rng = np.random.default_rng([41, w])
    src = rng.integers(0, 256, in_stride * n, dtype=np.uint8)
    want = np.full(out_stride * n, PREFILL, np.uint8)
    for i in range(n):
        F.yuv422_to_rgb24(w, h, src[i * in_stride:i * in_stride + fsz], want[i * out_stride:i * out_stride + pitch * h], pitch)
    dev = instance(F.FMT_422)
    d_in, d_out = dev.alloc(src.size), dev.alloc(want.size)
    dev.h2d(d_in, src)
    dev.memset(d_out, PREFILL, want.size)
    dev.to_rgb422(w, h, n, d_in, in_stride, d_out, pitch, out_stride)
    dev.sync()
    got = dev.d2h(d_out, want.size)
    assert first_diff(got, want) is None, first_diff(got, want)  # (the bytes between rows and frames are part of it)
    rc, _ = rc_of(dev, lambda: dev.to_rgb422(w + 8, h, n, d_in, in_stride, d_out, pitch, out_stride))
    assert rc == ERR_ARG
    dev.free(d_in)
    dev.free(d_out)
    dev.close()
