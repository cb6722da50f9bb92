"""Parity tests proper: the HIP path, called through the C ABI (libmi_rtjpeg.so), against the CPU
oracle and the committed golden vectors.  Bit-exact everywhere — this is integer/byte work.
Run on the GPU box with `pytest -m gpu`."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import edge_packets as E
import launch_shapes as LS
import rtjlib as R
from pkg import P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    d = P.MiRtj()
    yield d
    d.close()


@pytest.fixture(scope="module")
def G():
    return np.load(R.GOLDEN + "/rtjpeg_golden.npz")


def frame_bytes(w, h):
    return w * h * 3 // 2


def first_diff(a, b):
    d = np.nonzero(a != b)[0]
    return None if d.size == 0 else (int(d[0]), int(a[d[0]]), int(b[d[0]]), int(d.size))


WORKERS = 16  # oracle work runs on a pool of this size at most, whatever the machine has


def pmap(fn, items):
    items = list(items)
    with ThreadPoolExecutor(max_workers=max(1, min(WORKERS, len(items)))) as ex:
        return list(ex.map(fn, items))


def oracle_digests(pkts):
    """digest of the oracle's picture of every packet, each decoded on its own into zeros"""
    def one(p):
        want = np.zeros(frame_bytes(*packet_size(p)), np.uint8)
        R.OracleDecoder().decode(p, want)
        return R.digest(want)
    return pmap(one, pkts)


def device_digests(dev, d_out, fsz, n):
    """digest of every picture of an output buffer of n pictures of fsz bytes (read back one at a time)"""
    return pmap(R.digest, [dev.d2h(d_out, fsz, offset=k * fsz) for k in range(n)])


def explain_picture(dev, d_out, fsz, k, pkt, cls, form, frames, split):
    """the assertion message for picture k of a launch, whose digest is not the oracle's"""
    w, h = packet_size(pkt)
    got = dev.d2h(d_out, fsz, offset=k * fsz)
    want = np.zeros(fsz, np.uint8)
    R.OracleDecoder().decode(pkt, want)
    d = np.nonzero(got != want)[0]
    if d.size == 0:
        return f"class {cls}, form {form}, picture {k}: digest differs, bytes read back again do not"
    off = int(d[0])
    return (f"class {cls} ({w}x{h}), form {form}, picture {k} of {frames}: {d.size} bytes differ from the oracle, first at "
            f"byte {off}: got {int(got[off])} want {int(want[off])}; "
            + LS.Shapes().describe_byte(w, h, off, "split" if split else "classic", frame=k, frames=frames))


def packet_size(p):
    return int(p[6]) | (int(p[7]) << 8), int(p[8]) | (int(p[9]) << 8)


def batch_layout(sizes, guard=0, odd16=False):
    """out_offset of every picture and the size of the output buffer.  Pictures start at multiples of 256 — with odd16
    every other one at a multiple of 16 that is not one of 256 (the contract of mi_rtj_plan_create is 16) — and `guard`
    bytes lie before the first, between any two and behind the last."""
    oo = np.zeros(len(sizes), np.uint64)
    cur = guard
    for i, s in enumerate(sizes):
        cur = (cur + 255) // 256 * 256
        if odd16 and i % 2:
            cur += 16 * (1 + (i // 2) % 15)
        oo[i] = cur
        cur += s + guard
    return oo, max(cur, 1)


def batch_decode(dev, pkts, prefill=None, align=1, check_index=True, guard=0, odd16=False, report=None, launches=1):
    """Independent decode of each packet through a plan.  Returns list of plane arrays.
    guard / odd16: see batch_layout(); every byte of the output buffer outside the pictures must come back as it was
    filled.  launches: decodes queued back to back without a sync in between.  report: a dict that receives what the
    plan says about the launch (decode_form(), overlapped())."""
    d_stream, po, pl, hdrs = dev.upload_packets(pkts, align=align)
    sizes = [frame_bytes(*packet_size(p)) for p in pkts]
    oo, total = batch_layout(sizes, guard, odd16)
    fill = 0 if prefill is None else prefill
    d_out = dev.alloc(total)
    dev.memset(d_out, fill, total)
    plan = dev.plan(hdrs, po, pl, oo)
    for _ in range(launches):
        plan.decode(d_stream, d_out)
    dev.sync()
    if report is not None:
        report["form"], report["classic_left"], report["parts_listed"] = plan.decode_form()
        report["overlapped"] = plan.overlapped()
        report["out_offsets"] = oo.copy()
    whole = dev.d2h(d_out, total)
    outs = [whole[int(oo[i]):int(oo[i]) + sizes[i]] for i in range(len(pkts))]
    at = 0
    for i in range(len(pkts) + 1):  # the gaps: guards and alignment padding
        end = int(oo[i]) if i < len(pkts) else total
        bad = np.nonzero(whole[at:end] != fill)[0]
        assert bad.size == 0, (f"byte {at + int(bad[0])} of the output buffer, {int(oo[i - 1]) + sizes[i - 1] if i else 0} + "
                               f"{int(bad[0])} (outside every picture, before picture {i}) was written: "
                               f"{int(whole[at + bad[0]])} instead of {fill} ({bad.size} bytes of the gap)")
        if i < len(pkts):
            at = end + sizes[i]
    if check_index:
        idx = plan.read_index()
        k = 0
        dec = R.OracleDecoder()
        for i, p in enumerate(pkts):
            want = dec.block_offsets(p).astype(np.int64) - 12
            got = idx[k:k + want.size].astype(np.int64)
            k += want.size
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, f"block index of packet {i}: first mismatch at block {bad[0]}: got {got[bad[0]]} want {want[bad[0]]} ({bad.size} wrong of {want.size})"
    plan.close()
    dev.free(d_stream)
    dev.free(d_out)
    return outs


# --------------------------------------------------------------------------- golden vectors
def test_golden_intra_streams_batch(dev, G):
    pkts = [G[f"intra{ci}_{n}_pkt"] for (ci, n, *_) in G["intra_meta"]]
    outs = batch_decode(dev, pkts, align=1)
    for (ci, n, *_), got in zip(G["intra_meta"], outs):
        assert first_diff(got, G[f"intra{ci}_{n}_planes"]) is None, (ci, n)


def test_golden_adversarial_known_answers(dev, G):
    pkts = [G[f"kat_{ki}_pkt"] for (ki, *_) in G["kat_meta"]]
    outs = batch_decode(dev, pkts, prefill=99)
    for (ki, *_), got in zip(G["kat_meta"], outs):
        assert first_diff(got, G[f"kat_{ki}_planes"]) is None, ki


def test_golden_inter_sequence_single_stream(dev, G):
    """0xFF blocks keep the previous picture: the one-packet path holds it on the device like
    priv->frame (lib/video_rtjpeg.c:31-35)."""
    w, h, Q, key, lm, cm, nfr = [int(x) for x in G["inter_meta"]]
    d = P.MiRtj()
    out = np.zeros(frame_bytes(w, h), np.uint8)
    for n in range(nfr):
        d.decode(G[f"inter_{n}_pkt"], out)
        assert first_diff(out, G[f"inter_{n}_planes"]) is None, n
    assert d.state() == (w, h, Q)
    d.close()


# --------------------------------------------------------------------------- oracle, seeded
@pytest.mark.parametrize("w,h,Q,amp,n", [(16, 16, 255, 8, 3), (64, 48, 200, 30, 4), (320, 240, 255, 8, 6),
                                          (320, 240, 128, 64, 3), (336, 256, 1, 64, 2), (1920, 1088, 255, 8, 2),
                                          (1920, 1088, 64, 64, 1), (4096, 16, 90, 20, 2), (16, 2048, 255, 64, 2),
                                          (65520, 16, 255, 8, 1), (16, 65520, 200, 30, 1)])  # the header's 16-bit limits
def test_decode_matches_oracle(dev, w, h, Q, amp, n):
    enc = R.OracleEncoder(w, h, Q)
    pkts = [enc.encode(R.synth_frame(w, h, i, seed=11, amp=amp)) for i in range(n)]
    outs = batch_decode(dev, pkts, align=1)  # align=1: packets start at arbitrary byte addresses
    dec = R.OracleDecoder()
    for i, (p, got) in enumerate(zip(pkts, outs)):
        want = np.zeros(frame_bytes(w, h), np.uint8)
        dec.decode(p, want)
        assert first_diff(got, want) is None, (i, first_diff(got, want))


def test_mixed_batch_sizes_and_qualities(dev):
    """cfg 5 shape: one plan holding packets of different geometry and quality."""
    rng = np.random.default_rng(5)
    pkts = []
    for i in range(24):
        w, h = [(320, 240), (64, 48), (640, 368), (176, 144)][i % 4]
        Q = int(rng.choice([64, 128, 255, 30]))
        pkts.append(R.OracleEncoder(w, h, Q).encode(R.synth_frame(w, h, i, seed=i, amp=int(rng.integers(0, 60)))))
    outs = batch_decode(dev, pkts, align=1)
    dec = R.OracleDecoder()  # the plan applies the header state machine in order, like one decoder
    for i, (p, got) in enumerate(zip(pkts, outs)):
        w, h = int(p[6]) | (int(p[7]) << 8), int(p[8]) | (int(p[9]) << 8)
        want = np.zeros(frame_bytes(w, h), np.uint8)
        dec.decode(p, want)
        assert first_diff(got, want) is None, i


def test_skip_blocks_leave_destination_untouched_in_batches(dev):
    w, h, Q = 320, 240, 200
    enc = R.OracleEncoder(w, h, Q, key_rate=6, lmask=3, cmask=3)
    pkts = [enc.encode(R.synth_frame(w, h, n // 4, seed=9, amp=2)) for n in range(8)]
    assert any((p[12:] == 255).any() for p in pkts)
    outs = batch_decode(dev, pkts, prefill=0x5A)
    for p, got in zip(pkts, outs):
        want = np.full(frame_bytes(w, h), 0x5A, np.uint8)
        R.OracleDecoder().decode(p, want)
        assert first_diff(got, want) is None


def test_random_token_streams(dev):
    """Adversarial blocks (random bytes, random runs, some 0xFF) at qualities where the int16
    narrowing of RTjpeg_s2b and DESCALE is observable."""
    pkts, qs = E.adversarial_packets(seed=2025)
    # each packet gets its own decoder state in the oracle; do the same on the device
    for p, Q in zip(pkts, qs):
        w, h = int(p[6]) | (int(p[7]) << 8), int(p[8]) | (int(p[9]) << 8)
        d = P.MiRtj()
        got = np.full(frame_bytes(w, h), 7, np.uint8)
        want = got.copy()
        # pre-seed the device picture so that skipped blocks are comparable
        d.decode(R.OracleEncoder(w, h, 100).encode(R.synth_frame(w, h, 0)), got)
        od = R.OracleDecoder()
        od.decode(R.OracleEncoder(w, h, 100).encode(R.synth_frame(w, h, 0)), want)
        d.decode(p, got)
        od.decode(p, want)
        assert first_diff(got, want) is None, Q
        d.close()


def test_truncated_and_empty_packets(dev):
    w, h = 64, 32
    pkt = R.OracleEncoder(w, h, 255).encode(R.synth_frame(w, h, 0, amp=30))
    cases = [pkt[:12], pkt[:13], pkt[: 12 + 40], pkt[: pkt.size // 2], pkt[:-1]]
    outs = batch_decode(dev, cases)
    for c, got in zip(cases, outs):
        want = np.zeros(frame_bytes(w, h), np.uint8)
        R.OracleDecoder().decode(c, want)
        assert first_diff(got, want) is None, c.size


def test_quality_zero_state_machine(dev):
    w, h = 32, 16
    enc = R.OracleEncoder(w, h, 100)
    p0 = enc.encode(R.synth_frame(w, h, 0))
    p0[10] = 0
    p1 = enc.encode(R.synth_frame(w, h, 1))
    d, od = P.MiRtj(), R.OracleDecoder()
    got = np.zeros(frame_bytes(w, h), np.uint8)
    want = got.copy()
    for p in (p0, p1, p0):
        d.decode(p, got)
        od.decode(p, want)
        assert first_diff(got, want) is None
        assert d.state()[2] == od.quality()
    d.close()


def test_bad_geometry_and_arguments(dev):
    pkt = np.zeros(64, np.uint8)
    pkt[4], pkt[6], pkt[8], pkt[10] = 12, 24, 16, 100
    with pytest.raises(P.MiRtjError, match="multiples of 16"):
        dev.decode(pkt, np.zeros(24 * 16 * 3 // 2, np.uint8))
    with pytest.raises(P.MiRtjError, match="header"):
        dev.decode(pkt[:5], None)


def test_nocopy_path_returns_the_whole_coded_picture(dev):
    w, h = 320, 240
    enc = R.OracleEncoder(w, h, 230, key_rate=3, lmask=2, cmask=2)
    d, od = P.MiRtj(), R.OracleDecoder()
    want = np.zeros(frame_bytes(w, h), np.uint8)
    for i in range(5):
        pkt = enc.encode(R.synth_frame(w, h, i // 2, seed=2, amp=3))
        y, u, v = d.decode_nocopy(pkt)
        od.decode(pkt, want)
        assert first_diff(np.concatenate([y, u, v]), want) is None, i
    d.close()


def test_crop_and_strides_like_gavl_frame_copy(dev):
    """1080p is coded as 1920x1088 and handed back as the 1920x1080 crop with the caller's strides
    (lib/video_rtjpeg.c:50-51,82)."""
    w, h, cw, ch = 1920, 1088, 1920, 1080
    pkt = R.OracleEncoder(w, h, 255).encode(R.synth_frame(w, h, 3))
    want_full = np.zeros(frame_bytes(w, h), np.uint8)
    R.OracleDecoder().decode(pkt, want_full)
    strides = (2048, 1024, 1024)
    out = np.full(strides[0] * ch + 2 * strides[1] * (ch // 2), 0xEE, np.uint8)
    d = P.MiRtj()
    d.decode(pkt, out, crop=(cw, ch), strides=strides)
    y = out[: strides[0] * ch].reshape(ch, strides[0])
    u = out[strides[0] * ch: strides[0] * ch + strides[1] * (ch // 2)].reshape(ch // 2, strides[1])
    v = out[strides[0] * ch + strides[1] * (ch // 2):].reshape(ch // 2, strides[1])
    wy = want_full[: w * h].reshape(h, w)
    wu = want_full[w * h: w * h * 5 // 4].reshape(h // 2, w // 2)
    wv = want_full[w * h * 5 // 4:].reshape(h // 2, w // 2)
    assert np.array_equal(y[:, :cw], wy[:ch, :cw]) and (y[:, cw:] == 0xEE).all()
    assert np.array_equal(u[:, : cw // 2], wu[: ch // 2, : cw // 2]) and (u[:, cw // 2:] == 0xEE).all()
    assert np.array_equal(v[:, : cw // 2], wv[: ch // 2, : cw // 2])
    d.close()


def test_serial_and_parallel_index_agree(dev, monkeypatch):
    """MI_RTJ_INDEX=serial keeps the one-wave-per-packet walker as an A/B baseline of the
    chunk-parallel index; both must produce the oracle's offsets (batch_decode checks them)."""
    w, h = 640, 368
    pkts = [R.OracleEncoder(w, h, Q).encode(R.synth_frame(w, h, i, seed=4, amp=a))
            for i, (Q, a) in enumerate([(255, 8), (255, 64), (40, 64), (128, 0), (200, 120)])]
    inter = R.OracleEncoder(w, h, 180, key_rate=3, lmask=4, cmask=4)
    pkts += [inter.encode(R.synth_frame(w, h, n // 2, seed=8, amp=3)) for n in range(4)]
    want = []
    for p in pkts:
        o = np.zeros(frame_bytes(w, h), np.uint8)
        R.OracleDecoder().decode(p, o)
        want.append(o)
    for mode in ("serial", "parallel"):
        monkeypatch.setenv("MI_RTJ_INDEX", mode)
        outs = batch_decode(dev, pkts)
        for o, wnt in zip(outs, want):
            assert first_diff(o, wnt) is None, mode


def test_chunk_boundaries_and_long_blocks(dev):
    """Streams built to stress the chunked index: maximal 64-byte blocks (no zero runs), minimal
    1-byte (0xFF) blocks, and mixtures, so macroblocks straddle every chunk boundary differently."""
    w, h = 1024, 256  # 1024 macroblocks: long-block packets span ~110 chunks
    pkts = E.chunk_boundary_packets(seed=77, w=w, h=h)
    outs = batch_decode(dev, pkts, prefill=3)
    for p, got in zip(pkts, outs):
        want = np.full(frame_bytes(w, h), 3, np.uint8)
        R.OracleDecoder().decode(p, want)
        assert first_diff(got, want) is None


def test_fuzz_arbitrary_bytes(dev):
    """Packets whose payload is arbitrary bytes (not produced by any encoder): every value of the
    DC / raw / token bytes, runs that overshoot the block, 0xFF in every position, payloads far
    shorter or longer than the picture needs.  The behaviour is fully defined (oracle header) and
    the device must match it and must not fault."""
    rng = np.random.default_rng(4242)
    pkts = []
    for trial in range(40):
        w, h = [(16, 16), (48, 32), (160, 64), (320, 240), (16, 512)][trial % 5]
        Q = int(rng.choice([0, 1, 2, 17, 100, 129, 200, 255]))
        nblk = (w // 16) * (h // 16) * 6
        n = int(rng.integers(0, nblk * 70))
        kind = trial % 4
        if kind == 0:
            body = rng.integers(0, 256, n, dtype=np.uint8)
        elif kind == 1:  # run-heavy
            body = rng.choice(np.array([0x40, 0x7F, 0x7E, 0x00, 0xFF, 0x3F, 0x80], np.uint8), n)
        elif kind == 2:  # mostly small coefficients, occasional anything
            body = rng.integers(0, 8, n, dtype=np.uint8)
            m = rng.random(n) < 0.05
            body[m] = rng.integers(0, 256, int(m.sum()), dtype=np.uint8)
        else:            # many skip markers
            body = rng.choice(np.array([0xFF, 0xFF, 0x10, 0x7F], np.uint8), n)
        total = 12 + n
        hdr = np.array([total & 255, (total >> 8) & 255, (total >> 16) & 255, (total >> 24) & 255, 12, 0,
                        w & 255, w >> 8, h & 255, h >> 8, Q, 0], np.uint8)
        pkts.append(np.concatenate([hdr, body]))
    # the plan applies the header state machine across the batch starting from the instance's
    # state (a quality-0 header means "zero tables" only on a fresh decoder): mirror it in the oracle
    q_before = dev.state()[2]
    outs = batch_decode(dev, pkts, prefill=0x21, check_index=False)
    dec = R.OracleDecoder()
    if q_before:
        dec.decode(R.OracleEncoder(16, 16, q_before).encode(R.synth_frame(16, 16, 0)), np.zeros(384, np.uint8))
    for i, (p, got) in enumerate(zip(pkts, outs)):
        w, h = int(p[6]) | (int(p[7]) << 8), int(p[8]) | (int(p[9]) << 8)
        want = np.full(frame_bytes(w, h), 0x21, np.uint8)
        dec.decode(p, want)
        assert first_diff(got, want) is None, (i, first_diff(got, want))


def test_low_4x4_transform_path_and_its_boundary(dev):
    """k_decode runs a four-input transform when no block of a wave has a coefficient outside the low
    4x4, and a three-input one when none reaches row 3 or column 3 either.  Packets are built so that whole waves qualify, whole waves do not, a wave stops qualifying from
    one macroblock group to the next, and the single coefficient sits on every one of the 63 AC slots
    (inside, on the edge of and outside the 4x4) with values where the int16 narrowing shows."""
    pkts = E.low_4x4_packets(seed=99)
    outs = batch_decode(dev, pkts, prefill=0x33)
    dec = R.OracleDecoder()
    for i, (p, got) in enumerate(zip(pkts, outs)):
        w, h = int(p[6]) | (int(p[7]) << 8), int(p[8]) | (int(p[9]) << 8)
        want = np.full(frame_bytes(w, h), 0x33, np.uint8)
        dec.decode(p, want)
        assert first_diff(got, want) is None, (i, first_diff(got, want))


@pytest.mark.parametrize("w,h,Q", [(320, 240, 255), (1920, 1088, 255), (640, 368, 128), (320, 240, 20)])
def test_flat_and_half_flat_content(dev, w, h, Q):
    """Encoder-made streams whose luma waves take the low-4x4 path (flat gradient), do not (noise), and
    pictures that are flat on the left and noisy on the right."""
    flat = R.synth_frame(w, h, 0, amp=0)
    noisy = R.synth_frame(w, h, 1, amp=40)
    half = flat.copy()
    y = half[: w * h].reshape(h, w)
    y[:, w // 2:] = noisy[: w * h].reshape(h, w)[:, w // 2:]
    enc = R.OracleEncoder(w, h, Q)
    pkts = [enc.encode(f) for f in (flat, half, noisy, flat)]
    outs = batch_decode(dev, pkts)
    dec = R.OracleDecoder()
    for i, (p, got) in enumerate(zip(pkts, outs)):
        want = np.zeros(frame_bytes(w, h), np.uint8)
        dec.decode(p, want)
        assert first_diff(got, want) is None, (i, first_diff(got, want))


# --------------------------------------------------------------------------- generator side (N1)
@pytest.mark.parametrize("w,h,amp", [(64, 48, 8), (320, 240, 64), (1920, 1088, 8)])
def test_synth_matches_numpy_twin(dev, w, h, amp):
    n = 3
    d = dev.synth(w, h, 5, n, seed=777, amp=amp)
    dev.sync()
    got = dev.d2h(d, frame_bytes(w, h) * n)
    dev.free(d)
    for i in range(n):
        want = R.synth_frame(w, h, 5 + i, seed=777, amp=amp)
        assert first_diff(got[i * want.size:(i + 1) * want.size], want) is None, i


@pytest.mark.parametrize("w,h,Q,amp", [(64, 48, 255, 8), (320, 240, 128, 64), (320, 240, 1, 64), (1920, 1088, 255, 8)])
def test_encoder_matches_oracle_bytes(dev, w, h, Q, amp):
    n = 3
    d_fr = dev.synth(w, h, 0, n, seed=31, amp=amp)
    d_st, po, pl = dev.encode(w, h, Q, n, d_fr, align=1)
    dev.sync()
    for i in range(n):
        got = dev.d2h(d_st, int(pl[i]), offset=int(po[i]))
        want = R.OracleEncoder(w, h, Q).encode(R.synth_frame(w, h, i, seed=31, amp=amp))
        assert got.size == want.size and first_diff(got, want) is None, i
    dev.free(d_fr)
    dev.free(d_st)


@pytest.mark.parametrize("w,h,Q,key_rate,lm,cm", [(320, 240, 200, 4, 2, 2), (160, 128, 255, 255, 16, 16), (64, 48, 90, 1, 0, 0)])
def test_stream_encoder_with_skip_blocks_matches_oracle(dev, w, h, Q, key_rate, lm, cm):
    """mi_rtj_encode_stream == RTjpeg_compress with RTjpeg_set_intra(key_rate, lmask, cmask): same bytes,
    same key counter in the header, and the packets decode in order to the oracle's pictures."""
    n = 9
    frames = [R.synth_frame(w, h, i // 3, seed=13, amp=3) for i in range(n)]  # repeats -> unchanged blocks
    d_fr = dev.alloc(frame_bytes(w, h) * n)
    dev.h2d(d_fr, np.concatenate(frames))
    d_st, po, pl = dev.encode(w, h, Q, n, d_fr, align=1, key_rate=key_rate, lmask=lm, cmask=cm)
    dev.sync()
    enc = R.OracleEncoder(w, h, Q, key_rate, lm, cm)
    d, od = P.MiRtj(), R.OracleDecoder()
    got = np.zeros(frame_bytes(w, h), np.uint8)
    want = got.copy()
    skips = 0
    for i in range(n):
        pkt = dev.d2h(d_st, int(pl[i]), offset=int(po[i]))
        ref = enc.encode(frames[i])
        assert pkt.size == ref.size and first_diff(pkt, ref) is None, i
        skips += int((pkt[12:] == 255).sum())
        d.decode(pkt, got)
        od.decode(ref, want)
        assert first_diff(got, want) is None, i
    assert skips > 0
    d.close()
    dev.free(d_fr)
    dev.free(d_st)


# --------------------------------------------------------------------------- benchmark sizes
@pytest.mark.parametrize("row", [0, 1, 2, 3])
def test_benchmark_size_digests_from_reference(dev, G, row):
    """Content, packet and planes regenerated entirely on the device must hash to what the
    reference's own encoder/decoder produced for the same seeded frame (tests/golden)."""
    w, h, Q, amp, n, plen = [int(x) for x in G["big_meta"][row]]
    dfr, dpkt, dpl = [str(x) for x in G["big_digests"][row]]
    d_fr = dev.synth(w, h, n, 1, seed=12345, amp=amp)
    d_st, po, pl = dev.encode(w, h, Q, 1, d_fr)
    dev.sync()
    assert R.digest(dev.d2h(d_fr, frame_bytes(w, h))) == dfr
    assert int(pl[0]) == plen
    pkt = dev.d2h(d_st, plen, offset=int(po[0]))
    assert R.digest(pkt) == dpkt
    d_out = dev.alloc(frame_bytes(w, h))
    plan = dev.plan(pkt[:12], po, pl, np.zeros(1, np.uint64))
    plan.decode(d_st, d_out)
    dev.sync()
    assert R.digest(dev.d2h(d_out, frame_bytes(w, h))) == dpl
    for p in (d_fr, d_st, d_out):
        dev.free(p)


def test_full_size_batch_properties(dev, monkeypatch):
    """256 distinct 1080p frames (BASELINE config), in the form the plan's policy chooses and with the split form
    forced: decode is deterministic (two passes give the same bytes, every picture), EVERY picture is the oracle's
    (each launch gives its pictures eight different XCD stripes: a sample would see half of them), and a sample of
    frames is independent of batch position (frame k decoded alone == inside the batch)."""
    w, h, Q, n = 1920, 1088, 255, 256
    fsz = frame_bytes(w, h)
    d_fr = dev.synth(w, h, 0, n, seed=12345, amp=8)
    d_st, po, pl = dev.encode(w, h, Q, n, d_fr)
    dev.free(d_fr)
    hdr = dev.d2h(d_st, 12, offset=int(po[0]))
    hdrs = np.tile(hdr, (n, 1))
    for i in range(n):  # only framesize differs between headers
        hdrs[i, 0:4] = np.frombuffer(np.uint32(pl[i]).tobytes(), np.uint8)
    oo = np.arange(n, dtype=np.uint64) * np.uint64(fsz)
    d_out = dev.alloc(fsz * n)
    host = dev.d2h(d_st, int(po[-1]) + int(pl[-1]))
    pkts = [host[int(po[k]):int(po[k]) + int(pl[k])] for k in range(n)]
    want = oracle_digests(pkts)
    assert len(want) == n
    sample = [0, 1, 127, 255]
    monkeypatch.delenv("MI_RTJ_ROTATE", raising=False)
    for form, split in (("policy", None), ("split", "1")):
        with monkeypatch.context() as m:
            m.delenv("MI_RTJ_SPLIT", raising=False)
            if split is not None:
                m.setenv("MI_RTJ_SPLIT", split)
            plan = dev.plan(hdrs, po, pl, oo)
        dev.memset(d_out, 0, fsz * n)
        plan.decode(d_st, d_out)
        dev.sync()
        first = {k: dev.d2h(d_out, fsz, offset=k * fsz) for k in sample}
        pass1 = device_digests(dev, d_out, fsz, n)
        dev.memset(d_out, 0, fsz * n)
        plan.decode(d_st, d_out)
        dev.sync()
        ran = plan.decode_form()[0]
        assert ran == 0 if split else ran in (0, 1), (form, plan.decode_form())
        pass2 = device_digests(dev, d_out, fsz, n)
        assert pass1 == pass2, (form, [k for k in range(n) if pass1[k] != pass2[k]][:8])
        for k in range(n):
            assert pass2[k] == want[k], explain_picture(dev, d_out, fsz, k, pkts[k], "1920x1088 x 256", form, n, ran == 0)
        for k in sample:
            again = dev.d2h(d_out, fsz, offset=k * fsz)
            assert first_diff(again, first[k]) is None
            wantk = np.zeros(fsz, np.uint8)
            R.OracleDecoder().decode(pkts[k], wantk)
            assert first_diff(again, wantk) is None, k
            alone = np.zeros(fsz, np.uint8)
            dd = P.MiRtj()
            dd.decode(pkts[k], alone)
            dd.close()
            assert first_diff(alone, wantk) is None, k
        plan.close()
    dev.free(d_st)
    dev.free(d_out)


def test_packed_passes_on_both_sides_of_their_16_bit_budget(dev):
    """k_decode runs the transform two int16 values to a register when every block of the wave satisfies
    sum g[r] g[c] |coefficient| <= budget (csrc/rtj_idct_pk.h; tests/test_bounds.py proves the bound), and one value to a
    register otherwise.  Blocks here are built from token values so that the kernel's own weighted sum lands well
    inside, just inside (the largest sum not above the budget that stepping one token reaches), just outside and well
    outside the budget, with sparse and dense coefficient patterns and both signs; most waves hold blocks of several
    kinds, some are all inside.  Chroma blocks get the same treatment with coefficients in the low 3x3 only (the
    three-input form has a packed twin with a budget of its own) and anywhere."""
    pkts, seen, _ = E.budget_packets(seed=2024)
    assert seen["in"] > 1000 and seen["out"] > 300 and seen["near"] > 300, seen
    outs = batch_decode(dev, pkts, prefill=0x55)
    dec = R.OracleDecoder()
    for i, (p, got) in enumerate(zip(pkts, outs)):
        w, h = int(p[6]) | (int(p[7]) << 8), int(p[8]) | (int(p[9]) << 8)
        want = np.full(frame_bytes(w, h), 0x55, np.uint8)
        dec.decode(p, want)
        assert first_diff(got, want) is None, (i, first_diff(got, want))
