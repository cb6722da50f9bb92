"""Pictures built around DC-only blocks ("DC, zeros, one run": the pixel clamp((int16(DC * q0) + 4) >> 3) 64 times
over, lib/RTjpeg.c:2223-2238), which is what five of six chroma blocks of the bench content are: flat chroma under busy
luma, half-flat pictures (macroblock groups that mix DC-only and busy blocks), all-flat pictures, unchanged (0xFF)
blocks among them, and DC-only blocks spelled in ways the encoder never uses.  Every case runs through the three forms
of a batch launch, each forced by the environment and checked against what the plan says ran: a wave per part of a
group (k_decode<false, false>, MI_RTJ_ROTATE=0), the split form (k_decode_split: luma waves, chroma waves that pool the
busy blocks of three groups, and k_decode_list for what they decline; MI_RTJ_ROTATE=1 MI_RTJ_SPLIT=1) and the classic
form (k_decode<true, false>: a wave takes all three parts of its groups; MI_RTJ_ROTATE=1 MI_RTJ_SPLIT=0).  Bit-exact
against the oracle everywhere."""
import numpy as np
import pytest

import edge_packets as E
import rtjlib as R
import test_gpu_parity as T
from pkg import P

pytestmark = pytest.mark.gpu


# form -> (environment of the plan, what plan.decode_form() says ran)
FORMS = {
    "part-per-wave": (dict(MI_RTJ_ROTATE="0"), -1),
    "split": (dict(MI_RTJ_ROTATE="1", MI_RTJ_SPLIT="1"), 0),
    "classic": (dict(MI_RTJ_ROTATE="1", MI_RTJ_SPLIT="0"), 1),
}


@pytest.fixture(params=list(FORMS))
def dev(request, monkeypatch):
    env, form = FORMS[request.param]
    for k in ("MI_RTJ_ROTATE", "MI_RTJ_SPLIT", "MI_RTJ_DEC_SLOTS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = P.MiRtj()
    d.expect_form = form
    yield d
    d.close()


def decode_batch(dev, pkts, prefill=0):
    """batch decode through one plan, launched twice over the same buffers; returns the planes per packet."""
    d_stream, po, pl, hdrs = dev.upload_packets(pkts, align=1)
    sizes = [T.frame_bytes(int(p[6]) | (int(p[7]) << 8), int(p[8]) | (int(p[9]) << 8)) for p in pkts]
    oo = (np.cumsum([0] + [(s + 255) // 256 * 256 for s in sizes])).astype(np.uint64)
    d_out = dev.alloc(int(oo[-1]))
    dev.memset(d_out, prefill, int(oo[-1]))
    plan = dev.plan(hdrs, po, pl, oo[:-1].copy())
    plan.decode(d_stream, d_out)
    plan.decode(d_stream, d_out)
    dev.sync()
    assert plan.decode_form()[0] == dev.expect_form, (plan.decode_form(), dev.expect_form)
    outs = [dev.d2h(d_out, sizes[i], offset=int(oo[i])) for i in range(len(pkts))]
    plan.close()
    dev.free(d_stream)
    dev.free(d_out)
    return outs


def check(pkts, outs, prefill=0):
    for i, (p, got) in enumerate(zip(pkts, outs)):
        w, h = int(p[6]) | (int(p[7]) << 8), int(p[8]) | (int(p[9]) << 8)
        want = np.full(T.frame_bytes(w, h), prefill, np.uint8)
        R.OracleDecoder().decode(p, want)
        assert T.first_diff(got, want) is None, (i, T.first_diff(got, want))


def test_bench_content_flat_chroma_under_busy_luma(dev):
    """Q=255, noise +-8 on luma and +-4 on chroma: five of six chroma blocks are DC only."""
    w, h = 1920, 1088
    pkts = [R.OracleEncoder(w, h, 255).encode(R.synth_frame(w, h, i, amp=8)) for i in range(2)]
    check(pkts, decode_batch(dev, pkts))


def half_flat(w, h, n, seed):
    """left half flat (every block DC only), right half noisy: luma groups mix both kinds."""
    f = R.synth_frame(w, h, n, seed=seed, amp=40)
    y, u, v = R.split_planes(f, w, h)
    y = y.reshape(h, w).copy()
    u = u.reshape(h // 2, w // 2).copy()
    v = v.reshape(h // 2, w // 2).copy()
    y[:, : w // 2] = 77
    u[:, : w // 4] = 90
    v[:, : w // 4] = 200
    return np.concatenate([y.ravel(), u.ravel(), v.ravel()])


@pytest.mark.parametrize("Q", [255, 200, 128, 30])
def test_half_flat_pictures(dev, Q):
    w, h = 640, 368
    pkts = [R.OracleEncoder(w, h, Q).encode(half_flat(w, h, i, 3)) for i in range(3)]
    check(pkts, decode_batch(dev, pkts, prefill=0x33), prefill=0x33)


def test_flat_pictures(dev):
    w, h = 320, 240
    flat = np.concatenate([np.full(w * h, 120, np.uint8), np.full(w * h // 4, 60, np.uint8),
                           np.full(w * h // 4, 190, np.uint8)])
    pkts = [R.OracleEncoder(w, h, Q).encode(flat) for Q in (255, 128, 5)]
    check(pkts, decode_batch(dev, pkts, prefill=1), prefill=1)


def test_unchanged_blocks_among_dc_only_ones(dev):
    """inter stream over a half-flat picture: 0xFF blocks keep what the buffer held (prefill)."""
    w, h, Q = 640, 368, 220
    enc = R.OracleEncoder(w, h, Q, key_rate=8, lmask=2, cmask=2)
    pkts = [enc.encode(half_flat(w, h, n // 3, 5)) for n in range(6)]
    assert any((p[12:] == 255).any() for p in pkts)
    check(pkts, decode_batch(dev, pkts, prefill=0x5A), prefill=0x5A)


def test_dc_only_blocks_spelled_unusually(dev):
    """DC followed by zero coefficients written out, by several short runs, by a run that overshoots, or with a
    non-zero raw byte: none is the encoder's "DC, zeros, one run" form; mixed with blocks that are."""
    pkts = E.dc_spelling_packets(seed=12, w=512, h=64)
    check(pkts, decode_batch(dev, pkts, prefill=9), prefill=9)
