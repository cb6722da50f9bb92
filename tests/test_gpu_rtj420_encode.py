"""The 4:2:0 arm of the encoder kernel (k_encode_fmt<4:2:0>, csrc/rtj_encode_kernels.h) at the smallest launch shapes at
which it can go wrong: packet bytes, pkt_len and pkt_offset byte for byte against the pinned oracle's encoder, inter
streams back through the decoder in order, and the format table's refusals against tests/golden/rtj_format_pins.json.
No tolerance anywhere.  Run on the GPU box with `pytest -m gpu`."""
import json
import os
import sys

import numpy as np
import pytest

import rtj420_enc as T
import rtjfmt as F
import rtjlib as R
from pkg import P, ROOT
from test_gpu_rtjfmt_encode import assert_stream_equals, device_packets, first_diff

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_rtj_format_pins as M  # noqa: E402

pytestmark = pytest.mark.gpu

FMT = F.FMT_420
INTRA_SHAPES = [
    (16, 16),   # one macroblock; 31 idle macroblock positions in every part
    (512, 16),  # exactly one full group
    (528, 16),  # a second group of one macroblock
    (176, 48),  # 33 macroblocks, 11 per row: groups wrap picture rows
    (48, 32),   # the smallest shape with two macroblock rows
]


@pytest.mark.parametrize("w,h", INTRA_SHAPES)
def test_intra_against_the_oracle(w, h):
    dev = P.MiRtj()
    for Q, align in ((1, 1), (128, 64), (255, 1)):
        pics = [F.make_picture(FMT, w, h, i, seed=Q + amp, amp=amp) for i, amp in enumerate((0, 8, 64))]
        want = T.oracle_packets(w, h, Q, pics)
        pkts, po, pl, _, stream = device_packets(dev, FMT, w, h, Q, pics, align=align)
        assert_stream_equals((w, h, Q), want, pkts, po, pl, align, stream)
        assert all(p[11] == 0 and p[10] == Q for p in pkts)
    dev.close()


@pytest.mark.parametrize("w,h", T.INTER_SHAPES)
def test_inter_streams_against_the_oracle_and_back_in_order(w, h):
    dev, back_dev = P.MiRtj(), P.MiRtj()
    # the device's packets go through the device's one-packet decoder and the oracle's, in order; both keep their picture
    # from stream to stream (at quality 1 with masks of 2 even a stream's first packet is unchanged blocks alone)
    dec, back = R.OracleDecoder(), np.zeros(F.plane_bytes(FMT, w, h), np.uint8)
    for key, Q in T.INTER_SETTINGS:
        for lmask, cmask in T.MASKS:
            what = (w, h, key, Q, lmask, cmask)
            align = 64 if key == 3 else 1
            pics = T.inter_pictures(w, h, seed=key + lmask)
            want = T.oracle_packets(w, h, Q, pics, key, lmask, cmask)
            pkts, po, pl, _, stream = device_packets(dev, FMT, w, h, Q, pics, align=align, key=key, lmask=lmask, cmask=cmask)
            assert_stream_equals(what, want, pkts, po, pl, align, stream)
            T.assert_skip_rule(what, pkts, key, Q, lmask, cmask)
            for i, p in enumerate(pkts):
                dec.decode(p, back)
                got = np.zeros_like(back)
                back_dev.decode(p, got)
                assert first_diff(got, back) is None, (what, i, first_diff(got, back))
    dev.close()
    back_dev.close()


def test_257_pictures_cross_the_pass_boundary():
    """an intra call takes 256 pictures per pass: picture 256 is the second pass's only one"""
    w, h, Q, n = 16, 16, 200, 257
    pics = [F.make_picture(FMT, w, h, i, seed=3, amp=(0, 8, 64)[i % 3]) for i in range(n)]
    dev = P.MiRtj()
    pkts, po, pl, _, stream = device_packets(dev, FMT, w, h, Q, pics, align=64)
    assert_stream_equals("257", T.oracle_packets(w, h, Q, pics), pkts, po, pl, 64, stream)
    assert len({p.tobytes() for p in pkts[250:]}) > 1
    dev.close()


# ---- the table's answers where the per-call-site arithmetic and texts used to be ----
def test_refusals_and_their_texts_are_the_pinned_ones():
    with open(M.PINS) as f:
        want = json.load(f)["refusals"]
    got = M.refusals()  # (made once per process)
    assert len(want) == len(got) == len(M.FMTS) * len(M.SIZES) ** 2
    for a, b in zip(want, got):
        assert a == b, (a, b)
    refused = [r for r in want if r[3][0] != 0]
    assert len(refused) > len(want) // 2 and all(r[3][1] and r[4][1] for r in refused)


def test_the_maker_reproduces_the_committed_pins_byte_for_byte():
    with open(M.PINS) as f:
        assert M.text({"bound": M.bounds(), "refusals": M.refusals()}) == f.read()
