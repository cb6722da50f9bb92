"""No-GPU checks of the 4:2:2 and greyscale decoders' checker and interface: the restatement of tests/rtjfmt.py equals
golden vectors made by the reference's own code, equals that code where it was built, the numpy colour helper equals
RTjpeg_yuv422rgb24, and the library exports the format entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import edge_packets as E
import rtjfmt as F
import rtjlib as R
from pkg import P, ROOT

SHAPES = [(F.FMT_422, 48, 24), (F.FMT_422, 176, 40), (F.FMT_GREY, 24, 8), (F.FMT_GREY, 136, 72)]
needs_ref = pytest.mark.skipif(not R.have_reference(), reason="reference build (oracle/_ref) not present")


def first_diff(a, b):
    d = np.nonzero(a != b)[0]
    return None if d.size == 0 else (int(d[0]), int(a[d[0]]), int(b[d[0]]), int(d.size))


def test_restatement_equals_the_golden():
    cases = F.golden_cases(F.load_golden())
    assert {(c[0], c[1], c[2]) for c in cases} == set(SHAPES)
    unchanged = 0
    for fmt, w, h, Q, key, pkts, outs in cases:
        dec = F.Restated(fmt)
        planes = np.full(F.plane_bytes(fmt, w, h), 77, np.uint8)
        for i, (pkt, want) in enumerate(zip(pkts, outs)):
            used, offs = dec.decode(pkt, planes)
            assert used == pkt.size, (fmt, w, h, Q, i, used, pkt.size)
            assert offs.size == F.nblocks(fmt, w, h) + 1 and offs[0] == 0 and offs[-1] == pkt.size - F.HEADER
            assert first_diff(planes, want) is None, (fmt, w, h, Q, i, first_diff(planes, want))
            unchanged += int(np.count_nonzero(np.diff(offs.astype(np.int64)) == 1))
    assert unchanged > 0  # the inter streams of the golden do have 0xFF blocks


@needs_ref
@pytest.mark.parametrize("fmt,w,h", SHAPES)
def test_restatement_equals_the_live_reference(fmt, w, h):
    pictures = 0
    for Q in (1, 128, 180, 230, 255):
        for amp in (0, 8, 64):
            for key in (0, 3):
                enc = F.RefFmt(fmt)
                enc.setup_encoder(w, h, Q, key, 2, 2)
                ref, dec = F.RefFmt(fmt), F.Restated(fmt)
                want = np.full(F.plane_bytes(fmt, w, h), 77, np.uint8)
                got = want.copy()
                pics = F.make_stream(fmt, w, h, 3, seed=Q + amp, amp=amp) if key else \
                    [F.make_picture(fmt, w, h, i, seed=Q + amp, amp=amp) for i in range(3)]
                for i, pic in enumerate(pics):
                    pkt = enc.encode(pic)
                    ref.decode(pkt, want)
                    used, _ = dec.decode(pkt, got)
                    assert used == pkt.size, (Q, amp, key, i)
                    assert first_diff(got, want) is None, (Q, amp, key, i, first_diff(got, want))
                    pictures += 1
    assert pictures == 90


@needs_ref
@pytest.mark.parametrize("fmt", (F.FMT_422, F.FMT_GREY))
def test_restatement_equals_the_live_reference_on_boundary_packets(fmt):
    """the packets tests/test_gpu_rtjfmt.py sends through the serial walker (64-byte blocks, 1-byte blocks, run tokens):
    what the device is compared with there is the reference's own picture here"""
    pkts = E.format_boundary_packets(fmt)
    assert len(pkts) == 6
    lens = []
    for i, pkt in enumerate(pkts):
        w, h, _ = F.header_of(pkt)
        want = np.full(F.plane_bytes(fmt, w, h), 0x4D, np.uint8)
        got = want.copy()
        F.RefFmt(fmt).decode(pkt, want)
        used, offs = F.Restated(fmt).decode(pkt, got)
        assert used == pkt.size and offs.size == F.nblocks(fmt, w, h) + 1 and offs[-1] == pkt.size - F.HEADER, i
        assert first_diff(got, want) is None, (i, first_diff(got, want))
        lens.append(np.diff(offs.astype(np.int64)))
    lens = np.concatenate(lens)
    assert lens.min() == 1 and lens.max() == 64  # the set holds the shortest and the longest block there is


@needs_ref
def test_numpy_colour_helper_equals_the_reference():
    for w, h, seed in ((48, 24, 1), (176, 40, 2)):
        planes = np.random.default_rng(seed).integers(0, 256, F.plane_bytes(F.FMT_422, w, h), dtype=np.uint8)
        pitch = 3 * w + 16
        want = np.full(h * pitch, 0x4D, np.uint8)
        got = want.copy()
        F.RefFmt(F.FMT_422).to_rgb24(w, h, planes, want, pitch)
        F.yuv422_to_rgb24(w, h, planes, got, pitch)
        assert first_diff(got, want) is None, (w, h, first_diff(got, want))
        assert np.all(got.reshape(h, pitch)[:, 3 * w:] == 0x4D)


def test_geometry_rule_of_the_restatement():
    assert F.Restated(F.FMT_422).decode(np.zeros(12, np.uint8), np.zeros(1, np.uint8)) is None
    assert F.geometry_ok(F.FMT_422, 48, 24) and not F.geometry_ok(F.FMT_420, 48, 24)
    assert not F.geometry_ok(F.FMT_422, 40, 24) and not F.geometry_ok(F.FMT_422, 48, 20)
    assert F.geometry_ok(F.FMT_GREY, 24, 8) and not F.geometry_ok(F.FMT_GREY, 24, 12)


def test_library_exports_the_format_entry_points():
    hdr = open(os.path.join(ROOT, "include", "mi_rtjpeg.h")).read()
    L = C.CDLL(P.lib_path())
    for name in ("mi_rtj_set_format", "mi_rtj_get_format", "mi_rtj_yuv422_to_rgb24"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(L, name), name
        assert name in P.binding.EXPORTS, name
    for name, value in (("MI_RTJ_FMT_YUV420", 0), ("MI_RTJ_FMT_YUV422", 1), ("MI_RTJ_FMT_GREY", 2)):
        assert re.search(name + r"\s*=\s*%d\b" % value, hdr), name
    assert (P.binding.FMT_YUV420, P.binding.FMT_YUV422, P.binding.FMT_GREY) == (0, 1, 2)
