"""Runs on 4:2:2 and greyscale plans, without a GPU: mi_rtj_plan_set_runs_fmt is exported, the block rectangles of
tests/runlib_fmt.py tile the planes, the run rule the device implements equals the in-order decode of the restatement
(tests/rtjfmt.py), and that in-order decode equals the golden planes made by the reference and, where oracle/_ref was
built, the reference's own decoder on the streams tests/test_gpu_fmt_runs.py uses.  Bit for bit, no tolerance."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rtjfmt as F
import rtjlib as R
import runlib_fmt as RF
from pkg import P, ROOT

SHAPES = [(F.FMT_422, 48, 24), (F.FMT_422, 176, 40), (F.FMT_GREY, 24, 8), (F.FMT_GREY, 136, 72)]
QK = [(200, 4), (90, 1), (255, 255)]  # (quality, key_rate) of the encoder-made streams, masks 2 / 2
needs_ref = pytest.mark.skipif(not R.have_reference(), reason="reference build (oracle/_ref) not present")


def stream(fmt, w, h, Q, kr):
    return F.make_packets(fmt, w, h, Q, 9, seed=3, key_rate=kr, lmask=2, cmask=2)


def same(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), (what, i)


def test_set_runs_fmt_is_exported_and_declared():
    L = C.CDLL(P.binding.lib_path())
    hdr = open(os.path.join(ROOT, "include", "mi_rtjpeg.h")).read()
    assert hasattr(L, "mi_rtj_plan_set_runs_fmt")
    assert re.search(r"\bmi_rtj_plan_set_runs_fmt\s*\(", hdr)
    assert "mi_rtj_plan_set_runs_fmt" in P.binding.EXPORTS
    assert hasattr(P.binding.Plan, "set_runs_fmt")


def test_set_runs_fmt_refuses_a_missing_plan():
    L = P.binding.load()
    lens = (C.c_int * 1)(1)
    assert L.mi_rtj_plan_set_runs_fmt(None, 1, lens) == -3


@pytest.mark.parametrize("fmt,w,h", SHAPES)
def test_block_rectangles_tile_every_plane_once(fmt, w, h):
    plane, y0, x0 = RF.block_rects(fmt, w, h)
    assert plane.size == F.nblocks(fmt, w, h)
    pic = np.zeros(F.plane_bytes(fmt, w, h), np.uint16)
    views = RF.plane_views(fmt, pic, w, h)
    for b in range(plane.size):
        views[plane[b]][y0[b]:y0[b] + 8, x0[b]:x0[b] + 8] += 1
    assert np.all(pic == 1)
    if fmt == F.FMT_422:
        # macroblock 1 of the second macroblock row: Y right is rows 8..15, columns 24..31; Cr rows 8..15, columns 8..15
        b = 4 * (w // 16 + 1)
        assert (plane[b + 1], y0[b + 1], x0[b + 1]) == (0, 8, 24) and (plane[b + 3], y0[b + 3], x0[b + 3]) == (2, 8, 8)
    elif h > 8:
        b = w // 8 + 2  # third block of the second block row
        assert (plane[b], y0[b], x0[b]) == (0, 8, 16)


@pytest.mark.parametrize("fmt,w,h", SHAPES)
@pytest.mark.parametrize("Q,kr", QK)
def test_rule_equals_in_order_decode_on_encoder_streams(fmt, w, h, Q, kr):
    pkts = stream(fmt, w, h, Q, kr)
    assert RF.has_both_kinds(fmt, pkts, [9])
    for runs in ([9], [1, 8], [4, 1, 4], [1] * 9):
        prev = [RF.rand_pic(fmt, w, h, r) for r in range(len(runs))]
        want = RF.in_order(fmt, pkts, runs, prev)
        got, copied = RF.by_rule(fmt, pkts, runs, prev)
        same(got, want, (runs,))
        unchanged = 0
        i = 0
        for n in runs:
            unchanged += sum(int((~RF.coded_blocks(fmt, p)).sum()) for p in pkts[i + 1:i + n])
            i += n
        assert copied == unchanged


@pytest.mark.parametrize("fmt,w,h", [(F.FMT_422, 48, 24), (F.FMT_GREY, 24, 8), (F.FMT_GREY, 136, 72)])
@pytest.mark.parametrize("n", [2, 65, 129])
def test_rule_equals_in_order_decode_on_crafted_packets(fmt, w, h, n):
    pkts = RF.crafted_run(fmt, n, w, h, seed=n)
    assert RF.has_both_kinds(fmt, pkts, [n])
    prev = [RF.rand_pic(fmt, w, h, n)]
    got, copied = RF.by_rule(fmt, pkts, [n], prev)
    same(got, RF.in_order(fmt, pkts, [n], prev), n)
    assert copied > 0


def test_in_order_decode_equals_the_golden_key_rate_cases():
    cases = [c for c in F.golden_cases(F.load_golden()) if c[4] > 0]
    assert {(c[0], c[1], c[2]) for c in cases} == {(F.FMT_422, 48, 24), (F.FMT_422, 176, 40), (F.FMT_GREY, 136, 72)}
    for fmt, w, h, Q, key, pkts, outs in cases:
        n = len(pkts)
        assert RF.has_both_kinds(fmt, pkts, [n])
        prev = [np.full(F.plane_bytes(fmt, w, h), 77, np.uint8)]
        same(RF.in_order(fmt, pkts, [n], prev), outs, (fmt, w, h))
        got, copied = RF.by_rule(fmt, pkts, [n], prev)
        same(got, outs, ("rule", fmt, w, h))
        assert copied > 0


def test_unchanged_counts_of_the_streams():
    """what the generator and the golden were seen to hold: second packets' unchanged blocks"""
    for (fmt, w, h), (unch, total) in zip(SHAPES, [(20, 36), (120, 220), (1, 3), (63, 153)]):
        c = RF.coded_blocks(fmt, stream(fmt, w, h, 200, 4)[1])
        assert (int((~c).sum()), c.size) == (unch, total), (fmt, w, h)
    got = {}
    for fmt, w, h, Q, key, pkts, outs in F.golden_cases(F.load_golden()):
        if key > 0:
            c = RF.coded_blocks(fmt, pkts[1])
            got[(fmt, w, h)] = (int((~c).sum()), c.size)
    # (the greyscale case: 36 unchanged, 117 coded)
    assert got == {(F.FMT_422, 48, 24): (24, 36), (F.FMT_422, 176, 40): (142, 220), (F.FMT_GREY, 136, 72): (36, 153)}


@needs_ref
@pytest.mark.parametrize("fmt,w,h", SHAPES)
def test_in_order_decode_equals_the_live_reference(fmt, w, h):
    for Q, kr in QK:
        pkts = stream(fmt, w, h, Q, kr)
        prev = [RF.rand_pic(fmt, w, h, Q)]
        same(RF.in_order(fmt, pkts, [9], prev), RF.in_order(fmt, pkts, [9], prev, make=F.RefFmt), (Q, kr))
    n = 65
    pkts = RF.crafted_run(fmt, n, w, h, seed=n)
    prev = [RF.rand_pic(fmt, w, h, n)]
    same(RF.in_order(fmt, pkts, [n], prev), RF.in_order(fmt, pkts, [n], prev, make=F.RefFmt), "crafted")


@pytest.mark.parametrize("fmt,w,h", [(F.FMT_422, 176, 40), (F.FMT_GREY, 136, 72)])
def test_the_bench_tools_in_order_decode_is_the_restatements(fmt, w, h):
    """tools/bench_format_runs.py checks its pictures with a loop that steps over stretches of 0xFF at once"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_format_runs", os.path.join(ROOT, "tools", "bench_format_runs.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    pkts = stream(fmt, w, h, 200, 4) + RF.crafted_run(fmt, 5, w, h, Q=60, seed=1)
    prev = RF.rand_pic(fmt, w, h, 4)
    want = RF.in_order(fmt, pkts, [len(pkts)], [prev])[-1]
    assert np.array_equal(tool.decode_in_order(fmt, pkts, prev.copy()), want)
    for f in (0, 1, 2):  # the scene in the three plane layouts
        pics = list(tool.content(f, 1920, 1088, 2))
        assert [p.size for p in pics] == [F.plane_bytes(f, 1920, 1088)] * 2 and not np.array_equal(pics[0], pics[1])
