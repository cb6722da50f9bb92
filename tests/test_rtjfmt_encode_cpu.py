"""No-GPU checks of the 4:2:2 and greyscale encoders' checker and interface: the restatement of tests/rtjfmt_enc.py
equals the golden 4:2:2 packets the reference made, equals the reference's own encoder where it was built (4:2:2 directly;
greyscale through a buffer in which the reference reads the picture's own blocks, where one exists), the bound and the
binding's `fmt` argument."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rtjfmt as F
import rtjfmt_enc as E
import rtjlib as R
from pkg import P, ROOT

B = P.binding
needs_ref = pytest.mark.skipif(not R.have_reference(), reason="reference build (oracle/_ref) not present")
SHAPES_422 = [(16, 8), (48, 24), (176, 40), (528, 8)]


def same(a, b):
    return a.size == b.size and np.array_equal(a, b)


def assert_not_vacuous(fmt, pkts, what, Q, lmask=2, cmask=2):
    """every inter packet after the first holds at least one unchanged and at least one coded block — except at quality 1
    with masks of 2 (rtjfmt_enc.all_blocks_forced_unchanged), where no coefficient leaves the mask of the cleared store:
    there every block of every packet, the first included, has to be unchanged"""
    if E.all_blocks_forced_unchanged(Q, lmask, cmask):
        assert all(E.block_kinds(fmt, p)[1] == 0 for p in pkts), what
        return
    for i, p in enumerate(pkts[1:], 1):
        unchanged, coded = E.block_kinds(fmt, p)
        assert unchanged > 0 and coded > 0, (what, i, unchanged, coded)


# ---- the restatement's own plumbing ----
def test_arrangement_is_repack_read_backwards():
    """a picture whose every block is filled with its stream-order number: the 4:2:0 picture's luma blocks 0, 1, 2, ...
    and chroma blocks hold the numbers repack() picks them up in"""
    for fmt, w, h in ((F.FMT_422, 48, 24), (F.FMT_422, 176, 40), (F.FMT_GREY, 24, 8), (F.FMT_GREY, 136, 72)):
        pic = np.zeros(F.plane_bytes(fmt, w, h), np.uint8)
        y, cb, cr = F.split(fmt, pic, w, h)
        y = y.reshape(h, w)
        if fmt == F.FMT_422:
            cb, cr = cb.reshape(h, w // 2), cr.reshape(h, w // 2)
            for m in range((w // 16) * (h // 8)):
                i, j = divmod(m, w // 16)
                y[8 * i:8 * i + 8, 16 * j:16 * j + 8] = (4 * m + 1) % 251
                y[8 * i:8 * i + 8, 16 * j + 8:16 * j + 16] = (4 * m + 2) % 251
                cb[8 * i:8 * i + 8, 8 * j:8 * j + 8] = (4 * m + 3) % 251
                cr[8 * i:8 * i + 8, 8 * j:8 * j + 8] = (4 * m + 4) % 251
        else:
            for b in range((w // 8) * (h // 8)):
                i, j = divmod(b, w // 8)
                y[8 * i:8 * i + 8, 8 * j:8 * j + 8] = (b + 1) % 251
        W, H = F.source_size(fmt, w, h)
        a = E.arrange(fmt, w, h, pic)
        Y, U, V = R.split_planes(a, W, H)
        Y, U, V = Y.reshape(H, W), U.reshape(H // 2, W // 2), V.reshape(H // 2, W // 2)
        luma = []
        chroma = []
        for mb in range((W // 16) * (H // 16)):
            my, mx = divmod(mb, W // 16)
            for q in range(4):
                blk = Y[16 * my + 8 * (q >> 1):16 * my + 8 * (q >> 1) + 8, 16 * mx + 8 * (q & 1):16 * mx + 8 * (q & 1) + 8]
                assert np.all(blk == blk[0, 0])
                luma.append(int(blk[0, 0]))
            chroma += [int(U[8 * my, 8 * mx]), int(V[8 * my, 8 * mx])]
        if fmt == F.FMT_422:
            seq = []
            for m in range((w // 16) * (h // 8)):
                seq += [luma[2 * m], luma[2 * m + 1], chroma[2 * m], chroma[2 * m + 1]]
            assert seq == [(k + 1) % 251 for k in range(F.nblocks(fmt, w, h))]
            assert not any(luma[2 * (w // 16) * (h // 8):])
        else:
            n = F.nblocks(fmt, w, h)
            assert luma[:n] == [(b + 1) % 251 for b in range(n)] and not any(luma[n:]) and not any(chroma)


# ---- golden: always runs ----
def test_restatement_equals_the_golden_422_packets():
    cases = E.golden_422()
    assert sum(len(c[6]) for c in cases) == 8
    for ci, w, h, Q, key, pics, want in cases:
        got = E.encode_all(F.FMT_422, w, h, Q, pics, key, 2, 2)
        for i, (g, wnt) in enumerate(zip(got, want)):
            assert same(g, wnt), (ci, w, h, Q, key, i)
        if key:
            assert_not_vacuous(F.FMT_422, got, ("golden", ci), Q)


# ---- the reference's own encoder, where it was built ----
@needs_ref
@pytest.mark.parametrize("w,h", SHAPES_422)
def test_422_equals_the_live_reference(w, h):
    packets = 0
    for Q in (1, 64, 128, 230, 255):
        for amp in (0, 8, 64):
            for key in (0, 3):
                ref = F.RefFmt(F.FMT_422)
                ref.setup_encoder(w, h, Q, key, 2, 2)
                pics = E.make_stream(F.FMT_422, w, h, 3, seed=Q + amp, amp=amp) if key else \
                    [F.make_picture(F.FMT_422, w, h, i, seed=Q + amp, amp=amp) for i in range(3)]
                got = E.encode_all(F.FMT_422, w, h, Q, pics, key, 2, 2)
                for i, pic in enumerate(pics):
                    assert same(got[i], ref.encode(pic)), (Q, amp, key, i)
                    packets += 1
                if key:
                    assert_not_vacuous(F.FMT_422, got, (w, h, Q, amp), Q)
    assert packets == 90  # 360 over the four shapes


# twelve pictures of the five extreme kinds, neighbours often equal: longer than every key period below
EXTREME_STREAM = ("zeros", "zeros", "full", "stripes", "stripes", "binary", "uniform", "uniform", "zeros", "full", "full",
                  "binary")


@needs_ref
@pytest.mark.parametrize("w,h", SHAPES_422)
def test_422_extreme_pictures_equal_the_live_reference(w, h):
    packets = 0
    pics = [E.extreme_picture(F.FMT_422, w, h, kind) for kind in EXTREME_STREAM]
    for key in (0, 1, 2, 3):
        for lmask, cmask in ((0, 0), (16, 16), (2, 5)):
            ref = F.RefFmt(F.FMT_422)
            ref.setup_encoder(w, h, 255 if key % 2 else 128, key, lmask, cmask)
            got = E.encode_all(F.FMT_422, w, h, 255 if key % 2 else 128, pics, key, lmask, cmask)
            for i, pic in enumerate(pics):
                assert same(got[i], ref.encode(pic)), (key, lmask, cmask, i, EXTREME_STREAM[i])
                packets += 1
            if key:  # a repeated picture is all 0xFF blocks unless its packet is a key frame
                assert any(E.block_kinds(F.FMT_422, p)[1] == 0 for p in got[1:]), (key, lmask, cmask)
    assert packets == 144  # 576 over the four shapes


@needs_ref
@pytest.mark.parametrize("w,h", [(8, 8), (24, 8), (40, 32), (136, 64)])
def test_grey_intra_equals_the_live_reference_on_its_own_lines(w, h):
    packets = 0
    for Q in (1, 128, 255):
        for amp in (0, 8, 64):
            pic = F.make_picture(F.FMT_GREY, w, h, 0, seed=Q + amp, amp=amp)
            ref = F.RefFmt(F.FMT_GREY)
            ref.setup_encoder(w, h, Q)
            want = ref.encode(E.ref_grey_planes(pic, w, h, inter=False))
            assert same(E.encode_all(F.FMT_GREY, w, h, Q, [pic])[0], want), (Q, amp)
            packets += 1
    assert packets == 9  # 36 over the four shapes


def grey_line_stream(w, seed):
    """five 8-line pictures: odd ones repeat their predecessor (every block unchanged), even ones renew the left third of
    the blocks (at 8x8, the one block) — a picture of 8 lines has no block that make_stream's new top third leaves alone"""
    pics = [F.make_picture(F.FMT_GREY, w, 8, 0, seed, 8)]
    for i in range(1, 5):
        p = pics[-1].copy()
        if i % 2 == 0:
            cols = 8 * ((w // 8 + 2) // 3)
            p.reshape(8, w)[:, :cols] = F.make_picture(F.FMT_GREY, w, 8, 5 * i, seed, 64).reshape(8, w)[:, :cols]
        pics.append(p)
    return pics


@needs_ref
@pytest.mark.parametrize("w", (8, 24, 136))
def test_grey_inter_equals_the_live_reference_on_its_own_lines(w):
    packets = 0
    for Q in (128, 255):
        pics = grey_line_stream(w, seed=Q)
        ref = F.RefFmt(F.FMT_GREY)
        ref.setup_encoder(w, 8, Q, 3, 2, 2)
        got = E.encode_all(F.FMT_GREY, w, 8, Q, pics, 3, 2, 2)
        kinds = []
        for i, pic in enumerate(pics):
            assert same(got[i], ref.encode(E.ref_grey_planes(pic, w, 8, inter=True))), (Q, i)
            kinds.append(E.block_kinds(F.FMT_GREY, got[i]))
            packets += 1
        assert kinds[1][1] == 0 and kinds[3][1] == 0 and kinds[2][1] > 0  # repeated: all unchanged; renewed: some coded
        assert w == 8 or kinds[2][0] > 0  # ... and the blocks right of the renewed third stay
        assert got[4][11] == 0 and kinds[4][0] == 0  # packet 4 is a key frame again: the store was cleared, all coded
    assert packets == 10  # 30 over the three widths


def test_no_buffer_for_the_reference_above_its_one_to_one_range():
    pic = np.zeros(136 * 72, np.uint8)
    assert E.ref_grey_planes(pic, 136, 72, inter=False) is None
    assert E.ref_grey_planes(pic[:136 * 16], 136, 16, inter=True) is None


# ---- interface ----
def test_library_exports_the_encode_entry_points():
    hdr = open(os.path.join(ROOT, "include", "mi_rtjpeg.h")).read()
    L = C.CDLL(P.lib_path())
    for name in ("mi_rtj_encode_bound_fmt", "mi_rtj_encode_frames_fmt", "mi_rtj_encode_stream_fmt"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(L, name), name
        assert name in B.EXPORTS, name


def test_bound_per_format():
    L = B.load()
    for w, h, n, align in ((16, 16, 1, 1), (48, 32, 3, 64), (1920, 1088, 1024, 64), (176, 48, 257, 4096)):
        up = lambda x: (x + align - 1) // align * align
        assert L.mi_rtj_encode_bound_fmt(B.FMT_YUV420, w, h, n, align) == L.mi_rtj_encode_bound(w, h, n, align) > 0
        assert L.mi_rtj_encode_bound_fmt(B.FMT_YUV422, w, h, n, align) == n * up(12 + 64 * (4 * w * h // 128)) + align
        assert L.mi_rtj_encode_bound_fmt(B.FMT_GREY, w, h, n, align) == n * up(12 + 64 * (w * h // 64)) + align
    # sizes that are legal in one format only
    assert L.mi_rtj_encode_bound_fmt(B.FMT_YUV422, 16, 8, 1, 1) == 12 + 4 * 64 + 1
    assert L.mi_rtj_encode_bound_fmt(B.FMT_GREY, 8, 8, 2, 16) == 2 * 80 + 16
    for fmt in (B.FMT_YUV420, B.FMT_YUV422, B.FMT_GREY):
        for bad in ((0, 8, 1, 1), (16, 0, 1, 1), (16, 8, 0, 1), (16, 8, 1, 0)):
            assert L.mi_rtj_encode_bound_fmt(fmt, *bad) == 0
    assert L.mi_rtj_encode_bound_fmt(3, 16, 16, 1, 1) == 0 and L.mi_rtj_encode_bound_fmt(-1, 16, 16, 1, 1) == 0


class FakeLib:
    """records what MiRtj.encode / encode_bound hand to the library"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 4096 if "bound" in name else 0
        return call


def test_binding_forwards_the_format():
    dev = B.MiRtj.__new__(B.MiRtj)  # no device: the instance's library is the recorder
    dev.L, dev.h = FakeLib(), None
    assert dev.encode_bound(48, 24, 2, 64) == 4096 and dev.encode_bound(48, 24, 2, 64, fmt=B.FMT_YUV422) == 4096
    assert dev.L.calls == [("mi_rtj_encode_bound", (48, 24, 2, 64)), ("mi_rtj_encode_bound_fmt", (1, 48, 24, 2, 64))]
    for fmt, key, want in ((None, 0, "mi_rtj_encode_frames"), (None, 3, "mi_rtj_encode_stream"),
                           (B.FMT_YUV420, 0, "mi_rtj_encode_frames"), (B.FMT_YUV422, 0, "mi_rtj_encode_frames_fmt"),
                           (B.FMT_GREY, 3, "mi_rtj_encode_stream_fmt")):
        dev.L.calls.clear()
        kw = {} if fmt is None else {"fmt": fmt}
        d_stream, po, pl = dev.encode(48, 24, 200, 2, 1234, align=16, key_rate=key, lmask=2, cmask=5, d_stream=5678, **kw)
        assert d_stream == 5678 and po.size == 2 and pl.size == 2
        name, args = dev.L.calls[-1]
        assert name == want
        if want.endswith("_fmt"):
            assert len(dev.L.calls) == 1  # (a caller's buffer: no bound is asked for)
            assert args[:5] == (None, fmt, 48, 24, 200)
            assert args[5:-2] == ((3, 2, 5) if key else ()) + (2, 1234, 5678, 16)
        else:
            assert dev.L.calls[0] == ("mi_rtj_encode_bound", (48, 24, 2, 16)) and len(dev.L.calls) == 2
            assert args[:4] == (None, 48, 24, 200)
            assert args[4:-2] == ((3, 2, 5) if key else ()) + (2, 1234, 5678, 16)
    dev.L = None  # (nothing to destroy: __del__ sees h is None)
