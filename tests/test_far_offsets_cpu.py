"""The layout helper of the far-offset tests (tests/far_offsets.py) held to its own rules, for the size lists the GPU
tests use: every role is there in every variant, guards on both sides of every object, alias windows inside the buffer
and clear of every object and guard, and few enough window bytes that no test copies the gigabytes in between.  No GPU."""
import numpy as np
import pytest

import far_offsets as FO
import rtjfmt as F
import test_gpu_far_offsets as G
import test_gpu_parity as T


def size_lists():
    """(name, kind, sizes) of every list of objects tests/test_gpu_far_offsets.py lays out"""
    out = []
    for _, w, h in G.GEOMETRIES:
        pkts, _, _ = G.packets_and_wants(w, h)
        out.append((f"packets {w}x{h}", "packets", [p.size for p in pkts]))
        out.append((f"pictures {w}x{h}", "pictures", [T.frame_bytes(w, h)] * len(pkts)))
    pkts = G.repair_packets()[0]
    out.append(("repair packets", "packets", [p.size for p in pkts]))
    out.append(("repair pictures", "pictures", [T.frame_bytes(640, 368)] * len(pkts)))
    for fmt, w, h in G.RUN_CASES:
        out.append((f"run pictures format {fmt}", "pictures", [F.plane_bytes(fmt, w, h)] * 12))
        # an inter packet is between one byte per block and 64, behind its header
        out.append((f"run packets format {fmt}, shortest", "packets", [12 + F.nblocks(fmt, w, h)] * 12))
        out.append((f"run packets format {fmt}, longest", "packets", [12 + 64 * F.nblocks(fmt, w, h)] * 12))
    for fmt in G.ENC_FMTS:
        out.append((f"encoder chain pictures format {fmt}", "pictures", [F.plane_bytes(fmt, 176, 48)] * 6))
    return out


LISTS = size_lists()


@pytest.mark.parametrize("name,kind,sizes", LISTS, ids=[x[0] for x in LISTS])
def test_every_variant_of_every_list_obeys_the_rules(name, kind, sizes):
    seen = set()
    for variant in FO.variants(kind):
        lay = FO.layout(sizes, kind, variant)
        assert lay.total == FO.BUFFER_BYTES == (1 << 32) + (1 << 26)
        have = FO.check_layout(lay)
        assert have >= FO.required_roles(variant), (name, variant, have)
        seen |= have
    # over its variants a list has every placement for both lines, and a near object
    assert seen >= {"near"} | {(r, L) for L in FO.LINES for r in ("straddle", "at", "above")}


@pytest.mark.parametrize("name,kind,sizes", LISTS, ids=[x[0] for x in LISTS])
def test_near_and_alternating_layouts(name, kind, sizes):
    near = FO.near_layout(sizes, kind)
    assert FO.check_layout(near) == {"near"} and all(w is None for w in near.alias)
    alt = FO.alternating_layout(sizes, kind)
    FO.check_layout(alt)
    assert [int(o) > FO.WRAP for o in alt.offsets] == [bool(i & 1) for i in range(len(sizes))]
    assert all(b < FO.LINES[0] for (a, b), o in zip(alt.spans, alt.offsets) if int(o) < FO.WRAP)


def test_packet_variants_put_the_header_or_the_data_across_the_lines():
    sizes = [5000 + 37 * i for i in range(9)]
    for variant, part in (("header", "header"), ("data", "data")):
        lay = FO.layout(sizes, "packets", variant)
        for (role, L), (a, b) in zip(lay.roles, lay.spans):
            if role == "straddle":
                assert (a < L < a + 12) if part == "header" else (a + 12 <= L < b)
    at = FO.layout(sizes, "packets", "at")
    assert sorted(int(o) for o, (r, _) in zip(at.offsets, at.roles) if r == "at") == list(FO.LINES)


def test_alias_windows_are_where_a_narrowed_offset_lands():
    sizes = [353280] * 9
    for variant in FO.PICTURE_VARIANTS:
        lay = FO.layout(sizes, "pictures", variant)
        for (a, b), w in zip(lay.spans, lay.alias):
            if a >= FO.WRAP:
                assert w == (a & 0xFFFFFFFF, (a & 0xFFFFFFFF) + b - a)
            elif b > FO.WRAP:
                assert w == (0, b - FO.WRAP)  # where the sum of a 32-bit offset and a lane's share wraps to
            else:
                assert w is None


def test_a_broken_layout_is_caught():
    fsz = 4096
    with pytest.raises(AssertionError):  # two objects closer than their guards
        FO.check_layout(FO.Layout("pictures", "straddle", [fsz, fsz], [("near", 0), ("near", 0)], [1 << 30, (1 << 30) + fsz + 256]))
    with pytest.raises(AssertionError):  # an object in another's alias window
        FO.check_layout(FO.Layout("pictures", "at", [fsz, fsz], [("near", 0), ("at", FO.LINES[1])], [512, FO.LINES[1]]))
    with pytest.raises(AssertionError):  # past the buffer
        FO.check_layout(FO.Layout("pictures", "at", [fsz], [("above", FO.LINES[1])], [FO.BUFFER_BYTES - 16]))


def test_windows_cut_and_outside_objects():
    lay = FO.layout([1000 + 16 * i for i in range(7)], "pictures", "straddle")
    wins = [np.full(b - a, 7, np.uint8) for a, b in lay.windows]
    assert FO.outside_objects(lay, wins, 7) is None
    i = next(k for k, w in enumerate(lay.alias) if w)
    w = lay.alias[i]
    FO.cut(lay, wins, w)[3] = 9
    at, val, count, in_alias = FO.outside_objects(lay, wins, 7)
    assert (at, val, count, in_alias) == (w[0] + 3, 9, 1, True)
    assert "narrowed to 32 bits" in FO.alias_report(lay, wins, i, np.zeros(lay.sizes[i], np.uint8), 7)
    FO.cut(lay, wins, lay.spans[0])[:] = 1  # bytes of an object are the object's
    assert FO.outside_objects(lay, wins, 7)[0] == w[0] + 3
