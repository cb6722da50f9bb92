"""No-GPU checks of libmi_tga.so (include/mi_tga.h): the statement itself (tests/tgaraw.py: its loop-for-loop form against its
vectorised form over every type x depth x orientation x map depth and over the bad streams; both against the seven vectors
recorded from upstream's lib/targa.c), the host-only calls (mi_tga_parse against parse() field for field over every header
case, every refusal in upstream's order and every truncation; mi_tga_tile_pixels), the exported symbols, the signature table
and the info struct against the header."""
import ctypes as C
import importlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import tgaraw as T
from pkg import ROOT
from test_ctypes_signatures_cpu import ctypes_kind, prototypes

tga = importlib.import_module("gmerlin-avdecoder_amd.tga")

ORIENTATIONS = (0x00, 0x10, 0x20, 0x30)
# (image type, pixel depth, map depth or 0)
KINDS = [(t, d, 0) for t in (2, 3, 10, 11) for d in (8, 16, 24, 32)] + [(t, 8, m) for t in (1, 9) for m in (16, 24, 32)]
VECTORS = json.load(open(os.path.join(ROOT, "tests", "golden", "tga_vectors.json")))["vectors"]


def both(packet, palette=None, expect=None):
    a, b = T.decode(packet, palette, expect), T.decode_fast(packet, palette, expect)
    assert a[0] == b[0] and a[2] == b[2], (a[0], b[0])
    assert (a[1] is None) == (b[1] is None) == (a[0] != 0)
    if a[1] is not None:
        assert np.array_equal(a[1], b[1])
    return a


@pytest.mark.parametrize("image_type,depth,map_depth", KINDS, ids=[f"type{t}-{d}-map{m}" for t, d, m in KINDS])
def test_the_two_forms_of_the_statement_agree(image_type, depth, map_depth):
    rng = np.random.default_rng(1000 * image_type + 10 * depth + map_depth)
    for descriptor in ORIENTATIONS:
        for w, h in ((1, 1), (5, 3), (67, 2), (131, 5)):
            for origin in ((0, 3) if map_depth else (0,)):
                p = T.random_packet(rng, image_type, w, h, depth, descriptor, map_depth=map_depth or 24, map_origin=origin, ident=b"id!")
                st, pic, info = both(p)
                want = map_depth or depth
                assert st == 0 and pic.size == w * h * want // 8 == T.layout(info.format, w, h).picture_bytes
                assert (info.flip_x, info.flip_y) == (descriptor >> 4 & 1, 1 - (descriptor >> 5 & 1))
                assert both(p, None, (w, h, T.FORMATS[want // 8 - 1]))[0] == 0
                assert both(p, None, (w + 1, h, T.FORMATS[want // 8 - 1]))[0] == T.MISMATCH
                assert both(p, None, (w, h, T.FORMATS[(want // 8) % 4]))[0] == T.MISMATCH
    if map_depth == 32:  # the caller's palette
        pal = T.random_palette(rng, 7)
        p = T.random_packet(rng, image_type, 9, 4, 8, 0x20, from_palette=7)
        st, pic, info = both(p, pal)
        assert st == 0 and info.from_palette and (info.map_origin, info.map_length, info.map_depth) == (0, 7, 32)
        assert both(p, None)[0] == T.CMAP_MISSING


def test_orientation_and_last_pixel_rule_on_hand_written_pixels():
    px = np.arange(1, 25, dtype=np.uint8)  # 3 x 2 at 32 bits, stored order
    swapped = px.reshape(6, 4).copy()
    swapped[:5, [0, 2]] = swapped[:5, [2, 0]]
    for descriptor in ORIENTATIONS:
        st, pic, _ = both(T.packet(2, 3, 2, 32, px.tobytes(), descriptor))
        rows = swapped.reshape(2, 3, 4)
        rows = rows if descriptor & 0x20 else rows[::-1]
        rows = rows[:, ::-1] if descriptor & 0x10 else rows
        assert st == 0 and np.array_equal(pic, rows.reshape(-1))
    st, pic, _ = both(T.packet(2, 2, 1, 24, bytes([1, 2, 3, 4, 5, 6]), 0x30))
    assert st == 0 and list(pic) == [4, 5, 6, 1, 2, 3]  # 24 bits: no swap
    st, pic, _ = both(T.packet(2, 2, 1, 16, bytes([1, 2, 3, 4]), 0x20))
    assert st == 0 and list(pic) == [1, 2, 3, 4]


def test_the_bad_streams_in_the_loop_s_order():
    px = np.arange(12, dtype=np.uint8).reshape(4, 3)
    mk = lambda data: T.packet(10, 4, 1, 24, data)  # noqa: E731
    assert both(mk(T.rle(px, [("raw", 4)])))[0] == 0
    assert both(mk(T.rle(px, [("raw", 4)]) + b"\x00\xff"))[0] == 0               # bytes after a full picture
    assert both(mk(T.rle(px, [("raw", 2)])))[0] == T.SHORT                        # ends at a packet boundary
    assert both(mk(b""))[0] == T.SHORT
    assert both(mk(T.rle(px, [("raw", 2), ("run", 3)])))[0] == T.RLE
    assert both(mk(T.rle(px, [("raw", 2), ("raw", 3)])))[0] == T.RLE
    assert both(mk(T.rle(px, [("raw", 2), ("raw", 3)])[:9]))[0] == T.RLE          # raw: the count goes before the bytes
    assert both(mk(T.rle(px, [("raw", 2), ("run", 3)])[:9]))[0] == T.EOF          # run: the pixel goes before the count
    assert both(mk(T.rle(px, [("raw", 4)])[:-1]))[0] == T.EOF
    assert both(mk(T.rle(px, [("raw", 2)]) + b"\x81"))[0] == T.EOF                # a header and nothing behind it
    assert both(T.packet(2, 4, 1, 24, px.tobytes()[:-1]))[0] == T.EOF             # plain data one byte short
    # maps: an index at origin + length, an index below the origin, both
    cmap = bytes(range(30))
    mp = lambda idx: T.packet(1, 3, 1, 8, bytes(idx), 0x20, map_type=1, map_origin=3, map_length=10, map_depth=24, cmap=cmap)  # noqa: E731
    assert both(mp([3, 12, 5]))[0] == 0
    assert both(mp([3, 13, 5]))[0] == T.INDEX_RANGE
    assert both(mp([3, 2, 5]))[0] == T.BELOW_ORIGIN
    assert both(mp([2, 13, 5]))[0] == both(mp([13, 2, 5]))[0] == T.INDEX_RANGE


def as_packet(v):
    h = v["header"]
    return T.packet(h["image_type"], h["width"], h["height"], h["pixel_depth"], bytes(v["data"]), h.get("image_descriptor", 0),
                    map_type=h.get("color_map_type", 0), map_length=h.get("color_map_length", 0))


def as_palette(v):
    """the caller's palette whose high bytes are the recorded ones (V:111-117)"""
    if v["palette_bytes"] is None:
        return None
    return (np.array(v["palette_bytes"], np.uint16).reshape(-1, 4) << 8 | 0x5a).astype(np.uint16)


@pytest.mark.parametrize("v", VECTORS, ids=[str(i + 1) for i in range(len(VECTORS))])
def test_the_statement_gives_what_upstream_s_code_gave(v):
    st, pic, info = both(as_packet(v), as_palette(v))
    assert st == v["status"]
    if v["read"] != 0:
        assert st == v["read"]
    elif v["unmap"]:
        assert st == v["unmap"]
    if "map_after_read" in v:
        m = v["map_after_read"]
        assert (info.map_depth, info.map_length, info.map_origin) == (m["depth"], m["length"], m["origin"])
    if v["status"] == 0:
        stored = pic.reshape(info.height, info.width, -1)
        stored = stored[::-1] if info.flip_y else stored
        assert list(stored.reshape(-1)) == v["image"]
    assert len(VECTORS) == 7


# ------------------------------------------------------------------ the host-only calls
def header_cases():
    """(name, packet, palette entries, status): every good kind, then every refusal, each made so that the checks after it
    in upstream's order would refuse too where that is possible"""
    rng = np.random.default_rng(5)
    out = []
    for t, d, m in KINDS:
        for descriptor in ORIENTATIONS:
            out.append((f"good type {t} depth {d} map {m} desc {descriptor:#x}",
                        T.random_packet(rng, t, 5, 3, d, descriptor, map_depth=m or 24, map_origin=3 if m else 0, ident=b"abc"), 0, 0))
    out.append(("caller's palette", T.random_packet(rng, 1, 5, 3, 8, 0, from_palette=200), 200, 0))
    out.append(("caller's palette of 300", T.random_packet(rng, 9, 5, 3, 8, 0, from_palette=300), 300, 0))
    H, P = T.header, lambda h, tail=b"": np.frombuffer(h + tail, np.uint8)  # noqa: E731
    out += [
        ("map type 2, image type 0", P(H(0, 0, 0, 7, map_type=2)), 0, T.CMAP_TYPE),
        ("image type 0, zero size", P(H(0, 0, 0, 7)), 0, T.NO_IMG),
        ("image type 4", P(H(4, 0, 0, 7)), 0, T.IMG_TYPE),
        ("image type 12", P(H(12, 5, 3, 8)), 0, T.IMG_TYPE),
        ("mapped, no map, no palette", P(H(1, 0, 0, 7)), 0, T.CMAP_MISSING),
        ("mapped, no map, a palette, zero size", P(H(9, 0, 3, 8)), 4, T.ZERO_SIZE),
        ("mapped, map type 1, length 0, depth 15", P(H(1, 0, 0, 7, map_type=1, map_depth=15)), 4, T.CMAP_LENGTH),
        ("mapped, map type 0 with a length (OOPs), depth 15", P(H(1, 0, 0, 7, map_length=2, map_depth=15)), 4, T.CMAP_DEPTH),
        ("mapped, map depth 8", P(H(9, 5, 3, 8, map_type=1, map_length=2, map_depth=8)), 0, T.CMAP_DEPTH),
        ("width 0", P(H(2, 0, 3, 7)), 0, T.ZERO_SIZE),
        ("height 0", P(H(2, 5, 0, 24)), 0, T.ZERO_SIZE),
        ("depth 15", P(H(2, 5, 3, 15)), 0, T.PIXEL_DEPTH),
        ("depth 0", P(H(3, 5, 3, 0)), 0, T.PIXEL_DEPTH),
        ("mapped at depth 16", P(H(1, 5, 3, 16, map_type=1, map_length=2, map_depth=24), bytes(6)), 0, T.PIXEL_DEPTH),
        ("the id is short", P(H(2, 5, 3, 24, id_length=4), b"abc"), 0, T.EOF),
        ("the map is short", P(H(1, 5, 3, 8, map_type=1, map_origin=2, map_length=3, map_depth=24), bytes(8)), 0, T.EOF),
        ("the map is there", P(H(1, 5, 3, 8, map_type=1, map_origin=2, map_length=3, map_depth=24), bytes(9)), 0, 0),
        ("unmapped with a map of depth 15: 5 * 15 / 8 = 9 bytes", P(H(2, 5, 3, 24, map_type=1, map_length=5, map_depth=15), bytes(9)), 0, 0),
        ("unmapped with a map of depth 15, short", P(H(2, 5, 3, 24, map_type=1, map_length=5, map_depth=15), bytes(8)), 0, T.EOF),
        ("unmapped with a map of length 0", P(H(10, 5, 3, 24, map_type=1)), 0, 0),
        ("nothing", np.zeros(0, np.uint8), 0, T.EOF),
    ]
    return out


CASES = header_cases()


@pytest.mark.parametrize("name,packet,entries,status", CASES, ids=[c[0] for c in CASES])
def test_mi_tga_parse_is_parse_field_for_field(name, packet, entries, status):
    want = T.parse(packet, entries)
    assert want.status == status
    assert tuple(tga.parse(packet, entries)) == tuple(want) and tga.Info._fields == T.Info._fields
    if "unmapped with a map of depth 15:" in name:
        assert want.data_offset == 18 + 9 and want.map_offset == 18
    for cut in range(min(packet.size, 64) + 1):  # every truncation: a short read at any field is EOF, or an earlier refusal
        got, ref = tga.parse(packet[:cut], entries), T.parse(packet[:cut], entries)
        assert tuple(got) == tuple(ref), cut
        assert ref.status in (T.EOF, status) or cut >= want.data_offset


def test_parse_refuses_what_is_no_packet():
    with pytest.raises(tga.MiTgaError):
        tga.parse(np.zeros(18, np.uint8), -1)
    with pytest.raises(tga.MiTgaError):
        tga.parse(np.zeros(18, np.uint8), 65536)


def test_layout_and_tile_pixels():
    assert T.layout("GRAY8", 5, 3) == (15, 1, 5) and T.layout("RGB15", 5, 3) == (30, 2, 10)
    assert T.layout("BGR24", 67, 2) == (402, 3, 201) and T.layout(3, 1, 1) == (4, 4, 4)
    for bad in (("BGR24", 0, 1), ("BGR24", 1, 65536), ("RGBA32", 32768, 16384)):
        with pytest.raises(ValueError):
            T.layout(*bad)
    t = tga.tile_pixels()
    assert t >= 128 and t % 128 == 0 and t & (t - 1) == 0  # at most one tile begins in a packet; the index divides by shifts
    assert (tga.GRAY8, tga.RGB15, tga.BGR24, tga.RGBA32) == tuple(range(4)) == tuple(tga.FORMATS[f] for f in T.FORMATS)
    for name in ("EOF", "CMAP_TYPE", "IMG_TYPE", "NO_IMG", "CMAP_MISSING", "CMAP_LENGTH", "CMAP_DEPTH", "ZERO_SIZE", "PIXEL_DEPTH", "RLE",
                 "INDEX_RANGE", "SHORT", "BELOW_ORIGIN", "MISMATCH"):
        assert getattr(tga, "ST_" + name) == getattr(T, name)


def test_the_builders_build_what_they_say():
    px = np.array([[1], [1], [1], [2], [3], [3]], np.uint8)
    assert T.greedy(px) == [("run", 3), ("raw", 1), ("run", 2)]
    assert T.rle(px, T.greedy(px)) == bytes([0x82, 1, 0x00, 2, 0x81, 3])
    assert T.greedy(np.zeros((300, 1), np.uint8)) == [("run", 128), ("run", 128), ("run", 44)]
    assert T.greedy(np.arange(200, dtype=np.uint8).reshape(-1, 1)) == [("raw", 128), ("raw", 72)]
    assert T.header(2, 0x1234, 3, 24, 0x20, 5, 1, 0x0102, 0x0304, 16) == bytes([5, 1, 2, 2, 1, 4, 3, 16, 0, 0, 0, 0, 0x34, 0x12, 3, 0, 24, 0x20])
    pal = T.random_palette(np.random.default_rng(1), 256)
    assert pal.shape == (256, 4) and ((pal >> 8) != (pal & 0xff)).all()


# ------------------------------------------------------------------ the library and its table
def test_library_exports_exactly_the_declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "mi_tga.h")).read()
    declared = sorted(set(re.findall(r"\b(mi_tga_[a-z0-9_]+)\s*\(", hdr)))
    L = C.CDLL(tga.lib_path())
    for name in declared:
        assert hasattr(L, name), name
    assert sorted(tga.EXPORTS) == declared and len(declared) == 14
    out = subprocess.run(["nm", "-D", "--defined-only", tga.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = sorted(line.split()[-1] for line in out.splitlines() if " T " in line and "mi_tga" in line)
    assert exported == declared


def test_signature_table_matches_the_header():
    declared = prototypes("mi_tga.h", "mi_tga_")
    assert len(declared) == 14
    assert list(tga.SIGNATURES) == list(declared), "the header's order"
    assert set(tga.SIGNATURES) == set(declared) == set(tga.EXPORTS) and len(tga.EXPORTS) == len(declared)
    for name, (ret, args) in declared.items():
        restype, argtypes = tga.SIGNATURES[name]
        assert len(argtypes) == len(args), name
        assert ctypes_kind(restype) == ret, name
        assert [ctypes_kind(t) for t in argtypes] == args, name


def test_info_struct_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "mi_tga.h")).read()
    body = re.search(r"typedef struct mi_tga_info \{(.*?)\} mi_tga_info;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    kinds = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint16_t": C.c_uint16, "uint8_t": C.c_uint8}
    fields = []
    for ctype, names in re.findall(r"(u?int(?:8|16|32)_t)\s+([^;]+);", body):
        for n in names.split(","):
            n = n.strip()
            m = re.fullmatch(r"(\w+)\[(\d+)\]", n)
            fields.append((m.group(1), kinds[ctype] * int(m.group(2))) if m else (n, kinds[ctype]))
    assert [(n, C.sizeof(t)) for n, t in fields] == [(n, C.sizeof(t)) for n, t in tga._Info._fields_]
    assert C.sizeof(tga._Info) == 40 and [n for n, _ in fields[:-1]] == list(tga.Info._fields)
    assert re.search(r"typedef struct \{\s*uint16_t r, g, b, a;\s*\} mi_tga_color;", hdr)
    codes = dict(re.findall(r"MI_TGA_ST_(\w+) = (\d+)", hdr))
    assert {k: int(v) for k, v in codes.items()} == {"OK": 0, "EOF": 2, "CMAP_TYPE": 4, "IMG_TYPE": 5, "NO_IMG": 6, "CMAP_MISSING": 7,
                                                    "CMAP_LENGTH": 9, "CMAP_DEPTH": 10, "ZERO_SIZE": 11, "PIXEL_DEPTH": 12, "RLE": 15,
                                                    "INDEX_RANGE": 16, "SHORT": 32, "BELOW_ORIGIN": 33, "MISMATCH": 34}
