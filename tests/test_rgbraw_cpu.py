"""No-GPU checks of libmi_rgb.so (include/mi_rgb.h): the exported symbols, the signature table against the header, the
host-only calls (mi_rgb_codec_of over everything the two upstream inits accept and a list of what they refuse, mi_rgb_layout_of
against the statement's layout, tests/rgbraw.py, with every refusal and its message), and the statement itself: its
vectorised form against its loop-for-loop form at every shape of the GPU suite, and on hand-written pixels."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import rgbraw as R
from pkg import ROOT
from test_ctypes_signatures_cpu import c_kind, ctypes_kind, prototypes  # noqa: F401  (c_kind: what prototypes() is made of)

rgb = importlib.import_module("gmerlin-avdecoder_amd.rgb")

# the shapes of the GPU suite (tests/test_gpu_rgbraw.py pins them)
SUB_BYTE = {"QT1": [(8, 1), (16, 3), (24, 2), (720, 2)], "QT2": [(4, 1), (8, 3), (12, 2), (720, 2)],
            "QT4": [(2, 1), (4, 3), (6, 2), (720, 2)]}
BYTES = [(1, 1), (2, 2), (5, 3), (67, 2), (720, 2)]
SHAPES = {c: SUB_BYTE.get(c, BYTES) for c in R.CODECS}
CASES = [(c, w, h) for c in R.CODECS for w, h in SHAPES[c]]


def test_library_exports_exactly_the_declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "mi_rgb.h")).read()
    declared = sorted(set(re.findall(r"\b(mi_rgb_[a-z0-9_]+)\s*\(", hdr)))
    L = C.CDLL(rgb.lib_path())
    for name in declared:
        assert hasattr(L, name), name
    assert sorted(rgb.EXPORTS) == declared and len(declared) == 14
    # and nothing else with the prefix leaves the library
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", rgb.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = sorted(line.split()[-1] for line in out.splitlines() if " T " in line and "mi_rgb" in line)
    assert exported == declared


def test_signature_table_matches_the_header():
    declared = prototypes("mi_rgb.h", "mi_rgb_")
    assert len(declared) == 14
    assert list(rgb.SIGNATURES) == list(declared), "the header's order"
    assert set(rgb.SIGNATURES) == set(declared) == set(rgb.EXPORTS) and len(rgb.EXPORTS) == len(declared)
    for name, (ret, args) in declared.items():
        restype, argtypes = rgb.SIGNATURES[name]
        assert len(argtypes) == len(args), name
        assert ctypes_kind(restype) == ret, name
        assert [ctypes_kind(t) for t in argtypes] == args, name


def test_layout_struct_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "mi_rgb.h")).read()
    body = re.search(r"typedef struct mi_rgb_layout \{(.*?)\} mi_rgb_layout;", hdr, re.S).group(1)
    fields = []
    for ctype, names in re.findall(r"(int64_t|int32_t)\s+([^;]+);", body):
        fields += [(n.strip(), C.c_int64 if ctype == "int64_t" else C.c_int32) for n in names.split(",")]
    assert fields == list(rgb._Layout._fields_) and [n for n, _ in fields] == list(rgb.Layout._fields)
    color = re.search(r"typedef struct \{\s*uint16_t r, g, b, a;\s*\} mi_rgb_color;", hdr)
    assert color, "a palette entry is four uint16: what the (n, entries, 4) arrays of the view are"


# ------------------------------------------------------------------ mi_rgb_codec_of
def test_codec_of_everything_the_two_inits_accept():
    qt = {1: "QT1", 2: "QT2", 4: "QT4", 8: "QT8", 16: "QT16", 24: "QT24", 32: "QT32", 34: "QT2", 36: "QT4", 40: "QT8"}
    for depth, name in qt.items():
        assert rgb.codec_of("raw ", depth, True) == rgb.CODECS[name], depth
        # video_qtraw.c:242, :259, :292 refuse depths 1, 2, 8 without a palette; 4 is never decoded upstream (:276) and
        # needs its palette here; the init looks at no palette for 16, 24, 32 and the grey depths
        assert rgb.codec_of("raw ", depth, False) == (-1 if depth in (1, 2, 4, 8) else rgb.CODECS[name]), depth
    for fourcc in ("RGB ", "RGB3", "MTV "):
        for pal in (True, False):
            assert rgb.codec_of(fourcc, 8, pal) == (rgb.AVI8 if pal else rgb.AVI8_GRAY)  # video_aviraw.c:229-245
            assert rgb.codec_of(fourcc, 16, pal) == (rgb.MTV16 if fourcc == "MTV " else rgb.AVI16)  # :246-257
            assert rgb.codec_of(fourcc, 24, pal) == rgb.AVI24 and rgb.codec_of(fourcc, 32, pal) == rgb.AVI32
    assert rgb.codec_of(int.from_bytes(b"raw ", "big"), 24, False) == rgb.QT24
    assert rgb.codec_of(b"MTV ", 16, False) == rgb.MTV16
    assert tuple(rgb.CODECS) == R.CODECS and list(rgb.CODECS.values()) == list(range(13))


def test_codec_of_what_they_refuse():
    for fourcc, depth in (("raw ", 0), ("raw ", 3), ("raw ", 15), ("raw ", 33), ("raw ", 48), ("raw ", -1),
                          ("RGB ", 1), ("RGB ", 4), ("RGB3", 1), ("MTV ", 4),          # `#if 0` upstream
                          ("RGB ", 2), ("RGB ", 15), ("RGB ", 34), ("RGB3", 40), ("MTV ", 0),
                          ("rgb ", 24), ("RAW ", 24), ("raw", 24), ("yuv2", 16), ("2vuy", 16), ("\0\0\0\0", 8), ("BGR ", 24)):
        for pal in (True, False):
            assert rgb.codec_of(fourcc, depth, pal) == -1, (fourcc, depth, pal)


# ------------------------------------------------------------------ mi_rgb_layout_of
SIZES = [(w, h) for w in range(1, 51) for h in range(1, 51)] + [(720, 576), (1920, 1080)]


@pytest.mark.parametrize("codec", R.CODECS)
def test_layout_of_against_the_statement(codec):
    accepted = refused = 0
    mult = {"QT1": 8, "QT2": 4, "QT4": 2}.get(codec)
    for w, h in SIZES:
        try:
            want = R.layout(codec, w, h)
        except ValueError:
            with pytest.raises(rgb.MiRgbError, match=f"{codec} at {w} x {h}: the width is a multiple of {mult}$") as e:
                rgb.layout_of(codec, w, h)
            assert e.value.code == rgb.ERR_ARG
            refused += 1
            continue
        got = rgb.layout_of(codec, w, h)
        assert got == want, (codec, w, h, got, want)
        assert got.picture_bytes == w * h * got.bytes_per_pixel and got.packet_bytes == got.packet_stride * h
        accepted += 1
    assert accepted and bool(refused) == (mult is not None)


def test_layout_spot_values_and_the_issue_s_strides():
    assert [rgb.layout_of("QT24", w, 2).packet_stride for w in (1, 2, 5, 67)] == [4, 6, 16, 202]
    assert [rgb.layout_of("AVI24", w, 2).packet_stride for w in (1, 2, 5, 67)] == [4, 8, 16, 204]
    assert [rgb.layout_of("AVI16", w, 2).packet_stride for w in (1, 2, 5, 67)] == [4, 4, 12, 136]
    assert [rgb.layout_of("QT1", w, 1).packet_stride for w in (8, 16, 24, 720)] == [2, 2, 4, 90]
    assert [rgb.layout_of("QT2", w, 1).packet_stride for w in (4, 8, 12, 720)] == [2, 2, 4, 180]
    assert [rgb.layout_of("QT4", w, 1).packet_stride for w in (2, 4, 6, 720)] == [2, 2, 4, 360]
    assert rgb.layout_of("QT8", 5, 3) == (18, 45, 6, 3, 256, False)
    assert rgb.layout_of("AVI8", 5, 3) == (24, 45, 8, 3, 256, True)
    assert rgb.layout_of("AVI8_GRAY", 5, 3) == (24, 15, 8, 1, 0, True)
    assert rgb.layout_of("QT32", 1920, 1080) == (4 * 1920 * 1080, 4 * 1920 * 1080, 7680, 4, 0, False)
    assert rgb.layout_of("QT1", 1920, 1080) == (240 * 1080, 3 * 1920 * 1080, 240, 3, 2, False)
    assert [rgb.layout_of(c, 8, 1).palette_entries for c in ("QT1", "QT2", "QT4", "QT8", "AVI8")] == [2, 4, 16, 256, 256]


def test_every_other_refusal_and_its_message():
    for codec in R.CODECS:
        for w, h in ((0, 2), (8, 0), (-8, 2), (8, -4)):
            with pytest.raises(rgb.MiRgbError, match=f"{codec} at {w} x {h}: width and height are positive") as e:
                rgb.layout_of(codec, w, h)
            assert e.value.code == rgb.ERR_ARG
            with pytest.raises(ValueError, match="positive"):
                R.layout(codec, w, h)
    for codec, w, mult in (("QT1", 12, 8), ("QT1", 1, 8), ("QT2", 6, 4), ("QT2", 2, 4), ("QT4", 3, 2), ("QT4", 1, 2)):
        with pytest.raises(rgb.MiRgbError, match=f"the width is a multiple of {mult}"):
            rgb.layout_of(codec, w, 2)
        with pytest.raises(ValueError, match=f"the width is a multiple of {mult}"):
            R.layout(codec, w, 2)
    # 2^31 bytes or more: pictures of 3 and 4 bytes a pixel, packets of 4
    for codec, w, h in (("QT1", 32768, 21846), ("QT8", 32768, 21846), ("AVI24", 32768, 21846), ("QT32", 32768, 16384),
                        ("AVI32", 16384, 32768), ("QT16", 32768, 32768), ("AVI8_GRAY", 65536, 32768), ("QT24", 1 << 30, 1 << 30)):
        with pytest.raises(rgb.MiRgbError, match=f"{codec} at {w} x {h}: packets and pictures stay below 2\\^31 bytes"):
            rgb.layout_of(codec, w, h)
        with pytest.raises(ValueError, match="below 2\\^31"):
            R.layout(codec, w, h)
    assert rgb.layout_of("QT1", 32768, 21845).picture_bytes == 3 * 32768 * 21845 < 1 << 31
    for codec in (-1, 13, 99):
        with pytest.raises(rgb.MiRgbError, match=f"unknown codec {codec}"):
            rgb.layout_of(codec, 8, 4)
    with pytest.raises(ValueError, match="unknown codec"):
        R.layout("QT3", 8, 4)


def test_no_device_fails_loudly():
    if os.path.exists("/dev/kfd"):
        pytest.skip("only meaningful without a GPU")
    with pytest.raises(rgb.MiRgbError, match="no CPU path|no HIP device|gfx950"):
        rgb.MiRgb()


def test_the_view_refuses_a_short_palette_before_the_library_reads_past_it():
    for codec, entries in (("QT1", 2), ("QT2", 4), ("QT4", 16), ("QT8", 256), ("AVI8", 256)):
        with pytest.raises(rgb.MiRgbError, match="shorter palette is refused"):
            rgb._palettes(codec, 8, 1, np.zeros((1, entries - 1, 4), np.uint16))
        assert rgb._palettes(codec, 8, 1, np.zeros((2, entries, 4), np.uint16)).shape == (2, entries, 4)
        assert rgb._palettes(codec, 8, 1, np.zeros((entries, 4), np.uint16)).shape == (1, entries, 4)
        with pytest.raises(ValueError, match="palette"):
            R.unpack(codec, 8, 1, np.zeros(8, np.uint8), np.zeros((entries - 1, 4), np.uint16))


# ------------------------------------------------------------------ the statement: its two forms, and hand-written pixels
def palette_for(codec, rng):
    return R.random_palette(codec, rng) if R.layout(codec, 8, 1).palette_entries else None


@pytest.mark.parametrize("codec,w,h", CASES, ids=[f"{c}-{w}x{h}" for c, w, h in CASES])
def test_unpack_against_unpack_literal(codec, w, h):
    rng = np.random.default_rng(1000 * R.CODECS.index(codec) + w + h)
    packet, palette = R.random_packet(codec, w, h, rng), palette_for(codec, rng)
    before = packet.copy()
    a, b = R.unpack(codec, w, h, packet, palette), R.unpack_literal(codec, w, h, packet, palette)
    assert a.dtype == b.dtype == np.uint8 and a.size == b.size == R.layout(codec, w, h).picture_bytes
    assert np.array_equal(a, b), (codec, w, h, int(np.flatnonzero(a != b)[0]))
    assert np.array_equal(packet, before), "the statement works on a copy"


def test_random_palettes_tell_the_high_byte_from_the_low():
    rng = np.random.default_rng(2)
    for codec in ("QT1", "QT2", "QT4", "QT8", "AVI8"):
        p = R.random_palette(codec, rng)
        assert p.dtype == np.uint16 and p.shape == (R.layout(codec, 8, 1).palette_entries, 4)
        assert ((p >> 8) != (p & 0xff)).all()
    assert len({int(x) for x in R.random_palette("QT8", rng)[:, 0] >> 8}) > 100


def b(*v):
    return np.array(v, np.uint8)


def pal(*rgb16):
    return np.array([list(c) + [0xFFFF] for c in rgb16], np.uint16)


def test_QT1_bits_high_first_and_the_high_byte_of_the_palette():
    p = pal((0x1234, 0x5678, 0x9ABC), (0xFEDC, 0xBA98, 0x7654))
    got = R.unpack("QT1", 8, 1, b(0b10110001, 0xFF), p).reshape(8, 3)  # the second byte is the row's padding
    one, zero = [0xFE, 0xBA, 0x76], [0x12, 0x56, 0x9A]
    assert got.tolist() == [one, zero, one, one, zero, zero, zero, one]


def test_QT2_and_QT4_fields_high_first():
    p4 = pal(*[(0x100 * k + 0x80, 0x1000 + 0x100 * k, 0x2000 + 0x100 * k) for k in range(4)])
    assert R.unpack("QT2", 4, 1, b(0b11100100, 0), p4).reshape(4, 3)[:, 0].tolist() == [3, 2, 1, 0]
    p16 = pal(*[(0x100 * k + 0x7F, 0, 0) for k in range(16)])
    assert R.unpack("QT4", 4, 1, b(0xA5, 0x0F), p16).reshape(4, 3)[:, 0].tolist() == [0xA, 0x5, 0x0, 0xF]


def test_QT8_and_AVI8_rows_and_padding():
    p = pal(*[(0x100 * k + 1, 0x100 * (255 - k) + 2, 0x8000 + k) for k in range(256)])
    # QT8 3 x 2: stride 4, the fourth byte of a row is padding
    got = R.unpack("QT8", 3, 2, b(1, 2, 3, 0xEE, 4, 5, 6, 0xEE), p).reshape(2, 3, 3)
    assert got[:, :, 0].tolist() == [[1, 2, 3], [4, 5, 6]] and got[0, 0].tolist() == [1, 254, 0x80]
    # AVI8 the same bytes: bottom-up
    assert R.unpack("AVI8", 3, 2, b(1, 2, 3, 0xEE, 4, 5, 6, 0xEE), p).reshape(2, 3, 3)[:, :, 0].tolist() == [[4, 5, 6], [1, 2, 3]]
    assert R.unpack("AVI8_GRAY", 3, 2, b(1, 2, 3, 0xEE, 4, 5, 6, 0xEE)).tolist() == [4, 5, 6, 1, 2, 3]


def test_the_16_bit_codecs():
    assert R.unpack("QT16", 2, 1, b(0x12, 0x34, 0x56, 0x78)).view(np.uint16).tolist() == [0x1234, 0x5678]
    assert R.unpack("MTV16", 2, 1, b(0x12, 0x34, 0x56, 0x78)).tolist() == [0x34, 0x12, 0x78, 0x56]
    assert R.unpack("AVI16", 1, 2, b(1, 2, 0xEE, 0xEE, 3, 4, 0xEE, 0xEE)).tolist() == [3, 4, 1, 2]


def test_the_24_and_32_bit_codecs():
    assert R.unpack("QT24", 1, 2, b(1, 2, 3, 0xEE, 4, 5, 6, 0xEE)).tolist() == [1, 2, 3, 4, 5, 6]
    assert R.unpack("AVI24", 1, 2, b(1, 2, 3, 0xEE, 4, 5, 6, 0xEE)).tolist() == [4, 5, 6, 1, 2, 3]
    assert R.unpack("QT32", 1, 2, b(0xA0, 1, 2, 3, 0xA1, 4, 5, 6)).tolist() == [1, 2, 3, 0xA0, 4, 5, 6, 0xA1]
    assert R.unpack("AVI32", 1, 2, b(1, 2, 3, 4, 5, 6, 7, 8)).tolist() == [5, 6, 7, 8, 1, 2, 3, 4]


def test_the_statement_refuses_what_it_cannot_state():
    with pytest.raises(ValueError, match="upstream reads"):
        R.unpack("QT24", 2, 2, np.zeros(11, np.uint8))
    with pytest.raises(ValueError, match="palette"):
        R.unpack("QT8", 2, 2, np.zeros(4, np.uint8))
    with pytest.raises(ValueError, match="no palette"):
        R.unpack("QT24", 2, 2, np.zeros(12, np.uint8), np.zeros((256, 4), np.uint16))
