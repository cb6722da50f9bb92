"""The reference's own lib/video_yuv.c beside the statement tests/yuvraw.py.  TEST INFRASTRUCTURE ONLY.

oracle/Makefile builds lib/video_yuv.c, where the reference tree is present, into oracle/_ref/libvideo_yuv_ref.so against
csrc/compat_lite's stand-in header plus a few declarations and glue of this repository's own (oracle/video_yuv_ref/);
reference() loads it, have_reference() says whether it is there.  decode() sends one packet through the decoder of a
fourcc and returns the planes as that decoder left them, each as its rows at the width gavl gives the pixel format the
decoder set.  packets() are the seeded packets shared by tests/test_yuv_reference_cpu.py (live reference),
tests/golden/make_yuv_ref.py (its recorded answers) and tests/test_gpu_yuv_reference.py (the kernels against those)."""
import ctypes as C
import hashlib
import os

import numpy as np

import yuvraw as Y
from pkg import ROOT
from test_gpu_yuvraw import CASES, SHAPES  # noqa: F401  (the GPU suite's own table of shapes; importing it needs no device)

REF_SO = os.path.join(ROOT, "oracle", "_ref", "libvideo_yuv_ref.so")
PACKETS = 3
# width and height at the smallest values libmi_yuv accepts (yuvraw.layout's rules), one shape per codec
SMALLEST = {"yuv2": (2, 1), "2vuy": (2, 1), "VYUY": (2, 1), "yv12": (2, 2), "YV12": (2, 2), "yuv4": (2, 2), "YVU9": (4, 4),
            "v308": (1, 1), "v408": (1, 1), "v410": (1, 1), "v210": (2, 1)}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).view(np.uint8).tobytes()).hexdigest()


def fourcc(codec):
    a, b, c, d = codec.encode()
    return a << 24 | b << 16 | c << 8 | d


def have_reference():
    return os.path.exists(REF_SO)


_ref = None


def reference():
    global _ref
    if _ref is None:
        L = C.CDLL(REF_SO)
        L.mi_yuvref_fourcc.restype, L.mi_yuvref_fourcc.argtypes = C.c_uint32, [C.c_int]
        L.mi_yuvref_decode.restype = C.c_long
        L.mi_yuvref_decode.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_long, C.POINTER(C.c_int32)]
        _ref = L
    return _ref


def decoders():
    """the first fourcc of every registered decoder, in the order of registration, as text"""
    L = reference()
    return [L.mi_yuvref_fourcc(i).to_bytes(4, "big").decode() for i in range(L.mi_yuvref_num_decoders())]


def decode(codec, w, h, packet):
    """-> (planes: 2-D uint8 arrays of (rows, row bytes); strides the decoder left; handed_on: whether the rows lie in the
    packet itself).  The packet is given to the decoder in an allocation of exactly its size"""
    packet = np.ascontiguousarray(packet, np.uint8)
    out, info = np.zeros(6 * w * h + 64, np.uint8), np.zeros(14, np.int32)
    n = reference().mi_yuvref_decode(fourcc(codec), w, h, packet.ctypes.data, packet.size, out.ctypes.data, out.size, info.ctypes.data_as(C.POINTER(C.c_int32)))
    assert n > 0, f"{codec} at {w} x {h}: the reference build answered {n}"
    planes, strides, at = [], [], 0
    for p in range(int(info[1])):
        row, rows, stride = (int(x) for x in info[2 + 3 * p:5 + 3 * p])
        planes.append(out[at:at + row * rows].reshape(rows, row).copy())
        strides.append(stride)
        at += row * rows
    assert at == n
    return planes, strides


def packets(codec, w, h):
    """the three seeded packets of a shape: yuvraw.random_packet's, which have the reference's own row padding"""
    rng = np.random.default_rng(770000 + 1000 * Y.CODECS.index(codec) + 7 * w + h)
    return [Y.random_packet(codec, w, h, rng) for _ in range(PACKETS)]


# ------------------------------------------------------------------ the reference's recorded answers (tests/golden/yuv_ref.json)
FIXTURE = os.path.join(ROOT, "tests", "golden", "yuv_ref.json")
RAW_LIMIT = 2048  # a picture of at most this many bytes is kept as bytes, a larger one as its SHA-256


def case_id(codec, w, h):
    return f"{codec}-{w}x{h}"


def b64(a):
    import base64
    return base64.b64encode(np.ascontiguousarray(a).view(np.uint8).tobytes()).decode()


def kept(picture):
    """a picture as the fixture keeps it"""
    picture = np.ascontiguousarray(picture, np.uint8).reshape(-1)
    return {"bytes": b64(picture)} if picture.size <= RAW_LIMIT else {"sha256": sha(picture), "size": int(picture.size)}


def records(picture_of):
    """the fixture's content from an answerer picture_of(codec, w, h, packet) -> the tight picture's bytes.  With the
    reference's (ref_records) it is what the file holds; with the statement's it must come out the same"""
    out = {}
    for codec, w, h in CASES:
        ps = packets(codec, w, h)
        out[case_id(codec, w, h)] = {"packets": [sha(p) for p in ps], "pictures": [kept(picture_of(codec, w, h, p)) for p in ps]}
    return out


def ref_picture(codec, w, h, packet):
    return np.concatenate([p.reshape(-1) for p in decode(codec, w, h, packet)[0]])


def ref_records():
    return records(ref_picture)


def fixture():
    import json
    with open(FIXTURE) as f:
        return json.load(f)
