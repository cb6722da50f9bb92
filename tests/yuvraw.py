"""The uncompressed QuickTime YUV family as upstream decodes it: a numpy restatement of lib/video_yuv.c, the checker of
libmi_yuv.so (include/mi_yuv.h).

tests/test_yuv_reference_cpu.py holds this file to lib/video_yuv.c itself, which oracle/Makefile builds as it stands into
oracle/_ref/libvideo_yuv_ref.so where the reference tree is present (tests/yuvref.py), and tests/golden/yuv_ref.json keeps
that build's pictures for checkouts without it.  The restatement is written from the upstream lines cited at every function and from nothing in
csrc/: each function below is the upstream loop of those lines with numpy slices for its `for`, reading the packet at
upstream's strides (`priv->frame->strides`, set in the init_* functions) and writing a picture whose planes lie back to
back, each plane's rows at its own width (`f->strides[p]` = the row), 16-bit samples as native uint16.

  layout(codec, w, h)              Layout, or ValueError for a size at which upstream's loops do not cover the whole picture
                                   and nothing beyond it
  unpack(codec, w, h, packet)      the tight picture's bytes (uint8)
  random_packet(codec, w, h, rng)  a packet of the layout's size, every bit random: row padding, the bits v210 and v410
                                   drop and the fields of a v210 row's last group that no pixel uses included
"""
import collections

import numpy as np

CODECS = ("yuv2", "2vuy", "yv12", "YV12", "VYUY", "YVU9", "v308", "v408", "v410", "v210", "yuv4")  # :779-789
# packet_strides: upstream's priv->frame->strides of the planes the packet has; planes: (width in samples, height, bytes per
# sample) of the picture's planes in the picture's order
Layout = collections.namedtuple("Layout", "packet_bytes picture_bytes packet_strides planes")
LIMIT = 1 << 31


def PAD(size, a):  # :32
    return (size + a - 1) // a * a


def _need(ok, codec, w, h, rule):
    if not ok:
        raise ValueError(f"{codec} at {w} x {h}: {rule}")


def layout(codec, w, h):
    if codec not in CODECS:
        raise ValueError(f"unknown codec {codec}")
    _need(w > 0 and h > 0, codec, w, h, "width and height are positive")
    if codec in ("yuv2", "2vuy", "VYUY"):
        # :96, :209, :239 stride PAD(2w, 4); :71 w/2 pairs a row: an odd w loses its last pixel (and pads the row)
        _need(w % 2 == 0, codec, w, h, "the width is even")
        stride = PAD(2 * w, 4)
        planes = [(w, h, 1), (w // 2, h, 1), (w // 2, h, 1)] if codec == "yuv2" else [(w, h, 2)]
        lay = Layout(stride * h, 2 * w * h, (stride, 0, 0), tuple(planes))
    elif codec in ("yv12", "YV12"):
        # :269-271 strides PAD(w, 2) and half; :255 / :287 h/2 chroma rows
        _need(w % 2 == 0 and h % 2 == 0, codec, w, h, "width and height are even")
        s = PAD(w, 2)
        lay = Layout(s * h + 2 * (s // 2) * (h // 2), w * h + 2 * (w // 2) * (h // 2), (s, s // 2, s // 2),
                     ((w, h, 1), (w // 2, h // 2, 1), (w // 2, h // 2, 1)))
    elif codec == "YVU9":
        # :336-338 strides PAD(w, 8) and a quarter; :322 h/4 chroma rows
        _need(w % 4 == 0 and h % 4 == 0, codec, w, h, "width and height are multiples of 4")
        s = PAD(w, 8)
        lay = Layout(s * h + 2 * (s // 4) * (h // 4), w * h + 2 * (w // 4) * (h // 4), (s, s // 4, s // 4),
                     ((w, h, 1), (w // 4, h // 4, 1), (w // 4, h // 4, 1)))
    elif codec == "v308":  # :392
        lay = Layout(3 * w * h, 3 * w * h, (3 * w, 0, 0), ((w, h, 1),) * 3)
    elif codec == "v408":  # :178
        lay = Layout(4 * w * h, 4 * w * h, (4 * w, 0, 0), ((w, h, 4),))
    elif codec == "v410":  # :446
        lay = Layout(4 * w * h, 6 * w * h, (4 * w, 0, 0), ((w, h, 2),) * 3)
    elif codec == "v210":
        # :536; :476, :502 groups of 6 and a rest of 2 or 4: an odd width has a rest the code does not handle
        _need(w % 2 == 0, codec, w, h, "the width is even")
        stride = PAD(w, 48) * 8 // 3
        lay = Layout(stride * h, 4 * w * h, (stride, 0, 0), ((w, h, 2), (w // 2, h, 2), (w // 2, h, 2)))
    else:  # yuv4 :598 stride PAD(w, 2) * 3; :560 h/2 rows, :567 w/2 macropixels
        _need(w % 2 == 0 and h % 2 == 0, codec, w, h, "width and height are even")
        stride = PAD(w, 2) * 3
        lay = Layout(stride * (h // 2), w * h + 2 * (w // 2) * (h // 2), (stride, 0, 0),
                     ((w, h, 1), (w // 2, h // 2, 1), (w // 2, h // 2, 1)))
    _need(lay.packet_bytes < LIMIT and lay.picture_bytes < LIMIT, codec, w, h, "packet and picture stay below 2^31 bytes")
    return lay


def alpha_v408(x):
    """include/mi_yuv.h's closed form of decode_alpha_v408 (:104-138), for an array of bytes"""
    x = np.asarray(x).astype(np.int64)
    return np.where(x < 2, 0, np.minimum(255, ((x - 2) * 255 + 43) // 219)).astype(np.uint8)


def _rows(packet, stride, h):
    return packet[:stride * h].reshape(h, stride)


def _words(rows):
    """GAVL_PTR_2_32LE over every aligned word of the rows"""
    b = rows.astype(np.uint32)
    return b[:, 0::4] | b[:, 1::4] << 8 | b[:, 2::4] << 16 | b[:, 3::4] << 24


def _tight(*planes):
    return np.concatenate([np.ascontiguousarray(p).reshape(-1).view(np.uint8) for p in planes])


def _yuv2(w, h, lay, packet):  # :64-82
    src = _rows(packet, lay.packet_strides[0], h)[:, :2 * w]
    return _tight(src[:, 0::2], src[:, 1::4] ^ 0x80, src[:, 3::4] ^ 0x80)


def _handed_on(w, h, lay, packet):  # :191-196, :221-226: the packet is the frame
    return _tight(_rows(packet, lay.packet_strides[0], h)[:, :2 * w])


def _planar(w, h, lay, packet, first, second):
    """:253-255, :285-287, :320-322: the plane behind Y is planes[first], the one behind it planes[second]"""
    s, c = lay.packet_strides[0], lay.packet_strides[1]
    cw, ch, _ = lay.planes[1]
    planes = {0: _rows(packet, s, h)[:, :w]}
    planes[first] = _rows(packet[s * h:], c, ch)[:, :cw]
    planes[second] = _rows(packet[s * h + c * ch:], c, ch)[:, :cw]
    return _tight(planes[0], planes[1], planes[2])


def _v308(w, h, lay, packet):  # :358-377
    src = _rows(packet, 3 * w, h)
    return _tight(src[:, 1::3], src[:, 2::3], src[:, 0::3])


def _v408(w, h, lay, packet):  # :150-163
    src = _rows(packet, 4 * w, h)
    dst = np.empty_like(src)
    dst[:, 0::4], dst[:, 1::4], dst[:, 2::4], dst[:, 3::4] = src[:, 1::4], src[:, 0::4], src[:, 2::4], alpha_v408(src[:, 3::4])
    return _tight(dst)


def _v410(w, h, lay, packet):  # :414-432
    i = _words(_rows(packet, 4 * w, h))
    v, y, u = (i & 0xffc00000) >> 16, (i & 0x3ff000) >> 6, (i & 0xffc) << 4
    return _tight(y.astype(np.uint16), u.astype(np.uint16), v.astype(np.uint16))


def _v210(w, h, lay, packet):  # :468-522
    words = _words(_rows(packet, lay.packet_strides[0], h))
    groups = (w + 5) // 6  # :476 w/6 whole groups, :503 one more where pixels remain
    i1, i2, i3, i4 = (words[:, k:4 * groups:4] for k in range(4))
    lo, mid, hi = (lambda x: (x & 0x3ff) << 6), (lambda x: (x & 0xffc00) >> 4), (lambda x: (x & 0x3ff00000) >> 14)
    y = np.stack([mid(i1), lo(i2), hi(i2), mid(i3), lo(i4), hi(i4)], axis=2).reshape(h, 6 * groups)  # :486-498
    u = np.stack([lo(i1), mid(i2), hi(i3)], axis=2).reshape(h, 3 * groups)
    v = np.stack([hi(i1), lo(i3), mid(i4)], axis=2).reshape(h, 3 * groups)
    # :502-521 of the last group only the first 2 or 4 pixels and their chroma are written: the row ends at w
    return _tight(y[:, :w].astype(np.uint16), u[:, :w // 2].astype(np.uint16), v[:, :w // 2].astype(np.uint16))


def _yuv4(w, h, lay, packet):  # :560-583
    src = _rows(packet, lay.packet_strides[0], h // 2)[:, :3 * w]
    y = np.empty((h, w), np.uint8)
    y[0::2, 0::2], y[0::2, 1::2], y[1::2, 0::2], y[1::2, 1::2] = src[:, 2::6], src[:, 3::6], src[:, 4::6], src[:, 5::6]
    return _tight(y, src[:, 0::6] ^ 0x80, src[:, 1::6] ^ 0x80)


def unpack(codec, w, h, packet):
    lay = layout(codec, w, h)
    packet = np.ascontiguousarray(packet, np.uint8).reshape(-1)
    if packet.size < lay.packet_bytes:
        raise ValueError(f"{codec} at {w} x {h}: a packet of {packet.size} bytes, upstream reads {lay.packet_bytes}")
    if codec == "yuv2":
        pic = _yuv2(w, h, lay, packet)
    elif codec in ("2vuy", "VYUY"):
        pic = _handed_on(w, h, lay, packet)
    elif codec == "yv12":
        pic = _planar(w, h, lay, packet, 1, 2)
    elif codec in ("YV12", "YVU9"):
        pic = _planar(w, h, lay, packet, 2, 1)
    else:
        pic = {"v308": _v308, "v408": _v408, "v410": _v410, "v210": _v210, "yuv4": _yuv4}[codec](w, h, lay, packet)
    assert pic.size == lay.picture_bytes
    return pic


def random_packet(codec, w, h, rng):
    return rng.integers(0, 256, layout(codec, w, h).packet_bytes, dtype=np.uint8)


def planes_of(codec, w, h, pic):
    """the tight picture's planes as 2-D uint8 arrays of (height, row bytes)"""
    out, at = [], 0
    for pw, ph, bps in layout(codec, w, h).planes:
        out.append(pic[at:at + pw * ph * bps].reshape(ph, pw * bps))
        at += pw * ph * bps
    return out
