"""The raw RGB family of QuickTime and AVI as upstream decodes it: a restatement of lib/video_qtraw.c (Q below) and
lib/video_aviraw.c (A), the checker of libmi_rgb.so (include/mi_rgb.h).  Pinned by statement, not yet by build: nothing
holds this file to a build of the two upstream files.

It is written from the upstream lines cited at every function and from nothing in csrc/, and states the arithmetic twice:

  unpack(codec, w, h, packet, palette)          vectorised numpy: bit fields by shifts of whole rows, the palette as a
                                                fancy index, the flip as a reversed slice
  unpack_literal(codec, w, h, packet, palette)  upstream's loops one for one on a copy of the packet: the counter, the
                                                shift of the source byte in place, `src++`, `dst -= stride`

Both give the tight picture's bytes (uint8): rows of w * bytes_per_pixel, top row first, 16-bit pixels as native uint16.

  layout(codec, w, h)              Layout, or ValueError for a size at which upstream's row loop leaves the row it was given
  random_packet(codec, w, h, rng)  a packet of the layout's size, every bit random, row padding included
  random_palette(codec, rng)       (entries, 4) uint16: r, g, b, a; the high and the low byte of every component differ,
                                   so `>> 8` cannot be mistaken for `& 0xff` or for a rounding conversion

A palette entry gives R, G, B = r >> 8, g >> 8, b >> 8 (BGAV_PALETTE_2_RGB24, avdec_private.h:122-125)."""
import collections

import numpy as np

CODECS = ("QT1", "QT2", "QT4", "QT8", "QT16", "QT24", "QT32", "AVI8", "AVI8_GRAY", "AVI16", "MTV16", "AVI24", "AVI32")
Layout = collections.namedtuple("Layout", "packet_bytes picture_bytes packet_stride bytes_per_pixel palette_entries bottom_up")
LIMIT = 1 << 31

# codec: (bits a pixel in the packet, bytes a pixel in the picture, palette entries)
_QT = {"QT1": (1, 3, 2), "QT2": (2, 3, 4), "QT4": (4, 3, 16), "QT8": (8, 3, 256), "QT16": (16, 2, 0), "QT24": (24, 3, 0),
       "QT32": (32, 4, 0)}
_AVI = {"AVI8": (8, 3, 256), "AVI8_GRAY": (8, 1, 0), "AVI16": (16, 2, 0), "MTV16": (16, 2, 0), "AVI24": (24, 3, 0),
        "AVI32": (32, 4, 0)}


def _need(ok, codec, w, h, rule):
    if not ok:
        raise ValueError(f"{codec} at {w} x {h}: {rule}")


def layout(codec, w, h):
    if codec not in CODECS:
        raise ValueError(f"unknown codec {codec}")
    _need(w > 0 and h > 0, codec, w, h, "width and height are positive")
    if codec in _QT:
        bits, bpp, entries = _QT[codec]
        if bits < 8:
            # Q:240, :257, :274 bytes_per_line = width / (8 / bits), and the row loop takes `width` pixels (Q:400): another
            # width reads the next row's first byte
            _need(w % (8 // bits) == 0, codec, w, h, f"the width is a multiple of {8 // bits}")
        stride = w * bits // 8  # Q:240, :257, :274, :290, :306, :316, :326
        if stride & 1:          # Q:365-366
            stride += 1
        bottom_up = False
    else:
        bits, bpp, entries = _AVI[codec]
        stride = (w * bits + 7) // 8  # A:273
        if stride % 4:                # A:276-279
            stride += 4 - stride % 4
        bottom_up = True              # A:183-192
    lay = Layout(stride * h, w * bpp * h, stride, bpp, entries, bottom_up)
    _need(lay.packet_bytes < LIMIT and lay.picture_bytes < LIMIT, codec, w, h, "packets and pictures stay below 2^31 bytes")
    return lay


def random_packet(codec, w, h, rng):
    return rng.integers(0, 256, layout(codec, w, h).packet_bytes, dtype=np.uint8)


def random_palette(codec, rng):
    entries = (_QT.get(codec) or _AVI[codec])[2]
    assert entries, f"{codec} has no palette"
    hi = rng.integers(0, 256, (entries, 4), dtype=np.uint16)
    lo = (hi + rng.integers(1, 256, (entries, 4), dtype=np.uint16)) & 0xff  # never the high byte
    return (hi << 8 | lo).astype(np.uint16)


def _checked(codec, w, h, packet, palette):
    lay = layout(codec, w, h)
    packet = np.ascontiguousarray(packet, np.uint8).reshape(-1)
    if packet.size < lay.packet_bytes:
        raise ValueError(f"{codec} at {w} x {h}: a packet of {packet.size} bytes, upstream reads {lay.packet_bytes}")
    if lay.palette_entries:
        if palette is None:
            raise ValueError(f"{codec}: a palette of {lay.palette_entries} entries is needed")
        palette = np.asarray(palette, np.uint16)
        if palette.ndim != 2 or palette.shape[0] < lay.palette_entries or palette.shape[1] != 4:
            raise ValueError(f"{codec}: a palette of shape {palette.shape}, {lay.palette_entries} entries of r, g, b, a are needed")
    elif palette is not None:
        raise ValueError(f"{codec} has no palette")
    return lay, packet, palette


# ------------------------------------------------------------------ vectorised
def unpack(codec, w, h, packet, palette=None):
    lay, packet, palette = _checked(codec, w, h, packet, palette)
    rows = packet[:lay.packet_bytes].reshape(h, lay.packet_stride)
    if lay.bottom_up:
        rows = rows[::-1]  # A:185, :191: packet row i is picture row h - 1 - i
    bits = (_QT.get(codec) or _AVI[codec])[0]
    if lay.palette_entries:
        if bits == 8:  # Q:106-118, A:50-60
            index = rows[:, :w]
        else:          # Q:43-104: pixel i is the field of `bits` bits that begins at bit 7 - (i * bits) % 8 of byte i * bits / 8
            i = np.arange(w)
            index = (rows[:, i * bits // 8] >> (8 - bits - i * bits % 8).astype(np.uint8)) & ((1 << bits) - 1)
        pic = (palette[index, :3] >> 8).astype(np.uint8)
    elif codec in ("QT16", "MTV16"):  # Q:130-131 big-endian to native; A:98-102 the two bytes swapped (little-endian host)
        used = rows[:, :2 * w].astype(np.uint16)
        pic = (used[:, 0::2] << 8 | used[:, 1::2]).astype(np.uint16)
    elif codec == "QT32":  # Q:153-156
        used = rows[:, :4 * w].reshape(h, w, 4)
        pic = used[:, :, [1, 2, 3, 0]]
    else:  # Q:142, A:68, :80, :111, :117
        pic = rows[:, :w * lay.bytes_per_pixel]
    pic = np.ascontiguousarray(pic).reshape(-1).view(np.uint8)
    assert pic.size == lay.picture_bytes
    return pic


# ------------------------------------------------------------------ loop for loop
def _palette_2_rgb24(entry, dst, d):  # avdec_private.h:122-125
    dst[d] = int(entry[0]) >> 8
    dst[d + 1] = int(entry[1]) >> 8
    dst[d + 2] = int(entry[2]) >> 8


def _scanline_sub_byte(bits):
    """scanline_raw_1, _2, _4 (Q:43-104) and the two grey ones (Q:162-209), which differ in the constants only"""
    per_byte, mask, shift = 8 // bits, (0xff << (8 - bits)) & 0xff, 8 - bits

    def scanline(buf, src, dst, d, num_pixels, pal):
        counter = 0
        for _ in range(num_pixels):
            if counter == per_byte:
                counter = 0
                src += 1
            _palette_2_rgb24(pal[(buf[src] & mask) >> shift], dst, d)
            buf[src] = (buf[src] << bits) & 0xff  # *src <<= bits: the packet is destroyed
            d += 3
            counter += 1
    return scanline


def _scanline_8(buf, src, dst, d, num_pixels, pal):  # Q:106-118, A:50-60
    for _ in range(num_pixels):
        _palette_2_rgb24(pal[buf[src]], dst, d)
        src += 1
        d += 3


def _scanline_8_gray(buf, src, dst, d, num_pixels, pal):  # A:62-72
    for _ in range(num_pixels):
        dst[d] = buf[src]
        src += 1
        d += 1


def _scanline_raw_16(buf, src, dst, d, num_pixels, pal):  # Q:120-135
    for _ in range(num_pixels):
        pixel = (buf[src] << 8) | buf[src + 1]
        dst[d:d + 2] = np.array([pixel], np.uint16).view(np.uint8)  # *((uint16_t*)dst) = pixel
        src += 2
        d += 2


def _scanline_16_swap(buf, src, dst, d, num_pixels, pal):  # A:91-104, the arm of a little-endian host
    for i in range(num_pixels):
        dst[d + 2 * i] = buf[src + 2 * i + 1]
        dst[d + 2 * i + 1] = buf[src + 2 * i]


def _memcpy(bpp):  # Q:137-143, A:76-89 (the arm of a little-endian host), :108-118
    def scanline(buf, src, dst, d, num_pixels, pal):
        n = num_pixels * bpp
        dst[d:d + n] = buf[src:src + n]
    return scanline


def _scanline_raw_32(buf, src, dst, d, num_pixels, pal):  # Q:145-160
    for _ in range(num_pixels):
        dst[d] = buf[src + 1]
        dst[d + 1] = buf[src + 2]
        dst[d + 2] = buf[src + 3]
        dst[d + 3] = buf[src]
        d += 4
        src += 4


_SCANLINE = {"QT1": _scanline_sub_byte(1), "QT2": _scanline_sub_byte(2), "QT4": _scanline_sub_byte(4), "QT8": _scanline_8,
             "QT16": _scanline_raw_16, "QT24": _memcpy(3), "QT32": _scanline_raw_32, "AVI8": _scanline_8,
             "AVI8_GRAY": _scanline_8_gray, "AVI16": _memcpy(2), "MTV16": _scanline_16_swap, "AVI24": _memcpy(3),
             "AVI32": _memcpy(4)}


def unpack_literal(codec, w, h, packet, palette=None):
    lay, packet, palette = _checked(codec, w, h, packet, palette)
    buf = [int(x) for x in packet]  # a copy: the sub-byte scanlines shift it away
    stride = w * lay.bytes_per_pixel  # f->strides[0] of a tight frame
    dst = np.zeros(lay.picture_bytes, np.uint8)
    scanline, src = _SCANLINE[codec], 0
    if not lay.bottom_up:  # decode_qtraw, Q:395-406
        d = 0
        for _ in range(h):
            scanline(buf, src, dst, d, w, palette)
            src += lay.packet_stride
            d += stride
    else:  # decode_aviraw, A:183-192
        d = (h - 1) * stride
        for _ in range(h):
            scanline(buf, src, dst, d, w, palette)
            src += lay.packet_stride
            d -= stride
    return dst
