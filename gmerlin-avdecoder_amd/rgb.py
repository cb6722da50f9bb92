"""ctypes view of include/mi_rgb.h (libmi_rgb.so, the raw RGB family of QuickTime and AVI: 'raw ' of lib/video_qtraw.c and
'RGB ', 'RGB3', 'MTV ' of lib/video_aviraw.c).  No CPU path: without the library or a gfx950 device construction raises
MiRgbError with the library's own message; codec_of and layout_of are host-side and need no device.

Palettes are numpy uint16 arrays of shape (n_palettes, entries, 4): r, g, b, a of 16 bits each, as upstream's palette
entries; a single palette may be given as (entries, 4)."""
import collections
import ctypes as C

import numpy as np

from ._capi import Device, Library, cint, f32p, intp, sz, u8p, u32, vp

QT1, QT2, QT4, QT8, QT16, QT24, QT32, AVI8, AVI8_GRAY, AVI16, MTV16, AVI24, AVI32 = range(13)
CODECS = {"QT1": QT1, "QT2": QT2, "QT4": QT4, "QT8": QT8, "QT16": QT16, "QT24": QT24, "QT32": QT32, "AVI8": AVI8,
          "AVI8_GRAY": AVI8_GRAY, "AVI16": AVI16, "MTV16": MTV16, "AVI24": AVI24, "AVI32": AVI32}
OK, ERR_ARG, ERR_HIP, ERR_NOMEM, ERR_FORMAT = 0, -1, -2, -3, -4
u16p = C.POINTER(C.c_uint16)


class MiRgbError(RuntimeError):
    def __init__(self, message, code=ERR_ARG):
        super().__init__(message)
        self.code = code


class _Layout(C.Structure):
    _fields_ = [("packet_bytes", C.c_int64), ("picture_bytes", C.c_int64), ("packet_stride", C.c_int32),
                ("bytes_per_pixel", C.c_int32), ("palette_entries", C.c_int32), ("bottom_up", C.c_int32)]


# packet_stride: bytes between the packet's rows; palette_entries: 0 where the codec has none; bottom_up: packet row i is
# picture row h - 1 - i
Layout = collections.namedtuple("Layout", "packet_bytes picture_bytes packet_stride bytes_per_pixel palette_entries bottom_up")


# every function of include/mi_rgb.h, in its order: (what it returns, what it takes)
SIGNATURES = {
    "mi_rgb_device_count": (cint, []),
    "mi_rgb_create": (vp, [cint]),
    "mi_rgb_destroy": (None, [vp]),
    "mi_rgb_last_error": (C.c_char_p, [vp]),
    "mi_rgb_dev_alloc": (vp, [vp, sz]),
    "mi_rgb_dev_free": (None, [vp, vp]),
    "mi_rgb_h2d": (cint, [vp, vp, vp, sz]),
    "mi_rgb_d2h": (cint, [vp, vp, vp, sz]),
    "mi_rgb_sync": (cint, [vp]),
    "mi_rgb_codec_of": (cint, [u32, cint, cint]),
    "mi_rgb_layout_of": (cint, [cint, cint, cint, C.POINTER(_Layout)]),
    "mi_rgb_unpack_batch": (cint, [vp, cint, cint, cint, vp, sz, cint, vp, sz, vp, cint, u16p]),
    "mi_rgb_unpack_frame": (cint, [vp, cint, cint, cint, u8p, sz, vp, u8p, cint]),
    "mi_rgb_times": (cint, [vp, f32p, intp]),
}
EXPORTS = list(SIGNATURES)
LIB = Library("libmi_rgb.so", "MI_RGB_LIB", "mi_rgb_", MiRgbError, SIGNATURES)
lib_path, load = LIB.path, LIB.load


def codec_of(fourcc, depth, has_palette):
    """the codec of a stream: its fourcc (four characters, or BGAV_MK_FOURCC's integer), depth, and whether it has a
    palette; -1 for anything upstream's init refuses (host-side)"""
    if isinstance(fourcc, (str, bytes)):
        b = fourcc.encode("latin-1") if isinstance(fourcc, str) else fourcc
        if len(b) != 4:
            return -1
        fourcc = int.from_bytes(b, "big")
    return load().mi_rgb_codec_of(fourcc, depth, 1 if has_palette else 0)


def _codec(codec):
    return CODECS[codec] if isinstance(codec, str) else codec


def layout_of(codec, w, h):
    """the Layout of a codec (a number, or one of CODECS' names) at a size; MiRgbError names the rule a size breaks
    (host-side)"""
    L, v = load(), _Layout()
    rc = L.mi_rgb_layout_of(_codec(codec), w, h, C.byref(v))
    if rc != 0:
        raise MiRgbError(L.mi_rgb_last_error(None).decode(), rc)
    return Layout(v.packet_bytes, v.picture_bytes, v.packet_stride, v.bytes_per_pixel, v.palette_entries, bool(v.bottom_up))


def up16(n):
    return (n + 15) // 16 * 16


def _palettes(codec, w, h, palettes):
    """the palettes as a contiguous (n, entries, 4) uint16 array for a codec with a palette, None for None; a palette
    shorter than the codec's entries is refused here: the C interface takes a pointer and reads the codec's count"""
    if palettes is None:
        return None
    entries = layout_of(codec, w, h).palette_entries
    a = np.ascontiguousarray(palettes, np.uint16)
    if a.ndim == 2:
        a = a[None]
    if entries and (a.ndim != 3 or a.shape[2] != 4 or a.shape[1] < entries or a.shape[0] < 1):
        raise MiRgbError(f"palettes of shape {a.shape}: (n_palettes, {entries}, 4) for this codec; a shorter palette is refused")
    return np.ascontiguousarray(a[:, :entries]) if entries else a


class MiRgb(Device):
    LIB = LIB

    def _error(self, text, rc, what):
        return MiRgbError(text, {"create": ERR_HIP, "alloc": ERR_NOMEM}.get(what, rc))

    def unpack_batch(self, codec, w, h, d_packets, packet_stride, n, d_pics, pic_stride, palettes=None, palette_of=None):
        """packet i at d_packets + i * packet_stride -> picture i at d_pics + i * pic_stride, one launch queued on the
        instance's stream (bases and strides 16-byte aligned, strides at least the layout's sizes).  palettes: (n_palettes,
        entries, 4) uint16 for the palettised codecs; palette_of: n indices into them, or None: every packet uses palette
        0.  The library has its own copy of both when this returns."""
        pal = _palettes(codec, w, h, palettes)
        of = None if palette_of is None else np.ascontiguousarray(palette_of, np.uint16)
        if of is not None and of.size != n:
            raise MiRgbError(f"palette_of has {of.size} indices for {n} packets")
        self._chk(self.L.mi_rgb_unpack_batch(self.c, _codec(codec), w, h, d_packets, packet_stride, n, d_pics, pic_stride,
                                             None if pal is None else pal.ctypes.data, 0 if pal is None else pal.shape[0],
                                             None if of is None else of.ctypes.data_as(u16p)))

    def unpack_packets(self, codec, w, h, packets, palettes=None, palette_of=None):
        """host packets (n x the layout's packet bytes, uint8) -> host pictures (n x its picture bytes), through the batch
        path"""
        lay = layout_of(codec, w, h)
        packets = np.ascontiguousarray(packets, np.uint8).reshape(-1, lay.packet_bytes)
        n, ps, qs = packets.shape[0], up16(lay.packet_bytes), up16(lay.picture_bytes)
        slots = np.zeros((n, ps), np.uint8)
        slots[:, :lay.packet_bytes] = packets
        with self._resident(slots, n * qs) as (dp, dq):
            self.unpack_batch(codec, w, h, dp, ps, n, dq, qs, palettes, palette_of)
            self.sync()
            return self.d2h(dq, n * qs).reshape(n, qs)[:, :lay.picture_bytes].copy()

    def unpack_frame(self, codec, w, h, packet, palette=None, stride=None, plane=None):
        """one host packet into the picture's plane, top row first, at the given stride in bytes (default: the picture's
        row; plane None: zeros) -> the plane, a uint8 array of stride x height"""
        lay = layout_of(codec, w, h)
        packet = np.ascontiguousarray(packet, np.uint8)
        pal = _palettes(codec, w, h, palette)
        if pal is not None and pal.shape[0] != 1:
            raise MiRgbError(f"{pal.shape[0]} palettes for one packet")
        if stride is None:
            stride = w * lay.bytes_per_pixel
        if plane is None:
            plane = np.zeros(stride * h, np.uint8)
        self._chk(self.L.mi_rgb_unpack_frame(self.c, _codec(codec), w, h, packet.ctypes.data_as(u8p), packet.nbytes,
                                             None if pal is None else pal.ctypes.data, plane.ctypes.data_as(u8p), stride))
        return plane

    def times(self):
        """(total milliseconds, launches) of the unpack kernels since the last call"""
        return self._times(self.L.mi_rgb_times)
