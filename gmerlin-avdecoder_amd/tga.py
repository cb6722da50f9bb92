"""ctypes view of include/mi_tga.h (libmi_tga.so, Targa packets of fourcc 'tga ', run-length included: lib/video_tga.c over
lib/targa.c).  No CPU path: without the library or a gfx950 device construction raises MiTgaError with the library's own
message; parse and tile_pixels are host-side and need no device.

Palettes are numpy uint16 arrays of shape (n_palettes, entries, 4): r, g, b, a of 16 bits each, as upstream's palette
entries; a single palette may be given as (entries, 4)."""
import collections
import ctypes as C

import numpy as np

from ._capi import Device, Library, cint, f32p, intp, sz, u8p, u32p, u64p, vp

GRAY8, RGB15, BGR24, RGBA32 = range(4)
FORMATS = {"GRAY8": GRAY8, "RGB15": RGB15, "BGR24": BGR24, "RGBA32": RGBA32}
OK, ERR_ARG, ERR_HIP, ERR_NOMEM, ERR_FORMAT = 0, -1, -2, -3, -4
ST_OK, ST_EOF, ST_CMAP_TYPE, ST_IMG_TYPE, ST_NO_IMG, ST_CMAP_MISSING = 0, 2, 4, 5, 6, 7
ST_CMAP_LENGTH, ST_CMAP_DEPTH, ST_ZERO_SIZE, ST_PIXEL_DEPTH, ST_RLE, ST_INDEX_RANGE = 9, 10, 11, 12, 15, 16
ST_SHORT, ST_BELOW_ORIGIN, ST_MISMATCH = 32, 33, 34
u16p, i32p = C.POINTER(C.c_uint16), C.POINTER(C.c_int32)


class MiTgaError(RuntimeError):
    def __init__(self, message, code=ERR_ARG, status=None):
        super().__init__(message)
        self.code, self.status = code, status


class _Info(C.Structure):
    _fields_ = [("status", C.c_int32), ("data_offset", C.c_uint32), ("map_offset", C.c_uint32),
                ("map_origin", C.c_uint16), ("map_length", C.c_uint16), ("x_origin", C.c_uint16), ("y_origin", C.c_uint16),
                ("width", C.c_uint16), ("height", C.c_uint16),
                ("id_length", C.c_uint8), ("map_type", C.c_uint8), ("image_type", C.c_uint8), ("map_depth", C.c_uint8),
                ("pixel_depth", C.c_uint8), ("descriptor", C.c_uint8),
                ("format", C.c_uint8), ("bytes_per_pixel", C.c_uint8),
                ("rle", C.c_uint8), ("mapped", C.c_uint8), ("flip_x", C.c_uint8), ("flip_y", C.c_uint8), ("from_palette", C.c_uint8),
                ("reserved", C.c_uint8 * 3)]


# the fields of mi_tga_info but `reserved`, in its order
Info = collections.namedtuple("Info", [n for n, _ in _Info._fields_[:-1]])


def _info(v):
    return Info(*(getattr(v, n) for n in Info._fields))


# every function of include/mi_tga.h, in its order: (what it returns, what it takes)
SIGNATURES = {
    "mi_tga_device_count": (cint, []),
    "mi_tga_create": (vp, [cint]),
    "mi_tga_destroy": (None, [vp]),
    "mi_tga_last_error": (C.c_char_p, [vp]),
    "mi_tga_dev_alloc": (vp, [vp, sz]),
    "mi_tga_dev_free": (None, [vp, vp]),
    "mi_tga_h2d": (cint, [vp, vp, vp, sz]),
    "mi_tga_d2h": (cint, [vp, vp, vp, sz]),
    "mi_tga_sync": (cint, [vp]),
    "mi_tga_parse": (cint, [u8p, sz, cint, C.POINTER(_Info)]),
    "mi_tga_tile_pixels": (cint, []),
    "mi_tga_decode_batch": (cint, [vp, vp, u64p, u32p, cint, cint, cint, cint, vp, sz, vp, cint, cint, u16p, vp]),
    "mi_tga_decode_frame": (cint, [vp, u8p, sz, vp, cint, u8p, cint, C.POINTER(_Info)]),
    "mi_tga_times": (cint, [vp, f32p, intp]),
}
EXPORTS = list(SIGNATURES)
LIB = Library("libmi_tga.so", "MI_TGA_LIB", "mi_tga_", MiTgaError, SIGNATURES)
lib_path, load = LIB.path, LIB.load


def parse(packet, palette_entries=0):
    """the Info of a packet's header (host-side); Info.status is 0 or the code of the first check that fails"""
    packet = np.ascontiguousarray(packet, np.uint8)
    v = _Info()
    rc = load().mi_tga_parse(packet.ctypes.data_as(u8p), packet.nbytes, palette_entries, C.byref(v))
    if rc < 0:
        raise MiTgaError(load().mi_tga_last_error(None).decode(), rc)
    return _info(v)


def tile_pixels():
    """the expansion tile: stored pixels a checkpoint of the index (host-side)"""
    return load().mi_tga_tile_pixels()


def up16(n):
    return (n + 15) // 16 * 16


def _palettes(palettes):
    """(the palettes as a contiguous (n, entries, 4) uint16 array, entries), or (None, 0)"""
    if palettes is None:
        return None, 0
    a = np.ascontiguousarray(palettes, np.uint16)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[2] != 4 or a.shape[0] < 1 or a.shape[1] < 1:
        raise MiTgaError(f"palettes of shape {a.shape}: (n_palettes, entries, 4)")
    return a, a.shape[1]


class MiTga(Device):
    LIB = LIB

    def _error(self, text, rc, what):
        return MiTgaError(text, {"create": ERR_HIP, "alloc": ERR_NOMEM}.get(what, rc))

    parse = staticmethod(parse)
    tile_pixels = staticmethod(tile_pixels)

    def decode_batch(self, d_stream, offsets, lengths, w, h, fmt, d_pics, pic_stride, d_status, palettes=None, palette_of=None):
        """packet i, lengths[i] bytes at d_stream + offsets[i] -> picture i at d_pics + i * pic_stride and its status at
        d_status + 4 i; three launches queued on the instance's stream.  palettes: (n_palettes, entries, 4) uint16 or
        None; palette_of: n indices into them, or None: every packet uses palette 0.  The library has its own copy of
        offsets, lengths and both when this returns."""
        offsets, lengths = np.ascontiguousarray(offsets, np.uint64), np.ascontiguousarray(lengths, np.uint32)
        n = offsets.size
        if lengths.size != n:
            raise MiTgaError(f"{lengths.size} lengths for {n} offsets")
        pal, entries = _palettes(palettes)
        of = None if palette_of is None else np.ascontiguousarray(palette_of, np.uint16)
        if of is not None and of.size != n:
            raise MiTgaError(f"palette_of has {of.size} indices for {n} packets")
        self._chk(self.L.mi_tga_decode_batch(self.c, d_stream, offsets.ctypes.data_as(u64p), lengths.ctypes.data_as(u32p), n, w, h,
                                             FORMATS[fmt] if isinstance(fmt, str) else fmt, d_pics, pic_stride,
                                             None if pal is None else pal.ctypes.data, entries, 0 if pal is None else pal.shape[0],
                                             None if of is None else of.ctypes.data_as(u16p), d_status))

    def decode_packets(self, packets, w, h, fmt, palettes=None, palette_of=None):
        """a host list of packets (uint8 arrays or bytes) -> (pictures: n x picture bytes, uint8; statuses: n int32),
        through the batch path; the picture of a packet whose status is not 0 is zeros where nothing was written"""
        packets = [np.frombuffer(bytes(p), np.uint8) if isinstance(p, (bytes, bytearray)) else np.ascontiguousarray(p, np.uint8)
                   for p in packets]
        n = len(packets)
        lengths = np.array([p.size for p in packets], np.uint32)
        offsets = np.concatenate([[0], np.cumsum(lengths[:-1], dtype=np.uint64)]).astype(np.uint64)
        stream = np.concatenate(packets + [np.zeros(1, np.uint8)])
        size = w * h * ((FORMATS[fmt] if isinstance(fmt, str) else fmt) + 1)
        qs = up16(size)
        with self._resident(stream, np.zeros(n * qs, np.uint8), 4 * n) as (ds, dq, dst):
            self.decode_batch(ds, offsets, lengths, w, h, fmt, dq, qs, dst, palettes, palette_of)
            self.sync()
            return self.d2h(dq, n * qs).reshape(n, qs)[:, :size].copy(), self.d2h(dst, 4 * n, dtype=np.int32)

    def decode_frame(self, packet, palette=None, stride=None, plane=None):
        """one host packet into a plane, top row first, at the given stride in bytes (default: the picture's row; plane
        None: zeros) -> (the plane, a uint8 array of stride x height, and the packet's Info).  A bad packet raises
        MiTgaError with code ERR_FORMAT and the status in .status."""
        packet = np.ascontiguousarray(packet, np.uint8)
        pal, entries = _palettes(palette)
        if pal is not None and pal.shape[0] != 1:
            raise MiTgaError(f"{pal.shape[0]} palettes for one packet")
        head = parse(packet, entries)
        if head.status == 0:
            if stride is None:
                stride = head.width * head.bytes_per_pixel
            if plane is None:
                plane = np.zeros(stride * head.height, np.uint8)
        elif plane is None:
            plane, stride = np.zeros(1, np.uint8), stride or 0
        v = _Info()
        rc = self.L.mi_tga_decode_frame(self.c, packet.ctypes.data_as(u8p), packet.nbytes, None if pal is None else pal.ctypes.data,
                                        entries, plane.ctypes.data_as(u8p), stride, C.byref(v))
        if rc != 0:
            raise MiTgaError(self.last_error(), rc, v.status if rc == ERR_FORMAT else None)
        return plane, _info(v)

    def times(self):
        """((scan, index, expand) milliseconds, launches) of the kernels since the last call"""
        ms, n = (C.c_float * 3)(), C.c_int()
        self._chk(self.L.mi_tga_times(self.c, ms, C.byref(n)))
        return tuple(ms), n.value
