"""ctypes view of include/mi_spu.h (libmi_spu.so, DVD subpictures of fourcc 'DVDS': lib/subovl_dvd.c).  No CPU path: without
the library or a gfx950 device construction raises MiSpuError with the library's own message; parse is host-side and needs
no device.

A palette is the disc's: 16 uint32 as the IFO file holds them; palettes are numpy uint32 arrays of shape (n_palettes, 16), a
single one may be given as (16,).  A picture is w x h x 4 bytes, GAVL_YUVA_32."""
import collections
import ctypes as C

import numpy as np

from ._capi import Device, Library, cint, f32p, intp, sz, u8p, u32p, u64p, vp

OK, ERR_ARG, ERR_HIP, ERR_NOMEM, ERR_FORMAT = 0, -1, -2, -3, -4
ST_OK, ST_SHORT, ST_CTRL_RANGE, ST_RECT, ST_DATA_RANGE = range(5)
u16p = C.POINTER(C.c_uint16)


class MiSpuError(RuntimeError):
    def __init__(self, message, code=ERR_ARG, status=None):
        super().__init__(message)
        self.code, self.status = code, status


class _Info(C.Structure):
    _fields_ = [("status", C.c_int32), ("src_w", C.c_int32), ("src_h", C.c_int32), ("dst_x", C.c_int32), ("dst_y", C.c_int32),
                ("lines1", C.c_int32), ("lines2", C.c_int32),
                ("ctrl_start", C.c_uint16), ("offset1", C.c_uint16), ("offset2", C.c_uint16), ("x1", C.c_uint16), ("x2", C.c_uint16),
                ("y1", C.c_uint16), ("y2", C.c_uint16), ("sequences", C.c_uint16),
                ("palette", C.c_uint8 * 4), ("alpha", C.c_uint8 * 4), ("ctrl_end", C.c_uint32)]


INFO_BYTES = C.sizeof(_Info)
# the fields of mi_spu_info, in its order; palette and alpha as tuples of four
Info = collections.namedtuple("Info", [n for n, _ in _Info._fields_])


def _info(v):
    return Info(*(tuple(getattr(v, n)) if n in ("palette", "alpha") else getattr(v, n) for n in Info._fields))


# every function of include/mi_spu.h, in its order: (what it returns, what it takes)
SIGNATURES = {
    "mi_spu_device_count": (cint, []),
    "mi_spu_create": (vp, [cint]),
    "mi_spu_destroy": (None, [vp]),
    "mi_spu_last_error": (C.c_char_p, [vp]),
    "mi_spu_dev_alloc": (vp, [vp, sz]),
    "mi_spu_dev_free": (None, [vp, vp]),
    "mi_spu_h2d": (cint, [vp, vp, vp, sz]),
    "mi_spu_d2h": (cint, [vp, vp, vp, sz]),
    "mi_spu_sync": (cint, [vp]),
    "mi_spu_parse": (cint, [u8p, sz, cint, cint, C.POINTER(_Info)]),
    "mi_spu_decode_batch": (cint, [vp, vp, u64p, u32p, cint, cint, cint, vp, sz, u32p, cint, u16p, vp]),
    "mi_spu_decode_frame": (cint, [vp, u8p, sz, cint, cint, u32p, u8p, cint, C.POINTER(_Info)]),
    "mi_spu_times": (cint, [vp, f32p, intp]),
}
EXPORTS = list(SIGNATURES)
LIB = Library("libmi_spu.so", "MI_SPU_LIB", "mi_spu_", MiSpuError, SIGNATURES)
lib_path, load = LIB.path, LIB.load


def parse(packet, w, h):
    """the Info of a packet's control section for a video of w x h (host-side); Info.status is 0, SHORT, CTRL_RANGE or RECT"""
    packet = np.ascontiguousarray(packet, np.uint8)
    v = _Info()
    rc = load().mi_spu_parse(packet.ctypes.data_as(u8p), packet.nbytes, w, h, C.byref(v))
    if rc < 0:
        raise MiSpuError(load().mi_spu_last_error(None).decode(), rc)
    return _info(v)


def up16(n):
    return (n + 15) // 16 * 16


def infos(raw):
    """the Infos in the bytes of n mi_spu_info structs"""
    raw = np.ascontiguousarray(raw, np.uint8)
    return [_info(_Info.from_buffer_copy(raw[k:k + INFO_BYTES].tobytes())) for k in range(0, raw.size, INFO_BYTES)]


def _palettes(palettes):
    a = np.ascontiguousarray(palettes, np.uint32)
    if a.ndim == 1:
        a = a[None]
    if a.ndim != 2 or a.shape[1] != 16 or a.shape[0] < 1:
        raise MiSpuError(f"palettes of shape {a.shape}: (n_palettes, 16)")
    return a


class MiSpu(Device):
    LIB = LIB

    def _error(self, text, rc, what):
        return MiSpuError(text, {"create": ERR_HIP, "alloc": ERR_NOMEM}.get(what, rc))

    parse = staticmethod(parse)

    def decode_batch(self, d_stream, offsets, lengths, w, h, d_pics, pic_stride, palettes, d_info, palette_of=None):
        """packet i, lengths[i] bytes at d_stream + offsets[i] -> picture i (w x h x 4 bytes, all of them written) at
        d_pics + i * pic_stride and its mi_spu_info at d_info + INFO_BYTES * i; two launches queued on the instance's
        stream.  palettes: (n_palettes, 16) uint32; palette_of: n indices into them, or None: every packet uses palette 0.
        The library has its own copy of offsets, lengths and both when this returns."""
        offsets, lengths = np.ascontiguousarray(offsets, np.uint64), np.ascontiguousarray(lengths, np.uint32)
        n = offsets.size
        if lengths.size != n:
            raise MiSpuError(f"{lengths.size} lengths for {n} offsets")
        pal = _palettes(palettes)
        of = None if palette_of is None else np.ascontiguousarray(palette_of, np.uint16)
        if of is not None and of.size != n:
            raise MiSpuError(f"palette_of has {of.size} indices for {n} packets")
        self._chk(self.L.mi_spu_decode_batch(self.c, d_stream, offsets.ctypes.data_as(u64p), lengths.ctypes.data_as(u32p), n, w, h,
                                             d_pics, pic_stride, pal.ctypes.data_as(u32p), pal.shape[0],
                                             None if of is None else of.ctypes.data_as(u16p), d_info))

    def decode_packets(self, packets, w, h, palettes, palette_of=None):
        """a host list of packets (uint8 arrays or bytes) -> (pictures: n x (w * h * 4) uint8; the n Infos), through the
        batch path; the picture of a packet whose status is not 0 is zeros where nothing was written"""
        packets = [np.frombuffer(bytes(p), np.uint8) if isinstance(p, (bytes, bytearray)) else np.ascontiguousarray(p, np.uint8)
                   for p in packets]
        n = len(packets)
        lengths = np.array([p.size for p in packets], np.uint32)
        offsets = np.concatenate([[0], np.cumsum(lengths[:-1], dtype=np.uint64)]).astype(np.uint64)
        stream = np.concatenate(packets + [np.zeros(1, np.uint8)])
        size = w * h * 4
        qs = up16(size)
        with self._resident(stream, np.zeros(n * qs, np.uint8), INFO_BYTES * n) as (ds, dq, di):
            self.decode_batch(ds, offsets, lengths, w, h, dq, qs, palettes, di, palette_of)
            self.sync()
            return self.d2h(dq, n * qs).reshape(n, qs)[:, :size].copy(), infos(self.d2h(di, INFO_BYTES * n))

    def decode_frame(self, packet, w, h, palette, stride=None, plane=None):
        """one host packet into a plane of h rows at the given stride in bytes (default: w * 4; plane None: zeros) -> (the
        plane, a uint8 array of stride x h, and the packet's Info).  A bad packet raises MiSpuError with code ERR_FORMAT
        and the status in .status."""
        packet = np.ascontiguousarray(packet, np.uint8)
        pal = _palettes(palette)
        if pal.shape[0] != 1:
            raise MiSpuError(f"{pal.shape[0]} palettes for one packet")
        if stride is None:
            stride = w * 4
        if plane is None:
            plane = np.zeros(max(stride * h, 1), np.uint8)
        v = _Info()
        rc = self.L.mi_spu_decode_frame(self.c, packet.ctypes.data_as(u8p), packet.nbytes, w, h, pal.ctypes.data_as(u32p),
                                        plane.ctypes.data_as(u8p), stride, C.byref(v))
        if rc != 0:
            raise MiSpuError(self.last_error(), rc, v.status if rc == ERR_FORMAT else None)
        return plane, _info(v)

    def times(self):
        """((scan, decode) milliseconds, launches) of the kernels since the last call"""
        ms, n = (C.c_float * 2)(), C.c_int()
        self._chk(self.L.mi_spu_times(self.c, ms, C.byref(n)))
        return tuple(ms), n.value
