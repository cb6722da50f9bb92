"""ctypes view of include/mi_yuv.h (libmi_yuv.so, the uncompressed QuickTime YUV family of lib/video_yuv.c: yuv2, 2vuy, VYUY,
yv12, YV12, YVU9, v308, v408, v410, v210, yuv4).  No CPU path: without the library or a gfx950 device construction raises
MiYuvError with the library's own message; codec_of, layout_of and alpha_v408 are host-side and need no device."""
import collections
import ctypes as C

import numpy as np

from ._capi import Device, Library, cint, f32p, intp, sz, u8p, u8pp, u32, vp

YUV2, TWOVUY, YV12_LOWER, YV12_UPPER, VYUY, YVU9, V308, V408, V410, V210, YUV4 = range(11)
CODECS = {"yuv2": YUV2, "2vuy": TWOVUY, "yv12": YV12_LOWER, "YV12": YV12_UPPER, "VYUY": VYUY, "YVU9": YVU9, "v308": V308,
          "v408": V408, "v410": V410, "v210": V210, "yuv4": YUV4}
OK, ERR_ARG, ERR_HIP, ERR_NOMEM, ERR_FORMAT = 0, -1, -2, -3, -4


class MiYuvError(RuntimeError):
    def __init__(self, message, code=ERR_ARG):
        super().__init__(message)
        self.code = code


class _Layout(C.Structure):
    _fields_ = [("packet_bytes", C.c_int64), ("picture_bytes", C.c_int64), ("packet_strides", C.c_int32 * 3),
                ("planes", C.c_int32), ("plane_w", C.c_int32 * 3), ("plane_h", C.c_int32 * 3), ("plane_bps", C.c_int32 * 3)]


# packet_strides: the packet's row stride(s) in bytes; planes: (width in samples, height, bytes per sample) in picture order
Layout = collections.namedtuple("Layout", "packet_bytes picture_bytes packet_strides planes")


# every function of include/mi_yuv.h, in its order: (what it returns, what it takes)
SIGNATURES = {
    "mi_yuv_device_count": (cint, []),
    "mi_yuv_create": (vp, [cint]),
    "mi_yuv_destroy": (None, [vp]),
    "mi_yuv_last_error": (C.c_char_p, [vp]),
    "mi_yuv_dev_alloc": (vp, [vp, sz]),
    "mi_yuv_dev_free": (None, [vp, vp]),
    "mi_yuv_h2d": (cint, [vp, vp, vp, sz]),
    "mi_yuv_d2h": (cint, [vp, vp, vp, sz]),
    "mi_yuv_sync": (cint, [vp]),
    "mi_yuv_codec_of": (cint, [u32]),
    "mi_yuv_layout_of": (cint, [cint, cint, cint, C.POINTER(_Layout)]),
    "mi_yuv_alpha_v408": (cint, [u8p]),
    "mi_yuv_unpack_batch": (cint, [vp, cint, cint, cint, vp, sz, cint, vp, sz]),
    "mi_yuv_unpack_frame": (cint, [vp, cint, cint, cint, u8p, sz, u8pp, intp]),
    "mi_yuv_times": (cint, [vp, f32p, intp]),
}
EXPORTS = list(SIGNATURES)
LIB = Library("libmi_yuv.so", "MI_YUV_LIB", "mi_yuv_", MiYuvError, SIGNATURES)
lib_path, load = LIB.path, LIB.load


def codec_of(fourcc):
    """the codec of a fourcc, given as four characters or as BGAV_MK_FOURCC's integer; -1 for any other (host-side)"""
    if isinstance(fourcc, (str, bytes)):
        b = fourcc.encode("latin-1") if isinstance(fourcc, str) else fourcc
        if len(b) != 4:
            return -1
        fourcc = int.from_bytes(b, "big")
    return load().mi_yuv_codec_of(fourcc)


def _codec(codec):
    return CODECS[codec] if isinstance(codec, str) else codec


def layout_of(codec, w, h):
    """the Layout of a codec (a number, or one of CODECS' names) at a size; MiYuvError names the rule a size breaks
    (host-side)"""
    L, v = load(), _Layout()
    rc = L.mi_yuv_layout_of(_codec(codec), w, h, C.byref(v))
    if rc != 0:
        raise MiYuvError(L.mi_yuv_last_error(None).decode(), rc)
    return Layout(v.packet_bytes, v.picture_bytes, tuple(v.packet_strides),
                  tuple((v.plane_w[p], v.plane_h[p], v.plane_bps[p]) for p in range(v.planes)))


def alpha_v408():
    """v408's alpha for 0..255 (host-side)"""
    a = np.zeros(256, np.uint8)
    if load().mi_yuv_alpha_v408(a.ctypes.data_as(u8p)) != 0:
        raise MiYuvError(load().mi_yuv_last_error(None).decode())
    return a


def up16(n):
    return (n + 15) // 16 * 16


class MiYuv(Device):
    LIB = LIB

    def _error(self, text, rc, what):
        return MiYuvError(text, {"create": ERR_HIP, "alloc": ERR_NOMEM}.get(what, rc))

    def unpack_batch(self, codec, w, h, d_packets, packet_stride, n, d_pics, pic_stride):
        """packet i at d_packets + i * packet_stride -> picture i at d_pics + i * pic_stride, one launch queued on the
        instance's stream (bases and strides 16-byte aligned, strides at least the layout's sizes)"""
        self._chk(self.L.mi_yuv_unpack_batch(self.c, _codec(codec), w, h, d_packets, packet_stride, n, d_pics, pic_stride))

    def unpack_packets(self, codec, w, h, packets):
        """host packets (n x the layout's packet bytes, uint8) -> host pictures (n x its picture bytes), through the batch
        path"""
        lay = layout_of(codec, w, h)
        packets = np.ascontiguousarray(packets, np.uint8).reshape(-1, lay.packet_bytes)
        n, ps, qs = packets.shape[0], up16(lay.packet_bytes), up16(lay.picture_bytes)
        slots = np.zeros((n, ps), np.uint8)
        slots[:, :lay.packet_bytes] = packets
        with self._resident(slots, n * qs) as (dp, dq):
            self.unpack_batch(codec, w, h, dp, ps, n, dq, qs)
            self.sync()
            return self.d2h(dq, n * qs).reshape(n, qs)[:, :lay.picture_bytes].copy()

    def unpack_frame(self, codec, w, h, packet, strides=None, planes=None):
        """one host packet into the picture's planes at the given strides in bytes (default: the planes' rows; planes None:
        zeros) -> the planes, each a uint8 array of stride x height"""
        lay = layout_of(codec, w, h)
        packet = np.ascontiguousarray(packet, np.uint8)
        if strides is None:
            strides = [pw * bps for pw, _, bps in lay.planes]
        if planes is None:
            planes = [np.zeros(strides[i] * ph, np.uint8) for i, (_, ph, _) in enumerate(lay.planes)]
        pp = (u8p * 3)(*[p.ctypes.data_as(u8p) for p in planes])
        st = (C.c_int * 3)(*strides)
        self._chk(self.L.mi_yuv_unpack_frame(self.c, _codec(codec), w, h, packet.ctypes.data_as(u8p), packet.nbytes, pp, st))
        return planes

    def times(self):
        """(total milliseconds, launches) of the unpack kernels since the last call"""
        return self._times(self.L.mi_yuv_times)
