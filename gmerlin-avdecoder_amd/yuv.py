"""ctypes view of include/mi_yuv.h (libmi_yuv.so, the uncompressed QuickTime YUV family of lib/video_yuv.c: yuv2, 2vuy, VYUY,
yv12, YV12, YVU9, v308, v408, v410, v210, yuv4).  No CPU path: without the library or a gfx950 device construction raises
MiYuvError with the library's own message; codec_of, layout_of and alpha_v408 are host-side and need no device."""
import collections
import contextlib
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
YUV2, TWOVUY, YV12_LOWER, YV12_UPPER, VYUY, YVU9, V308, V408, V410, V210, YUV4 = range(11)
CODECS = {"yuv2": YUV2, "2vuy": TWOVUY, "yv12": YV12_LOWER, "YV12": YV12_UPPER, "VYUY": VYUY, "YVU9": YVU9, "v308": V308,
          "v408": V408, "v410": V410, "v210": V210, "yuv4": YUV4}
OK, ERR_ARG, ERR_HIP, ERR_NOMEM, ERR_FORMAT = 0, -1, -2, -3, -4
EXPORTS = ["mi_yuv_device_count", "mi_yuv_create", "mi_yuv_destroy", "mi_yuv_last_error", "mi_yuv_dev_alloc", "mi_yuv_dev_free",
           "mi_yuv_h2d", "mi_yuv_d2h", "mi_yuv_sync", "mi_yuv_codec_of", "mi_yuv_layout_of", "mi_yuv_alpha_v408",
           "mi_yuv_unpack_batch", "mi_yuv_unpack_frame", "mi_yuv_times"]
_LIB = None
u8p = C.POINTER(C.c_uint8)


class MiYuvError(RuntimeError):
    def __init__(self, message, code=ERR_ARG):
        super().__init__(message)
        self.code = code


class _Layout(C.Structure):
    _fields_ = [("packet_bytes", C.c_int64), ("picture_bytes", C.c_int64), ("packet_strides", C.c_int32 * 3),
                ("planes", C.c_int32), ("plane_w", C.c_int32 * 3), ("plane_h", C.c_int32 * 3), ("plane_bps", C.c_int32 * 3)]


# packet_strides: the packet's row stride(s) in bytes; planes: (width in samples, height, bytes per sample) in picture order
Layout = collections.namedtuple("Layout", "packet_bytes picture_bytes packet_strides planes")


def lib_path():
    return os.environ.get("MI_YUV_LIB") or os.path.join(HERE, "lib", "libmi_yuv.so")


def load():
    global _LIB
    if _LIB is not None:
        return _LIB
    p = lib_path()
    if not os.path.exists(p):
        raise MiYuvError(f"{p} is missing: run `python gmerlin-avdecoder_amd/build.py` (there is no CPU path)")
    L = C.CDLL(p)
    vp = C.c_void_p
    L.mi_yuv_device_count.restype = C.c_int
    L.mi_yuv_create.argtypes = [C.c_int]
    L.mi_yuv_create.restype = vp
    L.mi_yuv_destroy.argtypes = [vp]
    L.mi_yuv_destroy.restype = None
    L.mi_yuv_last_error.argtypes = [vp]
    L.mi_yuv_last_error.restype = C.c_char_p
    L.mi_yuv_dev_alloc.argtypes = [vp, C.c_size_t]
    L.mi_yuv_dev_alloc.restype = vp
    L.mi_yuv_dev_free.argtypes = [vp, vp]
    L.mi_yuv_dev_free.restype = None
    L.mi_yuv_h2d.argtypes = [vp, vp, vp, C.c_size_t]
    L.mi_yuv_d2h.argtypes = [vp, vp, vp, C.c_size_t]
    L.mi_yuv_sync.argtypes = [vp]
    L.mi_yuv_codec_of.argtypes = [C.c_uint32]
    L.mi_yuv_layout_of.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(_Layout)]
    L.mi_yuv_alpha_v408.argtypes = [u8p]
    L.mi_yuv_unpack_batch.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, C.c_int, vp, C.c_size_t]
    L.mi_yuv_unpack_frame.argtypes = [vp, C.c_int, C.c_int, C.c_int, u8p, C.c_size_t, C.POINTER(u8p), C.POINTER(C.c_int)]
    L.mi_yuv_times.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    _LIB = L
    return L


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


class MiYuv:
    def __init__(self, device=-1):
        self.L = load()
        self.c = self.L.mi_yuv_create(device)
        if not self.c:
            raise MiYuvError(self.L.mi_yuv_last_error(None).decode(), ERR_HIP)

    def _chk(self, rc):
        if rc != 0:
            raise MiYuvError(self.L.mi_yuv_last_error(self.c).decode(), rc)

    def alloc(self, n):
        d = self.L.mi_yuv_dev_alloc(self.c, n)
        if not d:
            raise MiYuvError(self.L.mi_yuv_last_error(self.c).decode(), ERR_NOMEM)
        return d

    def free(self, d):
        self.L.mi_yuv_dev_free(self.c, d)

    def h2d(self, d, a, offset=0):
        a = np.ascontiguousarray(a)
        self._chk(self.L.mi_yuv_h2d(self.c, d + offset, a.ctypes.data, a.nbytes))

    def d2h(self, d, n, offset=0):
        a = np.empty(n, np.uint8)
        self._chk(self.L.mi_yuv_d2h(self.c, a.ctypes.data, d + offset, n))
        return a

    def sync(self):
        self._chk(self.L.mi_yuv_sync(self.c))

    @contextlib.contextmanager
    def _resident(self, *what):
        """device buffers for the length of a with block: an array is uploaded, an int is a size in bytes"""
        ds = []
        try:
            for a in what:
                ds.append(self.alloc(a if isinstance(a, int) else a.nbytes))
                if isinstance(a, np.ndarray):
                    self.h2d(ds[-1], a)
            yield ds
        finally:
            for d in ds:
                self.free(d)

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
        ms, n = C.c_float(), C.c_int()
        self._chk(self.L.mi_yuv_times(self.c, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def close(self):
        if self.c:
            self.L.mi_yuv_destroy(self.c)
            self.c = None
