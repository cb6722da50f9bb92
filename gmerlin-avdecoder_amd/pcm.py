"""ctypes view of include/mi_pcm.h (libmi_pcm.so, the PCM family of lib/audio_pcm.c: integers of both byte orders, the DVD
LPCM group packings, floats and doubles through libsndfile's portable readers, u-law and A-law).  No CPU path: without the
library or a gfx950 device construction raises MiPcmError with the library's own message; codec_of, layout_of and
payload_of are host-side and need no device."""
import ctypes as C

import numpy as np

from ._capi import Device, Library, cint, f32p, i64, intp, sz, u8p, u32, u32p, u64, u64p, vp

OK, ERR_ARG, ERR_HIP, ERR_NOMEM = 0, -1, -2, -3
CODECS = ("COPY8", "COPY16", "SWAP16", "S24LE", "S24BE", "LPCM24", "LPCM24_MONO", "LPCM20", "LPCM20_MONO", "COPY32", "SWAP32",
          "F32LE", "F32BE", "F64LE", "F64BE", "ULAW", "ALAW")
LABELS = ("U8", "S8", "U16", "S16", "S32", "FLOAT", "DOUBLE")
SAMPLE_BYTES = (1, 2, 2, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 8, 8, 2, 2)
FRAME_SAMPLES, MAX_PACKETS, MAX_CHANNELS, TILE_BYTES = 1024, 1 << 20, 128, 16384
ENDIANESS_NONE, ENDIANESS_BIG, ENDIANESS_LITTLE = 0, 1, 2


class Format(C.Structure):
    _fields_ = [("codec", C.c_int32), ("label", C.c_int32), ("block_align", C.c_int32), ("sample_bytes", C.c_int32)]


class Layout(C.Structure):
    _fields_ = [("frames", C.c_uint64), ("written", C.c_uint64), ("consumed", C.c_uint64), ("out_bytes", C.c_uint64)]


class MiPcmError(RuntimeError):
    def __init__(self, message, code=ERR_ARG):
        super().__init__(message)
        self.code = code


# every function of include/mi_pcm.h, in its order: (what it returns, what it takes)
SIGNATURES = {
    "mi_pcm_device_count": (cint, []),
    "mi_pcm_create": (vp, [cint]),
    "mi_pcm_destroy": (None, [vp]),
    "mi_pcm_last_error": (C.c_char_p, [vp]),
    "mi_pcm_dev_alloc": (vp, [vp, sz]),
    "mi_pcm_dev_free": (None, [vp, vp]),
    "mi_pcm_h2d": (cint, [vp, vp, vp, sz]),
    "mi_pcm_d2h": (cint, [vp, vp, vp, sz]),
    "mi_pcm_sync": (cint, [vp]),
    "mi_pcm_codec_of": (cint, [u32, cint, cint, cint, u8p, cint, C.POINTER(Format)]),
    "mi_pcm_payload_of": (i64, [i64, i64, cint]),
    "mi_pcm_layout_of": (cint, [cint, cint, u64, C.POINTER(Layout)]),
    "mi_pcm_decode_batch": (cint, [vp, cint, cint, vp, u64p, u32p, cint, vp, u64p, vp]),
    "mi_pcm_decode_packet": (cint, [vp, cint, cint, u8p, sz, vp, u32p]),
    "mi_pcm_times": (cint, [vp, f32p, intp]),
}
EXPORTS = list(SIGNATURES)
LIB = Library("libmi_pcm.so", "MI_PCM_LIB", "mi_pcm_", MiPcmError, SIGNATURES)
lib_path, load = LIB.path, LIB.load


def fourcc(name):
    """BGAV_MK_FOURCC of four characters; a WAV id is its own fourcc"""
    if isinstance(name, int):
        return name
    a, b, c, d = name.encode("latin-1")
    return a << 24 | b << 16 | c << 8 | d


def codec_of(fcc, bits, channels, endianess=ENDIANESS_NONE, header=b""):
    """(codec, label, block_align, sample_bytes) as init_pcm chooses, or None where upstream returns 0 or goes on with a
    NULL decode_func (host-side)"""
    f = Format()
    h = (C.c_uint8 * max(len(header), 1)).from_buffer_copy(bytes(header) or b"\0")
    rc = load().mi_pcm_codec_of(fourcc(fcc), bits, channels, endianess, h if header else None, len(header), C.byref(f))
    return None if rc else (f.codec, f.label, f.block_align, f.sample_bytes)


def payload_of(length, duration, block_align):
    """get_packet's clamp (host-side)"""
    return load().mi_pcm_payload_of(length, duration, block_align)


def layout_of(codec, channels, length):
    """(frames, samples upstream writes, bytes consumed, output bytes) of a packet of `length` bytes (host-side)"""
    lay = Layout()
    if load().mi_pcm_layout_of(codec, channels, length, C.byref(lay)) != 0:
        raise MiPcmError(f"codec {codec} with {channels} channels")
    return lay.frames, lay.written, lay.consumed, lay.out_bytes


class MiPcm(Device):
    LIB = LIB

    def _error(self, text, rc, what):
        return MiPcmError(text, {"create": ERR_HIP, "alloc": ERR_NOMEM}.get(what, rc))

    codec_of, payload_of, layout_of = staticmethod(codec_of), staticmethod(payload_of), staticmethod(layout_of)

    def decode_batch(self, codec, channels, d_packets, offsets, lens, d_samples, sample_offsets, d_outside=None):
        """packet i, lens[i] bytes at d_packets + offsets[i] -> its samples at d_samples + sample_offsets[i]; d_outside:
        None or n uint32 counts of samples outside the float domain.  One launch queued on the instance's stream where
        any packet has a sample, and one more before it where d_outside is given.  The library has its own copy of what
        it needs of the three arrays when this returns."""
        offsets, lens = np.ascontiguousarray(offsets, np.uint64), np.ascontiguousarray(lens, np.uint32)
        sample_offsets = np.ascontiguousarray(sample_offsets, np.uint64)
        n = offsets.size
        if lens.size != n or sample_offsets.size != n:
            raise MiPcmError(f"{lens.size} lengths and {sample_offsets.size} sample offsets for {n} offsets")
        self._chk(self.L.mi_pcm_decode_batch(self.c, codec, channels, d_packets, offsets.ctypes.data_as(u64p), lens.ctypes.data_as(u32p),
                                             n, d_samples, sample_offsets.ctypes.data_as(u64p), d_outside))

    def decode_packet(self, codec, channels, data):
        """one host packet -> (its samples as bytes, the count of samples outside the float domain)"""
        data = np.ascontiguousarray(data, np.uint8)
        if not (0 <= codec < len(CODECS)):
            raise MiPcmError(f"codec {codec}")
        out = np.zeros(layout_of(codec, channels, data.size)[3], np.uint8)
        outside = C.c_uint32()
        self._chk(self.L.mi_pcm_decode_packet(self.c, codec, channels, data.ctypes.data_as(u8p), data.size, out.ctypes.data, C.byref(outside)))
        return out, outside.value

    def times(self):
        """(milliseconds, launches) of k_pcm_zero and k_pcm_decode since the last call"""
        return self._times(self.L.mi_pcm_times)
