"""ctypes view of include/mi_gsm.h (libmi_gsm.so, GSM 06.10 full rate and its Microsoft framing: lib/audio_gsm.c over
lib/GSM610/).  No CPU path: without the library or a gfx950 device construction raises MiGsmError with the library's own
message; explode is host-side and needs no device.

fmt 0 is the plain framing (a unit is a frame of 33 bytes and 160 samples), fmt 1 the Microsoft one (a unit is a block of
65 bytes and 320 samples).  A state is STATE_BYTES: 144 int16."""
import ctypes as C

import numpy as np

from ._capi import Device, Library, cint, f32p, intp, sz, u8p, u32p, u64p, vp

OK, ERR_ARG, ERR_HIP, ERR_NOMEM = 0, -1, -2, -3
FRAME_BYTES, BLOCK_BYTES, FRAME_SAMPLES, PARAMS, STATE_BYTES = 33, 65, 160, 76, 288
MAX_STREAMS, MAX_UNITS = 1 << 20, 1 << 24
i16p = C.POINTER(C.c_int16)


class MiGsmError(RuntimeError):
    def __init__(self, message, code=ERR_ARG):
        super().__init__(message)
        self.code = code


# every function of include/mi_gsm.h, in its order: (what it returns, what it takes)
SIGNATURES = {
    "mi_gsm_device_count": (cint, []),
    "mi_gsm_create": (vp, [cint]),
    "mi_gsm_destroy": (None, [vp]),
    "mi_gsm_last_error": (C.c_char_p, [vp]),
    "mi_gsm_dev_alloc": (vp, [vp, sz]),
    "mi_gsm_dev_free": (None, [vp, vp]),
    "mi_gsm_h2d": (cint, [vp, vp, vp, sz]),
    "mi_gsm_d2h": (cint, [vp, vp, vp, sz]),
    "mi_gsm_sync": (cint, [vp]),
    "mi_gsm_state_reset": (cint, [vp, vp, cint]),
    "mi_gsm_explode": (cint, [u8p, cint, i16p]),
    "mi_gsm_decode_batch": (cint, [vp, vp, u64p, u32p, cint, cint, vp, u64p, vp, vp]),
    "mi_gsm_decode_stream": (cint, [vp, u8p, sz, cint, i16p, vp, u32p]),
    "mi_gsm_times": (cint, [vp, f32p, intp]),
}
EXPORTS = list(SIGNATURES)
LIB = Library("libmi_gsm.so", "MI_GSM_LIB", "mi_gsm_", MiGsmError, SIGNATURES)
lib_path, load = LIB.path, LIB.load


def unit_bytes(fmt):
    return BLOCK_BYTES if fmt else FRAME_BYTES


def unit_samples(fmt):
    return FRAME_SAMPLES << (1 if fmt else 0)


def explode(block, fmt):
    """the 76 parameters of a 33-byte frame (fmt 0) or the 152 of a 65-byte block (fmt 1) as a list, in the order of the
    bit stream; None for a bad magic (host-side)"""
    block = np.ascontiguousarray(block, np.uint8)
    if fmt not in (0, 1) or block.size != unit_bytes(fmt):
        raise MiGsmError(f"a unit of fmt {fmt} is not {block.size} bytes")
    out = np.zeros(PARAMS << fmt, np.int16)
    rc = load().mi_gsm_explode(block.ctypes.data_as(u8p), fmt, out.ctypes.data_as(i16p))
    if rc < 0:
        raise MiGsmError(load().mi_gsm_last_error(None).decode(), rc)
    return None if rc else [int(x) for x in out]


class MiGsm(Device):
    LIB = LIB

    def _error(self, text, rc, what):
        return MiGsmError(text, {"create": ERR_HIP, "alloc": ERR_NOMEM}.get(what, rc))

    explode = staticmethod(explode)

    def state_reset(self, d_state, n):
        """n fresh states at d_state (queued on the instance's stream)"""
        self._chk(self.L.mi_gsm_state_reset(self.c, d_state, n))

    def decode_batch(self, d_stream, offsets, units, fmt, d_pcm, pcm_offsets, d_state=None, d_bad=None):
        """stream i, units[i] units at d_stream + offsets[i] -> its samples at d_pcm + pcm_offsets[i]; d_state: None (every
        stream starts fresh) or n states, read and written back; d_bad: None or n uint32 counts of bad magics.  One launch
        queued on the instance's stream.  The library has its own copy of the three arrays when this returns."""
        offsets, units = np.ascontiguousarray(offsets, np.uint64), np.ascontiguousarray(units, np.uint32)
        pcm_offsets = np.ascontiguousarray(pcm_offsets, np.uint64)
        n = offsets.size
        if units.size != n or pcm_offsets.size != n:
            raise MiGsmError(f"{units.size} unit counts and {pcm_offsets.size} sample offsets for {n} offsets")
        self._chk(self.L.mi_gsm_decode_batch(self.c, d_stream, offsets.ctypes.data_as(u64p), units.ctypes.data_as(u32p), n, fmt,
                                             d_pcm, pcm_offsets.ctypes.data_as(u64p), d_state, d_bad))

    def decode_stream(self, data, fmt, state=None):
        """one host stream -> (samples int16, the count of bad magics); state: None (fresh) or a uint8/int16 array of
        STATE_BYTES, which is updated in place.  A tail that is no whole unit is dropped."""
        data = np.ascontiguousarray(data, np.uint8)
        pcm = np.zeros(data.size // unit_bytes(fmt) * unit_samples(fmt), np.int16)
        if state is not None and (not isinstance(state, np.ndarray) or state.nbytes != STATE_BYTES or not state.flags.c_contiguous):
            raise MiGsmError(f"a state is a contiguous array of {STATE_BYTES} bytes")
        bad = C.c_uint32()
        self._chk(self.L.mi_gsm_decode_stream(self.c, data.ctypes.data_as(u8p), data.size, fmt, pcm.ctypes.data_as(i16p),
                                              None if state is None else state.ctypes.data, C.byref(bad)))
        return pcm, bad.value

    def times(self):
        """(milliseconds, launches) of k_gsm_decode since the last call"""
        return self._times(self.L.mi_gsm_times)
