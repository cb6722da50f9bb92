"""What the ctypes views of the eight libraries (binding.py, dv.py, yuv.py, rgb.py, tga.py, spu.py, gsm.py, pcm.py) share: a Library
opens one shared object and gives its functions the signatures of a table kept as plain data, a Device is the part of MiRtj,
MiDv, MiYuv, MiRgb, MiTga, MiSpu, MiGsm and MiPcm that the eight C interfaces spell alike (include/*.h: create, destroy, last_error, dev_alloc, dev_free, h2d, d2h, sync)."""
import contextlib
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# the types the signature tables are written in
vp, cint, uint, u32, u64, i64, sz = C.c_void_p, C.c_int, C.c_uint, C.c_uint32, C.c_uint64, C.c_longlong, C.c_size_t
u8p, u32p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
intp, i64p, f32p, u8pp = C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_float), C.POINTER(u8p)


class Library:
    """One shared object under lib/: `env` names the environment variable that points at another build of it, `prefix`
    is what its entry points begin with, `error` the class its view raises, `signatures` {name: (restype, [argtypes])} of
    every function its header declares (restype None: void).  Nothing is opened before load()."""

    def __init__(self, file, env, prefix, error, signatures):
        self.file, self.env, self.prefix, self.error, self.signatures = file, env, prefix, error, signatures
        self._lib = None

    def path(self):
        return os.environ.get(self.env) or os.path.join(HERE, "lib", self.file)

    def load(self):
        if self._lib is None:
            p = self.path()
            if not os.path.exists(p):
                raise self.error(f"{p} is missing: run `python gmerlin-avdecoder_amd/build.py` (there is no CPU path)")
            L = C.CDLL(p)
            for name, (restype, argtypes) in self.signatures.items():
                fn = getattr(L, name)
                fn.restype, fn.argtypes = restype, argtypes
            self._lib = L
        return self._lib


class Device:
    """One instance of a library on one device.  L is the loaded library, h the instance's handle (c reads the same)."""
    LIB = None  # the subclass's Library

    def __init__(self, device=-1):
        self.L = self.LIB.load()
        self.h = self._fn("create")(device)
        if not self.h:
            raise self._error(self.last_error(), None, "create")

    c = property(lambda self: self.h)

    def _fn(self, name):
        return getattr(self.L, self.LIB.prefix + name)

    def last_error(self):
        """the text of the instance's last failure (no instance, as after a failed create: of the last failed create)"""
        return self._fn("last_error")(self.h).decode()

    def _error(self, text, rc, what):
        """the exception for the library's message `text`: what is "create" or "alloc" (rc None), or None for a call that
        returned rc != 0.  The libraries word these differently; a subclass says how."""
        return self.LIB.error(text)

    def _chk(self, rc):
        if rc != 0:
            raise self._error(self.last_error(), rc, None)

    def close(self):
        if getattr(self, "h", None):
            self._fn("destroy")(self.h)
            self.h = None

    # -- device memory --
    def alloc(self, nbytes):
        d = self._fn("dev_alloc")(self.h, nbytes)
        if not d:
            raise self._error(self.last_error(), None, "alloc")
        return d

    def free(self, d):
        self._fn("dev_free")(self.h, d)

    def h2d(self, d, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        self._chk(self._fn("h2d")(self.h, d + offset, arr.ctypes.data, arr.nbytes))

    def d2h(self, d, nbytes, offset=0, dtype=np.uint8):
        a = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        self._chk(self._fn("d2h")(self.h, a.ctypes.data, d + offset, nbytes))
        return a

    def sync(self):
        self._chk(self._fn("sync")(self.h))

    def _times(self, fn):
        """(total milliseconds, launches) from one of the library's `int fn(ctx, float *, int *)` timers"""
        ms, n = C.c_float(), C.c_int()
        self._chk(fn(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    @contextlib.contextmanager
    def _resident(self, *what):
        """device buffers for the length of a with block: an array is uploaded, an int is a size in bytes, None stays None"""
        ds = []
        try:
            for a in what:
                ds.append(None if a is None else self.alloc(a if isinstance(a, int) else a.nbytes))
                if isinstance(a, np.ndarray):
                    self.h2d(ds[-1], a)
            yield ds
        finally:
            for d in ds:
                if d:
                    self.free(d)
