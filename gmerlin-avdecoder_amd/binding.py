"""ctypes view of include/mi_rtjpeg.h.  No CPU fallback: if the library is missing or there is no
gfx950 device, construction raises MiRtjError with the library's own message."""
import ctypes as C
import weakref

import numpy as np

from ._capi import Device, Library, cint, f32p, i64p, intp, sz, u8p, u8pp, u32, u32p, u64, u64p, vp


class MiRtjError(RuntimeError):
    pass


# every function of include/mi_rtjpeg.h, in its order: (what it returns, what it takes)
SIGNATURES = {
    "mi_rtj_device_count": (cint, []),
    "mi_rtj_create": (vp, [cint]),
    "mi_rtj_destroy": (None, [vp]),
    "mi_rtj_last_error": (C.c_char_p, [vp]),
    "mi_rtj_set_format": (cint, [vp, cint]),
    "mi_rtj_get_format": (cint, [vp]),
    "mi_rtj_decode": (cint, [vp, u8p, sz, u8pp, intp, cint, cint]),
    "mi_rtj_decode_nocopy": (cint, [vp, u8p, sz, u8pp, intp]),
    "mi_rtj_pipe_create": (vp, [vp, cint, cint, cint]),
    "mi_rtj_pipe_destroy": (None, [vp]),
    "mi_rtj_pipe_room": (cint, [vp]),
    "mi_rtj_pipe_pending": (cint, [vp]),
    "mi_rtj_pipe_submit": (cint, [vp, u8p, sz, u64]),
    "mi_rtj_pipe_next": (cint, [vp, u8pp, intp, intp, intp, u64p]),
    "mi_rtj_pipe_peek_tag": (cint, [vp, u64p]),
    "mi_rtj_pipe_flush": (cint, [vp]),
    "mi_rtj_pipe_profile": (cint, [vp, cint]),
    "mi_rtj_pipe_times": (cint, [vp, f32p, intp]),
    "mi_rtj_get_state": (None, [vp, intp, intp, intp]),
    "mi_rtj_dev_alloc": (vp, [vp, sz]),
    "mi_rtj_dev_free": (None, [vp, vp]),
    "mi_rtj_h2d": (cint, [vp, vp, vp, sz]),
    "mi_rtj_d2h": (cint, [vp, vp, vp, sz]),
    "mi_rtj_dev_memset": (cint, [vp, vp, cint, sz]),
    "mi_rtj_sync": (cint, [vp]),
    "mi_rtj_plan_create": (vp, [vp, cint, u8p, u64p, u32p, u64p]),
    "mi_rtj_plan_destroy": (None, [vp]),
    "mi_rtj_plan_decode": (cint, [vp, vp, vp]),
    "mi_rtj_plan_info": (None, [vp, intp, u64p, u64p, u64p]),
    "mi_rtj_plan_profile": (None, [vp, cint]),
    "mi_rtj_plan_times": (cint, [vp, f32p, intp]),
    "mi_rtj_plan_step_times": (cint, [vp, f32p, cint, intp]),
    "mi_rtj_plan_spec_stats": (cint, [vp, intp, i64p, i64p]),
    "mi_rtj_plan_spec_lead": (cint, [vp, intp, intp]),
    "mi_rtj_plan_decode_form": (cint, [vp, intp, intp, i64p]),
    "mi_rtj_plan_overlapped": (cint, [vp]),
    "mi_rtj_plan_set_runs": (cint, [vp, cint, intp]),
    "mi_rtj_plan_set_runs_fmt": (cint, [vp, cint, intp]),
    "mi_rtj_plan_run_times": (cint, [vp, f32p, intp]),
    "mi_rtj_plan_run_stats": (cint, [vp, i64p]),
    "mi_rtj_plan_read_index": (cint, [vp, u32p, sz]),
    "mi_rtj_synth_frames": (cint, [vp, cint, cint, cint, cint, u32, cint, vp]),
    "mi_rtj_synth_frames_lcg": (cint, [vp, cint, cint, cint, cint, u32, cint, vp]),
    "mi_rtj_encode_bound": (sz, [cint, cint, cint, cint]),
    "mi_rtj_encode_frames": (cint, [vp, cint, cint, cint, cint, vp, vp, cint, u64p, u32p]),
    "mi_rtj_encode_stream": (cint, [vp, cint, cint, cint, cint, cint, cint, cint, vp, vp, cint, u64p, u32p]),
    "mi_rtj_encode_bound_fmt": (sz, [cint, cint, cint, cint, cint]),
    "mi_rtj_encode_frames_fmt": (cint, [vp, cint, cint, cint, cint, cint, vp, vp, cint, u64p, u32p]),
    "mi_rtj_encode_stream_fmt": (cint, [vp, cint, cint, cint, cint, cint, cint, cint, cint, vp, vp, cint, u64p, u32p]),
    "mi_rtj_yuv420_to_rgb": (cint, [vp, cint, cint, cint, cint, vp, sz, vp, sz, sz]),
    "mi_rtj_yuv422_to_rgb24": (cint, [vp, cint, cint, cint, vp, sz, vp, sz, sz]),
    "mi_rtj_copy_ceiling": (cint, [vp, vp, vp, sz, cint, C.POINTER(C.c_double)]),
    "mi_rtj_get_tables": (cint, [cint, C.POINTER(C.c_int32), intp, intp]),
}
EXPORTS = list(SIGNATURES)
# MI_RTJ_LIB: an alternative build of the same library (A/B experiments under tools/)
LIB = Library("libmi_rtjpeg.so", "MI_RTJ_LIB", "mi_rtj_", MiRtjError, SIGNATURES)
lib_path, load = LIB.path, LIB.load

# picture formats (mi_rtj_set_format): RTJ_YUV420 / RTJ_YUV422 / RTJ_RGB8 of the reference
FMT_YUV420, FMT_YUV422, FMT_GREY = 0, 1, 2


def plane_sizes(fmt, w, h):
    """(bytes of Y, bytes of each chroma plane) of a w x h picture: chroma is w/2 x h/2 in 4:2:0, w/2 x h in 4:2:2, absent
    in greyscale."""
    return w * h, {FMT_YUV420: (w // 2) * (h // 2), FMT_YUV422: (w // 2) * h, FMT_GREY: 0}[fmt]


def blocks_of(fmt, w, h):
    """8x8 blocks of a w x h picture in stream order: 6 per 16x16 / 4 per 16x8 macroblock / 1 per block"""
    return {FMT_YUV420: (w // 16) * (h // 16) * 6, FMT_YUV422: (w // 16) * (h // 8) * 4, FMT_GREY: (w // 8) * (h // 8)}[fmt]


KERNELS = ("k_index_summarize", "k_index_resolve", "k_index_emit", "k_decode", "k_spec_walk", "k_spec_verify")


def device_count():
    return load().mi_rtj_device_count()


def get_tables(Q):
    t = (C.c_int32 * 128)()
    lb8, cb8 = C.c_int(), C.c_int()
    rc = load().mi_rtj_get_tables(Q, t, C.byref(lb8), C.byref(cb8))
    if rc != 0:
        raise MiRtjError(f"mi_rtj_get_tables({Q}) -> {rc}")
    a = np.array(t, dtype=np.int32)
    return a[:64], a[64:], lb8.value, cb8.value


def _run_lengths(lengths):
    """(how many runs, their lengths as the int array both set_runs calls take); [] or None: no runs"""
    lengths = [int(x) for x in (lengths or [])]
    return len(lengths), (C.c_int * max(len(lengths), 1))(*lengths)


class Plan:
    def __init__(self, owner, handle, n):
        self.owner, self.h, self.n = owner, handle, n
        self.fmt = owner.format  # a plan takes the instance's format when it is created
        owner._plans.add(self)

    def picture_bytes(self, w, h):
        """bytes a w x h picture of this plan takes in the output buffer (Y, then the chroma planes, contiguous)"""
        ysz, csz = plane_sizes(self.fmt, w, h)
        return ysz + 2 * csz

    def close(self):
        if self.h:
            self.owner.L.mi_rtj_plan_destroy(self.h)
            self.h = None
            self.owner._plans.discard(self)

    def __del__(self):
        self.close()

    def decode(self, d_stream, d_out):
        self.owner._chk(self.owner.L.mi_rtj_plan_decode(self.h, d_stream, d_out))

    def info(self):
        n = C.c_int()
        nb, bi, bo = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self.owner.L.mi_rtj_plan_info(self.h, C.byref(n), C.byref(nb), C.byref(bi), C.byref(bo))
        return dict(frames=n.value, blocks=nb.value, bytes_in=bi.value, bytes_out=bo.value)

    def profile(self, on=True):
        self.owner.L.mi_rtj_plan_profile(self.h, 1 if on else 0)

    def spec_stats(self):
        """(packets proven by the speculative index in the last decode, stream chunks it covered; 0 = unused)."""
        pr, wk, rp = C.c_int(), C.c_longlong(), C.c_longlong()
        self.owner._chk(self.owner.L.mi_rtj_plan_spec_stats(self.h, C.byref(pr), C.byref(wk), C.byref(rp)))
        self.repaired = rp.value
        return pr.value, wk.value

    def step_times(self, max_steps=4096):
        """device milliseconds of every decode since profile(True), first kernel's start to k_decode's end."""
        ms = (C.c_float * max_steps)()
        n = C.c_int()
        self.owner._chk(self.owner.L.mi_rtj_plan_step_times(self.h, ms, max_steps, C.byref(n)))
        return [float(ms[i]) for i in range(min(n.value, max_steps))]

    def decode_form(self):
        """(form of the transform kernel the policy chose for the next batch decode: 0 split / 1 classic / -1 none yet,
        classic decodes left, group parts the last decode left to k_decode_list)."""
        form, left, listed = C.c_int(), C.c_int(), C.c_longlong()
        self.owner._chk(self.owner.L.mi_rtj_plan_decode_form(self.h, C.byref(form), C.byref(left), C.byref(listed)))
        return form.value, left.value, listed.value

    def overlapped(self):
        """True if the last decode built its index on the plan's own stream, next to the previous decode's transform."""
        return bool(self.owner.L.mi_rtj_plan_overlapped(self.h))

    def spec_lead(self):
        """(bytes a walker parses before its chunk in the next decode, decodes left without speculation)."""
        lead, paused = C.c_int(), C.c_int()
        self.owner._chk(self.owner.L.mi_rtj_plan_spec_lead(self.h, C.byref(lead), C.byref(paused)))
        return lead.value, paused.value

    def times(self):
        ms = (C.c_float * len(KERNELS))()
        n = C.c_int()
        self.owner._chk(self.owner.L.mi_rtj_plan_times(self.h, ms, C.byref(n)))
        return dict(zip(KERNELS, [float(x) for x in ms])), n.value

    def set_runs(self, lengths):
        """Cut the plan into runs of consecutive pictures of one stream (include/mi_rtjpeg.h, "runs"); [] or None:
        independent pictures again.  Raises MiRtjError (and leaves the plan as it was) on a refused cut."""
        self.owner._chk(self.owner.L.mi_rtj_plan_set_runs(self.h, *_run_lengths(lengths)))

    def set_runs_fmt(self, lengths):
        """set_runs for a plan of any format (mi_rtj_plan_set_runs_fmt): on a 4:2:0 plan it is set_runs; on a 4:2:2 or
        greyscale plan "block b" of the run rule is in the format's stream order.  Same errors, same queries."""
        self.owner._chk(self.owner.L.mi_rtj_plan_set_runs_fmt(self.h, *_run_lengths(lengths)))

    def run_times(self):
        """(ms of the run kernels summed over the decodes since profile(True), decodes that ran them)."""
        ms, n = C.c_float(), C.c_int()
        self.owner._chk(self.owner.L.mi_rtj_plan_run_times(self.h, C.byref(ms), C.byref(n)))
        return float(ms.value), n.value

    def run_copied(self):
        """unchanged blocks the last decode copied from an earlier picture of their run (0: no run kernels ran)."""
        v = C.c_longlong()
        self.owner._chk(self.owner.L.mi_rtj_plan_run_stats(self.h, C.byref(v)))
        return v.value

    def read_index(self):
        cnt = self.info()["blocks"] + self.n
        a = np.zeros(cnt, dtype=np.uint32)
        self.owner._chk(self.owner.L.mi_rtj_plan_read_index(self.h, a.ctypes.data_as(u32p), cnt))
        return a


class Pipe:
    """View of mi_rtj_pipe (include/mi_rtjpeg.h, "pipelined session") for tests and bench.py."""

    def __init__(self, owner, depth, coded_w, coded_h):
        self.owner = owner
        self.h = owner.L.mi_rtj_pipe_create(owner.h, depth, coded_w, coded_h)
        if not self.h:
            raise MiRtjError("mi_rtj_pipe_create failed: " + owner.last_error())

    def close(self):
        if self.h:
            self.owner.L.mi_rtj_pipe_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def room(self):
        return self.owner.L.mi_rtj_pipe_room(self.h)

    def pending(self):
        return self.owner.L.mi_rtj_pipe_pending(self.h)

    def submit(self, pkt, tag=0):
        pkt = np.ascontiguousarray(pkt, dtype=np.uint8)
        self.owner._chk(self.owner.L.mi_rtj_pipe_submit(self.h, pkt.ctypes.data_as(u8p), pkt.size, tag))

    def next(self, drop=False):
        """(y, u, v, tag): numpy views of the session's pinned picture, valid until the next call; drop: tag only."""
        tag = C.c_uint64()
        if drop:
            self.owner._chk(self.owner.L.mi_rtj_pipe_next(self.h, None, None, None, None, C.byref(tag)))
            return tag.value
        planes = (u8p * 3)()
        st = (C.c_int * 3)()
        w, h = C.c_int(), C.c_int()
        self.owner._chk(self.owner.L.mi_rtj_pipe_next(self.h, planes, st, C.byref(w), C.byref(h), C.byref(tag)))
        mk = lambda p, n: np.ctypeslib.as_array(p, shape=(n,))
        n = w.value * h.value
        return mk(planes[0], n), mk(planes[1], n // 4), mk(planes[2], n // 4), tag.value

    def flush(self):
        self.owner._chk(self.owner.L.mi_rtj_pipe_flush(self.h))

    def profile(self, enable):
        """kernel timing of the packets decoded from here on (flushes the session; not for timed regions)"""
        self.owner._chk(self.owner.L.mi_rtj_pipe_profile(self.h, 1 if enable else 0))

    def times(self):
        """({kernel: ms summed over the packets decoded since profile(True)}, packets)"""
        ms = (C.c_float * len(KERNELS))()
        n = C.c_int()
        self.owner._chk(self.owner.L.mi_rtj_pipe_times(self.h, ms, C.byref(n)))
        return dict(zip(KERNELS, [float(x) for x in ms])), n.value


class MiRtj(Device):
    """One decoder instance (== one RTjpeg_t of the reference) bound to one device."""
    LIB = LIB

    def __init__(self, device=-1):
        self._plans = weakref.WeakSet()
        super().__init__(device)

    def _error(self, text, rc, what):
        return MiRtjError({"create": "mi_rtj_create failed: ", "alloc": "alloc failed: "}.get(what, f"rc={rc}: ") + text)

    def close(self):
        if getattr(self, "h", None):
            for p in list(self._plans):  # a plan must not outlive its instance
                p.close()
        super().close()

    def __del__(self):
        self.close()

    # -- picture format (RTjpeg_set_format) --
    def set_format(self, fmt):
        """FMT_YUV420 / FMT_YUV422 / FMT_GREY; before the first decode, plan or session (later: only the format it has)."""
        self._chk(self.L.mi_rtj_set_format(self.h, int(fmt)))

    @property
    def format(self):
        return self.L.mi_rtj_get_format(self.h)

    # -- one packet in, one frame out (decode_rtjpeg) --
    def decode(self, pkt, out=None, crop=None, strides=None):
        """pkt: uint8 array.  out: uint8 array receiving Y,U,V back to back (with `strides`, each plane
        has its own row pitch; 4:2:2: chroma planes of every line; greyscale: Y alone).  Returns rc-checked None."""
        pkt = np.ascontiguousarray(pkt, dtype=np.uint8)
        pp = pkt.ctypes.data_as(u8p)
        if out is None:
            self._chk(self.L.mi_rtj_decode(self.h, pp, pkt.size, None, None, 0, 0))
            return
        w = int(pkt[6]) | (int(pkt[7]) << 8)
        h = int(pkt[8]) | (int(pkt[9]) << 8)
        cw, ch = crop if crop else (w, h)
        fmt = self.format
        if strides is None:
            strides = (cw, (cw + 1) // 2, (cw + 1) // 2)
        ysz = strides[0] * ch
        if fmt == FMT_GREY:
            assert out.size >= ysz
            planes = (u8p * 3)(C.cast(out.ctypes.data, u8p), None, None)
            st = (C.c_int * 3)(strides[0], 0, 0)
            self._chk(self.L.mi_rtj_decode(self.h, pp, pkt.size, planes, st, cw, ch))
            return
        csz = strides[1] * (ch if fmt == FMT_YUV422 else (ch + 1) // 2)
        assert out.size >= ysz + 2 * csz
        base = out.ctypes.data
        planes = (u8p * 3)(C.cast(base, u8p), C.cast(base + ysz, u8p), C.cast(base + ysz + csz, u8p))
        st = (C.c_int * 3)(*strides)
        self._chk(self.L.mi_rtj_decode(self.h, pp, pkt.size, planes, st, cw, ch))

    def decode_nocopy(self, pkt):
        """Returns (y, u, v) numpy views of the instance's pinned picture, valid until the next decode (greyscale:
        u and v are None)."""
        pkt = np.ascontiguousarray(pkt, dtype=np.uint8)
        planes = (u8p * 3)()
        st = (C.c_int * 3)()
        self._chk(self.L.mi_rtj_decode_nocopy(self.h, pkt.ctypes.data_as(u8p), pkt.size, planes, st))
        w = int(pkt[6]) | (int(pkt[7]) << 8)
        h = int(pkt[8]) | (int(pkt[9]) << 8)
        mk = lambda p, n: np.ctypeslib.as_array(p, shape=(n,))
        ysz, csz = plane_sizes(self.format, w, h)
        if csz == 0:
            assert not planes[1] and not planes[2] and st[1] == 0 and st[2] == 0
            return mk(planes[0], ysz), None, None
        return mk(planes[0], ysz), mk(planes[1], csz), mk(planes[2], csz)

    def pipe(self, depth=4, coded_w=0, coded_h=0):
        """A pipelined session (mi_rtj_pipe_*): packets in, pictures out in order, several in flight."""
        return Pipe(self, depth, coded_w, coded_h)

    def state(self):
        w, h, q = C.c_int(), C.c_int(), C.c_int()
        self.L.mi_rtj_get_state(self.h, C.byref(w), C.byref(h), C.byref(q))
        return w.value, h.value, q.value

    def memset(self, dptr, value, nbytes, offset=0):
        self._chk(self.L.mi_rtj_dev_memset(self.h, dptr + offset, value, nbytes))

    # -- batches --
    def plan(self, headers, pkt_offset, pkt_len, out_offset):
        headers = np.ascontiguousarray(headers, dtype=np.uint8).reshape(-1)
        n = headers.size // 12
        po = np.ascontiguousarray(pkt_offset, dtype=np.uint64)
        pl = np.ascontiguousarray(pkt_len, dtype=np.uint32)
        oo = np.ascontiguousarray(out_offset, dtype=np.uint64)
        assert po.size == n and pl.size == n and oo.size == n
        h = self.L.mi_rtj_plan_create(self.h, n, headers.ctypes.data_as(u8p), po.ctypes.data_as(u64p),
                                      pl.ctypes.data_as(u32p), oo.ctypes.data_as(u64p))
        if not h:
            raise MiRtjError("plan_create failed: " + self.last_error())
        return Plan(self, h, n)

    def upload_packets(self, pkts, align=1):
        """Host packets -> one device stream buffer.  Returns (dptr, offsets, lens, headers)."""
        offs, lens, cur = [], [], 0
        for p in pkts:
            cur = (cur + align - 1) // align * align
            offs.append(cur)
            lens.append(p.size)
            cur += p.size
        host = np.zeros(max(cur, 1), dtype=np.uint8)
        hdrs = np.zeros((len(pkts), 12), dtype=np.uint8)
        for i, p in enumerate(pkts):
            host[offs[i]:offs[i] + p.size] = p
            m = min(12, p.size)
            hdrs[i, :m] = p[:m]
        d = self.alloc(host.size)
        self.h2d(d, host)
        return d, np.array(offs, np.uint64), np.array(lens, np.uint32), hdrs

    # -- colour stage (N2) --
    def to_rgb(self, fmt, w, h, n, d_planes, in_stride, d_rgb, row_pitch, out_stride):
        self._chk(self.L.mi_rtj_yuv420_to_rgb(self.h, fmt, w, h, n, d_planes, in_stride, d_rgb, row_pitch, out_stride))

    def to_rgb422(self, w, h, n, d_planes, in_stride, d_rgb, row_pitch, out_stride):
        """RTjpeg_yuv422rgb24: n frames of contiguous 4:2:2 planes to R, G, B bytes"""
        self._chk(self.L.mi_rtj_yuv422_to_rgb24(self.h, w, h, n, d_planes, in_stride, d_rgb, row_pitch, out_stride))

    def copy_ceiling(self, d_src, d_dst, nbytes, reps=10):
        """GB/s (read + write) a plain streaming copy kernel sustains on this device."""
        g = C.c_double()
        self._chk(self.L.mi_rtj_copy_ceiling(self.h, d_src, d_dst, nbytes, reps, C.byref(g)))
        return g.value

    # -- generator side --
    def synth(self, w, h, first, n, seed=12345, amp=8, dptr=None):
        fsz = w * h * 3 // 2
        d = dptr if dptr is not None else self.alloc(fsz * n)
        self._chk(self.L.mi_rtj_synth_frames(self.h, w, h, first, n, seed, amp, d))
        return d

    def synth_lcg(self, w, h, first, n, seed=12345, amp=8, dptr=None):
        """SURVEY 8d's generator: LCG noise, one sequence over all frames (see include/mi_rtjpeg.h)"""
        fsz = w * h * 3 // 2
        d = dptr if dptr is not None else self.alloc(fsz * n)
        self._chk(self.L.mi_rtj_synth_frames_lcg(self.h, w, h, first, n, seed, amp, d))
        return d

    def encode_bound(self, w, h, n, align=64, fmt=FMT_YUV420):
        if fmt == FMT_YUV420:
            return self.L.mi_rtj_encode_bound(w, h, n, align)
        return self.L.mi_rtj_encode_bound_fmt(int(fmt), w, h, n, align)

    def encode(self, w, h, Q, n, d_frames, align=64, key_rate=0, lmask=0, cmask=0, d_stream=None, fmt=FMT_YUV420):
        """Intra batch (key_rate 0) or one in-order stream with skip blocks (key_rate > 0).  d_stream: a buffer of
        encode_bound() bytes the caller allocated (else one is allocated here).  fmt: the pictures' format (FMT_YUV422:
        Y, Cb, Cr of 2 w h bytes; FMT_GREY: Y alone); it is the call's, not the instance's (set_format)."""
        if fmt != FMT_YUV420:
            return self._encode_fmt(int(fmt), w, h, Q, n, d_frames, align, key_rate, lmask, cmask, d_stream)
        bound = self.L.mi_rtj_encode_bound(w, h, n, align)
        if d_stream is None:
            d_stream = self.alloc(bound)
        po = np.zeros(n, np.uint64)
        pl = np.zeros(n, np.uint32)
        if key_rate > 0:
            self._chk(self.L.mi_rtj_encode_stream(self.h, w, h, Q, key_rate, lmask, cmask, n, d_frames, d_stream,
                                                  align, po.ctypes.data_as(u64p), pl.ctypes.data_as(u32p)))
        else:
            self._chk(self.L.mi_rtj_encode_frames(self.h, w, h, Q, n, d_frames, d_stream, align,
                                                  po.ctypes.data_as(u64p), pl.ctypes.data_as(u32p)))
        return d_stream, po, pl

    def _encode_fmt(self, fmt, w, h, Q, n, d_frames, align, key_rate, lmask, cmask, d_stream):
        """encode() for 4:2:2 and greyscale pictures: mi_rtj_encode_frames_fmt / mi_rtj_encode_stream_fmt"""
        own = d_stream is None
        if own:
            d_stream = self.alloc(max(self.L.mi_rtj_encode_bound_fmt(fmt, w, h, n, align), 1))
        po = np.zeros(max(n, 1), np.uint64)
        pl = np.zeros(max(n, 1), np.uint32)
        pop, plp = po.ctypes.data_as(u64p), pl.ctypes.data_as(u32p)
        if key_rate > 0:
            rc = self.L.mi_rtj_encode_stream_fmt(self.h, fmt, w, h, Q, key_rate, lmask, cmask, n, d_frames, d_stream,
                                                 align, pop, plp)
        else:
            rc = self.L.mi_rtj_encode_frames_fmt(self.h, fmt, w, h, Q, n, d_frames, d_stream, align, pop, plp)
        if rc != 0 and own:  # a refused call (the library names the rule) leaves nothing allocated
            self.free(d_stream)
        self._chk(rc)
        return d_stream, po[:n], pl[:n]
