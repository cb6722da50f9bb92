"""ctypes view of include/mi_dv.h (libmi_dv.so, the DV decoder and encoder: 525/60 4:1:1, 625/50 4:2:0 and 625/50 4:1:1 at
25 Mbit/s, both line systems in 4:2:2 at 50 Mbit/s).  No CPU path: without the library or a gfx950 device construction raises MiDvError with
the library's own message."""
import ctypes as C

import numpy as np

from ._capi import Device, Library, cint, f32p, i64, i64p, intp, sz, u8p, u8pp, uint, vp

FRAME_BYTES, PICTURE_BYTES, W, H, CW = 120000, 720 * 480 * 3 // 2, 720, 480, 180
SYS_525_60, SYS_625_50 = 0, 1
FRAME_BYTES_625, PICTURE_BYTES_625, H_625, CW_625, CH_625 = 144000, 720 * 576 + 2 * 360 * 288, 576, 360, 288
SYS_525_60_422, SYS_625_50_422 = 4, 5  # the 50 Mbit/s systems: VAUX stype 4 | DSF
FRAME_BYTES_525_422, PICTURE_BYTES_525_422, FRAME_BYTES_625_422, PICTURE_BYTES_625_422, CW_422 = \
    240000, 720 * 480 * 2, 288000, 720 * 576 * 2, 360
SYS_625_50_411 = 3  # DVCPRO 625/50 4:1:1 (DSF 1, stype 0, APT != 0): 625/50 frames, Y 720 x 576, Cb / Cr 180 x 576
CW_625_411, PICTURE_BYTES_625_411 = 180, 720 * 576 + 2 * 180 * 576
# per system: frame bytes, picture bytes, (width, height) of the planes Y, Cb, Cr
GEOMETRY = {SYS_525_60: (FRAME_BYTES, PICTURE_BYTES, ((W, H), (CW, H), (CW, H))),
            SYS_625_50: (FRAME_BYTES_625, PICTURE_BYTES_625, ((W, H_625), (CW_625, CH_625), (CW_625, CH_625))),
            SYS_625_50_411: (FRAME_BYTES_625, PICTURE_BYTES_625_411, ((W, H_625), (CW_625_411, H_625), (CW_625_411, H_625))),
            SYS_525_60_422: (FRAME_BYTES_525_422, PICTURE_BYTES_525_422, ((W, H), (CW_422, H), (CW_422, H))),
            SYS_625_50_422: (FRAME_BYTES_625_422, PICTURE_BYTES_625_422, ((W, H_625), (CW_422, H_625), (CW_422, H_625)))}
META_INTS = 16  # include/mi_dv.h: MI_DV_META_INTS; the row: found mask, timecode h m s f, drop, y m d, h m s, wide, raw x 3
META_HAS_TIMECODE, META_HAS_DATE, META_HAS_TIME, META_HAS_CONTROL = 1, 2, 4, 8
AUDIO_PAIRS, AUDIO_PAIR_BYTES = 4, 8192  # include/mi_dv.h: MI_DV_AUDIO_PAIRS, MI_DV_AUDIO_PAIR_BYTES
AUDIO_CHANNELS = {SYS_525_60: 1, SYS_625_50: 1, SYS_625_50_411: 1, SYS_525_60_422: 2, SYS_625_50_422: 2}  # DIF channels
STA_ERRORS = 0x8080  # the default mask of held macroblocks: STA 0111 and 1111 (include/mi_dv.h: MI_DV_STA_ERRORS)


class MiDvError(RuntimeError):
    pass


# every function of include/mi_dv.h, in its order: (what it returns, what it takes)
SIGNATURES = {
    "mi_dv_device_count": (cint, []),
    "mi_dv_create": (vp, [cint]),
    "mi_dv_destroy": (None, [vp]),
    "mi_dv_last_error": (C.c_char_p, [vp]),
    "mi_dv_dev_alloc": (vp, [vp, sz]),
    "mi_dv_dev_free": (None, [vp, vp]),
    "mi_dv_h2d": (cint, [vp, vp, vp, sz]),
    "mi_dv_d2h": (cint, [vp, vp, vp, sz]),
    "mi_dv_sync": (cint, [vp]),
    "mi_dv_decode_batch": (cint, [vp, vp, cint, vp]),
    "mi_dv_kernel_times": (cint, [vp, f32p, intp]),
    "mi_dv_decode_frame": (cint, [vp, u8p, sz, u8pp, intp]),
    "mi_dv_copy_tables": (sz, [vp, sz]),
    "mi_dv_system_of": (cint, [u8p, sz]),
    "mi_dv_profile_of": (cint, [u8p, sz]),
    "mi_dv_kind_of": (cint, [u8p, sz]),
    "mi_dv_decode_batch_sys": (cint, [vp, cint, vp, cint, vp]),
    "mi_dv_decode_frame_sys": (cint, [vp, cint, u8p, sz, u8pp, intp]),
    "mi_dv_mb_place": (cint, [cint, cint, cint, cint, intp, intp]),
    "mi_dv_mb_rects": (cint, [cint, cint, cint, cint, C.POINTER(C.c_int * 4)]),
    "mi_dv_held_macroblocks": (cint, [cint, u8p, sz, uint]),
    "mi_dv_decode_batch_held": (cint, [vp, cint, vp, cint, vp, cint, intp, vp, uint]),
    "mi_dv_hold_stats": (cint, [vp, i64p]),
    "mi_dv_hold_times": (cint, [vp, f32p, intp]),
    "mi_dv_decode_frame_held": (cint, [vp, cint, u8p, sz, u8pp, intp, uint, intp]),
    "mi_dv_hold_reset": (cint, [vp]),
    "mi_dv_encode_batch": (cint, [vp, cint, vp, cint, vp, cint]),
    "mi_dv_encode_frame": (cint, [vp, cint, u8pp, intp, u8p, sz, cint]),
    "mi_dv_encode_times": (cint, [vp, f32p, intp]),
    "mi_dv_encode_stats": (cint, [vp, i64p, i64p]),
    "mi_dv_audio_batch": (cint, [vp, cint, vp, cint, vp, cint, vp]),
    "mi_dv_audio_write_batch": (cint, [vp, cint, vp, cint, vp, cint, cint, intp]),
    "mi_dv_audio_samples": (cint, [cint, cint, i64]),
    "mi_dv_audio_times": (cint, [vp, f32p, intp]),
    "mi_dv_audio_copy_tables": (sz, [vp, sz]),
    "mi_dv_meta_batch": (cint, [vp, cint, vp, cint, vp]),
    "mi_dv_meta_write_batch": (cint, [vp, cint, vp, cint, i64, cint, i64, cint]),
    "mi_dv_timecode_of": (cint, [cint, i64, cint, intp]),
    "mi_dv_meta_times": (cint, [vp, f32p, intp]),
}
EXPORTS = list(SIGNATURES)
LIB = Library("libmi_dv.so", "MI_DV_LIB", "mi_dv_", MiDvError, SIGNATURES)
lib_path, load = LIB.path, LIB.load


def tables():
    """the decoder's constant tables as the kernels get them (host-side: works without a GPU)"""
    L = load()
    n = L.mi_dv_copy_tables(None, 0)
    a = np.zeros(n // 4, np.uint32)
    L.mi_dv_copy_tables(a.ctypes.data, n)
    return {"lut9": a[:512], "lut2": a[512:576], "tab": a[576:704].reshape(2, 64), "shift4": a[704:728]}


def audio_tables():
    """the sound's layout table as both audio kernels get it: first-slot shuffle [line system][sequence][audio block],
    stride and minimum samples (48, 44.1, 32 kHz) per line system (0: 525/60, 1: 625/50) (host-side)"""
    L = load()
    n = L.mi_dv_audio_copy_tables(None, 0)
    a = np.zeros(n // 2, np.uint16)
    L.mi_dv_audio_copy_tables(a.ctypes.data, n)
    return {"shuffle": a[:216].reshape(2, 12, 9), "stride": a[216:218], "min_samples": a[218:224].reshape(2, 3)}


def audio_samples(system, samplerate, k):
    """the samples per channel of frame k (from 0) of an unlocked stream of the system at the rate (host-side)"""
    L = load()
    n = L.mi_dv_audio_samples(system, samplerate, k)
    if n < 0:
        raise MiDvError(L.mi_dv_last_error(None).decode())
    return n


def timecode_of(system, frame, drop=0):
    """(hours, minutes, seconds, frames) of frame number `frame` (from 0) as write_meta_batch labels it: 25 or 30 frames a
    second, drop 1 (525/60 systems only): SMPTE drop-frame; hours wrap at 24 (host-side)"""
    L = load()
    v = (C.c_int * 4)()
    if L.mi_dv_timecode_of(system, frame, drop, v) != 0:
        raise MiDvError(L.mi_dv_last_error(None).decode())
    return tuple(v)


def geometry(system):
    """(frame bytes, picture bytes, ((w, h) of Y, Cb, Cr)) of a system"""
    if system not in GEOMETRY:
        raise MiDvError(f"unknown DV system {system}")
    return GEOMETRY[system]


def system_of(frame):
    """the 25 Mbit/s system a DIF frame announces (SYS_525_60 / SYS_625_50), -1 for other profiles and short frames
    (host-side)"""
    frame = np.ascontiguousarray(frame, np.uint8)
    return load().mi_dv_system_of(frame.ctypes.data_as(u8p), frame.nbytes)


def profile_of(frame):
    """the same over all four decodable profiles: SYS_525_60, SYS_625_50, SYS_525_60_422 or SYS_625_50_422; -1 for
    every other profile and for short frames (host-side)"""
    frame = np.ascontiguousarray(frame, np.uint8)
    return load().mi_dv_profile_of(frame.ctypes.data_as(u8p), frame.nbytes)


def kind_of(frame):
    """the same over all five decodable profiles: those of profile_of and SYS_625_50_411 (DSF 1, stype 0, APT != 0), for
    which profile_of and system_of keep answering -1; -1 for every other profile and for short frames (host-side)"""
    frame = np.ascontiguousarray(frame, np.uint8)
    return load().mi_dv_kind_of(frame.ctypes.data_as(u8p), frame.nbytes)


def place_of(system, seq, slot, m):
    """the kernels' placement of macroblock m of segment `slot` of sequence `seq` for any of the five systems: (x, y) —
    525/60 and 625/50 4:1:1 in 32-pixel columns and 8-line rows (0..59 / 0..71), 625/50 in 16 x 16 macroblocks, the 4:2:2
    systems in 16-pixel columns and 8-line rows with `seq` counting both channels' sequences (host-side)"""
    x, y = C.c_int(), C.c_int()
    L = load()
    if L.mi_dv_mb_place(system, seq, slot, m, C.byref(x), C.byref(y)) != 0:
        raise MiDvError(L.mi_dv_last_error(None).decode())
    return x.value, y.value


def mb_place(system, seq, slot, m):
    """place_of for the four systems profile_of names.  To this function 3 stays no system, as to profile_of and system_of
    (tests/test_dv422_cpu.py holds it to that): SYS_625_50_411 goes through place_of, as its frames go through kind_of"""
    if system == SYS_625_50_411:
        raise MiDvError(f"mb_place: system {system} is place_of's (as kind_of is to profile_of)")
    return place_of(system, seq, slot, m)


def mb_rects(system, seq, slot, m):
    """the three rectangles (x, y, w, h) macroblock m of segment `slot` of sequence `seq` covers, of Y, Cb and Cr, each in
    its plane's own pixels; `seq` as place_of takes it (host-side)"""
    r = (C.c_int * 4 * 3)()
    L = load()
    if L.mi_dv_mb_rects(system, seq, slot, m, r) != 0:
        raise MiDvError(L.mi_dv_last_error(None).decode())
    return tuple(tuple(q) for q in r)


def held_macroblocks(frame, system, sta_mask=0):
    """how many macroblocks of a frame the mask holds: those whose STA nibble is a set bit of it (0: STA_ERRORS)
    (host-side)"""
    frame = np.ascontiguousarray(frame, np.uint8)
    L = load()
    n = L.mi_dv_held_macroblocks(system, frame.ctypes.data_as(u8p), frame.nbytes, sta_mask)
    if n < 0:
        raise MiDvError(L.mi_dv_last_error(None).decode())
    return n


class MiDv(Device):
    LIB = LIB

    @staticmethod
    def _planes(system, strides, planes=None):
        """(planes, their pointers, strides) as the one-frame calls take them; planes None: zeros of the system's picture,
        strides None: the system's plane widths"""
        planes_wh = geometry(system)[2]
        if strides is None:
            strides = tuple(w for w, _ in planes_wh)
        if planes is None:
            planes = [np.zeros(strides[i] * planes_wh[i][1], np.uint8) for i in range(3)]
        return planes, (u8p * 3)(*[p.ctypes.data_as(u8p) for p in planes]), (C.c_int * 3)(*strides)

    def decode_batch(self, d_frames, n, d_pics):
        self._chk(self.L.mi_dv_decode_batch(self.c, d_frames, n, d_pics))

    def decode_batch_sys(self, system, d_frames, n, d_pics):
        self._chk(self.L.mi_dv_decode_batch_sys(self.c, system, d_frames, n, d_pics))

    def kernel_times(self):
        """(total milliseconds, launches) of k_dv_decode since the last call"""
        return self._times(self.L.mi_dv_kernel_times)

    def decode_frames(self, frames, system=SYS_525_60):
        """host frames (n x the system's frame bytes, uint8) -> host pictures (n x its picture bytes), through the batch
        path (525/60: 120000 -> 518400; 625/50, 4:2:0 and 4:1:1: 144000 -> 622080; 4:2:2: 240000 -> 691200, 288000 -> 829440)"""
        fb, pb, _ = geometry(system)
        frames = np.ascontiguousarray(frames, np.uint8).reshape(-1, fb)
        n = frames.shape[0]
        with self._resident(frames, n * pb) as (df, dp):
            if system == SYS_525_60:
                self.decode_batch(df, n, dp)
            else:
                self.decode_batch_sys(system, df, n, dp)
            self.sync()
            return self.d2h(dp, n * pb).reshape(n, pb)

    def decode_frame(self, frame, strides=None, system=SYS_525_60):
        """one host frame into three planes of the given strides (default: the system's plane widths)"""
        frame = np.ascontiguousarray(frame, np.uint8)
        planes, pp, st = self._planes(system, strides)
        if system == SYS_525_60:
            self._chk(self.L.mi_dv_decode_frame(self.c, frame.ctypes.data_as(u8p), frame.nbytes, pp, st))
        else:
            self._chk(self.L.mi_dv_decode_frame_sys(self.c, system, frame.ctypes.data_as(u8p), frame.nbytes, pp, st))
        return planes

    # ---- macroblocks flagged as errors keep the stream's last good pixels (include/mi_dv.h) ----
    def decode_batch_held(self, system, d_frames, n, d_pics, runs=None, d_prev=None, sta_mask=0):
        """decode_batch_sys, then held macroblocks from the nearest earlier picture of their run in which they are good,
        else from the run's picture of d_prev (len(runs) pictures back to back on the device), else left as decoded.
        runs: the lengths of the runs of consecutive frames of one stream (None: one run)"""
        rl = (C.c_int * len(runs))(*runs) if runs else None
        self._chk(self.L.mi_dv_decode_batch_held(self.c, system, d_frames, n, d_pics, len(runs) if runs else 0, rl, d_prev, sta_mask))

    def decode_frames_held(self, frames, system, runs=None, prev=None, sta_mask=0):
        """host frames -> host pictures through decode_batch_held; prev: one host picture per run, or None"""
        fb, pb, _ = geometry(system)
        frames = np.ascontiguousarray(frames, np.uint8).reshape(-1, fb)
        n = frames.shape[0]
        if prev is not None:
            prev = np.ascontiguousarray(prev, np.uint8).reshape(len(runs) if runs else 1, pb)
        with self._resident(frames, n * pb, prev) as (df, dp, dq):
            self.decode_batch_held(system, df, n, dp, runs, dq, sta_mask)
            self.sync()
            return self.d2h(dp, n * pb).reshape(n, pb)

    def decode_frame_held(self, frame, system, strides=None, sta_mask=0):
        """decode_frame with held macroblocks from the picture of the frame this call decoded last (none: the first frame,
        after hold_reset, after a frame of another system or a refused one) -> (planes, macroblocks taken from it)"""
        frame = np.ascontiguousarray(frame, np.uint8)
        planes, pp, st = self._planes(system, strides)
        held = C.c_int()
        self._chk(self.L.mi_dv_decode_frame_held(self.c, system, frame.ctypes.data_as(u8p), frame.nbytes, pp, st, sta_mask,
                                                 C.byref(held)))
        return planes, held.value

    def hold_reset(self):
        self._chk(self.L.mi_dv_hold_reset(self.c))

    def hold_stats(self):
        """the macroblocks the last held batch took from another picture"""
        v = C.c_longlong()
        self._chk(self.L.mi_dv_hold_stats(self.c, C.byref(v)))
        return v.value

    def hold_times(self):
        """(total milliseconds, launches) of the hold pass since the last call; kernel_times keeps k_dv_decode's"""
        return self._times(self.L.mi_dv_hold_times)

    # ---- the encoder (include/mi_dv.h; parity unpinned like the decoder) ----
    def encode_batch(self, system, d_pics, n, d_frames, flags=3):
        """n resident pictures of the system -> n resident DIF frames, queued on the instance's stream.  flags: bit 0 lets
        blocks take the 2-4-8 transform, bit 1 gives them classes by content"""
        self._chk(self.L.mi_dv_encode_batch(self.c, system, d_pics, n, d_frames, flags))

    def encode_frames(self, pics, system, flags=3):
        """host pictures (n x the system's picture bytes, uint8) -> host frames (n x its frame bytes), through the batch path"""
        fb, pb, _ = geometry(system)
        pics = np.ascontiguousarray(pics, np.uint8).reshape(-1, pb)
        n = pics.shape[0]
        with self._resident(pics, n * fb) as (dp, df):
            self.encode_batch(system, dp, n, df, flags)
            self.sync()
            return self.d2h(df, n * fb).reshape(n, fb)

    def encode_frame(self, planes, system, strides=None, flags=3, cap=None):
        """one picture from three host planes of the given strides (default: the system's plane widths) -> one host frame;
        cap: the room offered for it (default: the system's frame bytes)"""
        fb = geometry(system)[0]
        planes, pp, st = self._planes(system, strides, [np.ascontiguousarray(p, np.uint8) for p in planes])
        cap = fb if cap is None else cap
        frame = np.zeros(max(cap, 1), np.uint8)
        self._chk(self.L.mi_dv_encode_frame(self.c, system, pp, st, frame.ctypes.data_as(u8p), cap, flags))
        return frame[:fb]

    def encode_times(self):
        """(total milliseconds, launches) of k_dv_encode since the last call; kernel_times keeps k_dv_decode's"""
        return self._times(self.L.mi_dv_encode_times)

    def encode_stats(self):
        """(segments per chosen quantisation number [16], levels the overflow rule dropped) of the last encoded batch"""
        hist, dropped = (C.c_longlong * 16)(), C.c_longlong()
        self._chk(self.L.mi_dv_encode_stats(self.c, hist, C.byref(dropped)))
        return np.array(hist[:], np.int64), dropped.value

    # ---- the sound of resident frames (include/mi_dv.h; parity unpinned like the host reader) ----
    def audio_batch(self, system, d_frames, n, d_pcm, pairs, d_info):
        """n resident frames -> d_pcm[n][pairs][AUDIO_PAIR_BYTES] (interleaved stereo int16) and d_info[n][4] int32 (samples
        per channel, rate, pairs carried, bits), queued on the instance's stream"""
        self._chk(self.L.mi_dv_audio_batch(self.c, system, d_frames, n, d_pcm, pairs, d_info))

    def write_audio_batch(self, system, d_frames, n, d_pcm, pairs, samplerate, samples):
        """16-bit PCM (the layout audio_batch writes) into the audio blocks of n resident frames; samples: one count per
        frame, each within the system's window at the rate"""
        samples = [int(s) for s in samples]
        if len(samples) != n:
            raise MiDvError(f"write_audio_batch: {len(samples)} sample counts for {n} frames")
        self._chk(self.L.mi_dv_audio_write_batch(self.c, system, d_frames, n, d_pcm, pairs, samplerate, (C.c_int * n)(*samples)))

    def extract_audio(self, frames, system, pairs=None):
        """host frames -> (info, pcm): info an (n, 4) int32 array as audio_batch writes it, pcm[i][k] pair k of frame i as
        an int16 view of samples x 2 (left, right), trimmed to the frame's samples (none where the frame has no sound).
        pairs: how many pairs to fetch (default: as many as the system can carry in 12-bit mode)"""
        fb = geometry(system)[0]
        frames = np.ascontiguousarray(frames, np.uint8).reshape(-1, fb)
        n = frames.shape[0]
        pairs = 2 * AUDIO_CHANNELS[system] if pairs is None else pairs
        with self._resident(frames, n * max(pairs, 1) * AUDIO_PAIR_BYTES, n * 16) as (df, dp, di):
            self.audio_batch(system, df, n, dp, pairs, di)
            self.sync()
            info = self.d2h(di, n * 16).view(np.int32).reshape(n, 4)
            raw = self.d2h(dp, n * pairs * AUDIO_PAIR_BYTES).view(np.int16).reshape(n, pairs, AUDIO_PAIR_BYTES // 4, 2)
        return info, [[raw[i, k, :max(int(info[i, 0]), 0)] for k in range(pairs)] for i in range(n)]

    def write_audio(self, frames, system, pcm, samplerate, samples=None):
        """host frames with 16-bit sound written into their audio blocks -> host frames.  pcm[i][k]: int16, samples x 2, of
        pair k of frame i (at least the system's channels; shorter than the frame's samples: silence follows); samples:
        one count per frame (default: audio_samples(system, samplerate, i))"""
        fb = geometry(system)[0]
        frames = np.ascontiguousarray(frames, np.uint8).reshape(-1, fb)
        n, pairs = frames.shape[0], AUDIO_CHANNELS[system]
        if samples is None:
            samples = [audio_samples(system, samplerate, i) for i in range(n)]
        img = np.zeros((n, pairs, AUDIO_PAIR_BYTES // 2), np.int16)
        for i in range(n):
            for k in range(pairs):
                a = np.ascontiguousarray(pcm[i][k], np.int16).ravel()[:AUDIO_PAIR_BYTES // 2]
                img[i, k, :a.size] = a
        with self._resident(frames, img) as (df, dp):
            self.write_audio_batch(system, df, n, dp, pairs, samplerate, samples)
            self.sync()
            return self.d2h(df, n * fb).reshape(n, fb)

    def audio_times(self):
        """(total milliseconds, launches) of k_dv_audio_extract and k_dv_audio_write since the last call"""
        return self._times(self.L.mi_dv_audio_times)

    # ---- timecode, recording date and time, aspect of resident frames (include/mi_dv.h; parity unpinned: the readers
    # restate the reference's, the packs written are this repository's reading of IEC 61834) ----
    def meta_batch(self, system, d_frames, n, d_meta):
        """n resident frames -> d_meta[n][META_INTS] int32 (64-byte aligned): found mask, timecode h m s f, drop flag,
        recording y m d, h m s, wide, the three packs' bytes 1..4; queued on the instance's stream"""
        self._chk(self.L.mi_dv_meta_batch(self.c, system, d_frames, n, d_meta))

    def write_meta_batch(self, system, d_frames, n, first_frame=0, drop=0, rec_seconds=-1, wide=0):
        """the subcode and VAUX blocks of n resident frames, rewritten whole: frame k gets the timecode of frame number
        first_frame + k and the recording time rec_seconds (from 1970-01-01, no time zone; negative: none) + k frames"""
        self._chk(self.L.mi_dv_meta_write_batch(self.c, system, d_frames, n, first_frame, drop, rec_seconds, wide))

    def extract_meta(self, frames, system):
        """host frames -> an (n, META_INTS) int32 array as meta_batch writes it"""
        fb = geometry(system)[0]
        frames = np.ascontiguousarray(frames, np.uint8).reshape(-1, fb)
        n = frames.shape[0]
        with self._resident(frames, n * META_INTS * 4) as (df, dm):
            self.meta_batch(system, df, n, dm)
            self.sync()
            return self.d2h(dm, n * META_INTS * 4).view(np.int32).reshape(n, META_INTS)

    def write_meta(self, frames, system, first_frame=0, drop=0, rec_seconds=-1, wide=0):
        """host frames with timecode, recording date and time and aspect written into their subcode and VAUX blocks ->
        host frames"""
        fb = geometry(system)[0]
        frames = np.ascontiguousarray(frames, np.uint8).reshape(-1, fb)
        n = frames.shape[0]
        with self._resident(frames) as (df,):
            self.write_meta_batch(system, df, n, first_frame, drop, rec_seconds, wide)
            self.sync()
            return self.d2h(df, n * fb).reshape(n, fb)

    def meta_times(self):
        """(total milliseconds, launches) of k_dv_meta_extract and k_dv_meta_write since the last call"""
        return self._times(self.L.mi_dv_meta_times)
