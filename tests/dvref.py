"""The reference's own lib/dvframe.c beside this repository's DV frame readers.  TEST INFRASTRUCTURE ONLY.

oracle/Makefile builds lib/dvframe.c, where the reference tree is present, into oracle/_ref/libdvframe_ref.so against a
stand-in header and glue of this repository's own (oracle/dvframe_ref/); reference() loads it, have_reference() says
whether it is there.  host() loads csrc/dvframe_host.c's library.  The seeded frames below are shared by
tests/test_dvframe_reference_cpu.py (live reference), tests/golden/make_dvframe_ref.py (its recorded answers) and the
tests that hold the host reader, the statements and the kernels to those records.

WHERE THE REFERENCE HAS NO DEFINED ANSWER it is not asked (audio_defined, and the glue refuses the same cases):
  a rate field above 2          it indexes past audio_min_samples[3] and dv_audio_frequency[3]
  the 720p50 profile            12 DIF sequences, but the 10-row 525/60 shuffle table: rows 10 and 11 lie past it
  past the fourth pair buffer   12-bit sound on the two 1080 profiles, and on a 720p frame whose (frame[1] >> 2) & 3 is 0
  a NULL pair buffer            a 720p frame whose (frame[1] >> 2) & 3 is 0 starts at the third pair: with 1 or 2 pairs (of the
                                counts init_audio can set: 1, 2, 4) that pointer is NULL and the reference writes through it
  no profile                    every call but set_header dereferences the NULL profile
"""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

import dvaudio as A
import dvmeta as M
from pkg import ROOT

REF_SO = os.path.join(ROOT, "oracle", "_ref", "libdvframe_ref.so")
HOST_SO = os.path.join(os.environ.get("MI_SAN_LIBDIR") or os.path.join(ROOT, "gmerlin-avdecoder_amd", "lib"), "libmi_dvframe.so")
NO_PROFILE, UNDEFINED = -100, -101
PAIR_BYTES = 8192
u8p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)

# the nine profiles in the order of include/mi_dvframe.h's table: dsf, VAUX stype, DIF sequences a channel, channels, height
PROFILES = ((0, 0x00, 10, 1, 480), (1, 0x00, 12, 1, 576), (1, 0x00, 12, 1, 576), (0, 0x04, 10, 2, 480), (1, 0x04, 12, 2, 576),
            (0, 0x14, 10, 4, 1080), (1, 0x14, 12, 4, 1080), (0, 0x18, 10, 2, 720), (1, 0x18, 12, 2, 720))
SYSTEM_OF = {0: 0, 1: 1, 2: 3, 3: 4, 4: 5}  # profile -> the device's system number (the HD profiles are host-only)
PROFILE_OF = {s: p for p, s in SYSTEM_OF.items()}
P720P50 = 8
EXTRAS = (0, 1, 31, 62, 63)
PAIR_COUNTS = (1, 2, 4)
MODES = ((0, 0), (1, 0), (2, 0), (2, 1))  # (rate, quantisation) of the device launches


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).view(np.uint8).tobytes()).hexdigest()


def ptr(a):
    return a.ctypes.data_as(u8p)


# ------------------------------------------------------------------ the two libraries
def have_reference():
    return os.path.exists(REF_SO)


_ref = _host = None


def reference():
    global _ref
    if _ref is None:
        L = C.CDLL(REF_SO)
        L.mi_dvref_profile.argtypes = [u8p, i32p]
        L.mi_dvref_audio_format.argtypes = [u8p, i32p]
        L.mi_dvref_audio.argtypes = [u8p, C.c_int, u8p, i32p]
        L.mi_dvref_meta.argtypes = [u8p, i32p]
        _ref = L
    return _ref


def host():
    """csrc/dvframe_host.c's library with its argument types (what the fixture L of tests/test_dvframe_host.py sets up)"""
    global _host
    if _host is None:
        from test_dvframe_host import Profile
        so = os.path.join(ROOT, "gmerlin-avdecoder_amd", "lib", "libmi_dvframe.so")
        subprocess.run(["make", "-C", os.path.join(ROOT, "gmerlin-avdecoder_amd", "csrc"), so], check=True, capture_output=True)
        L, PP, ip = C.CDLL(HOST_SO), C.POINTER(Profile), C.POINTER(C.c_int)
        L.mi_dv_frame_profile.restype = L.mi_dv_profile_at.restype = PP
        L.mi_dv_frame_profile.argtypes = [u8p]
        L.mi_dv_extract_audio.argtypes = [PP, u8p, C.POINTER(u8p)]
        L.mi_dv_audio_12to16.restype, L.mi_dv_audio_12to16.argtypes = C.c_uint16, [C.c_uint16]
        L.mi_dv_audio_format.argtypes = [PP, u8p] + [ip] * 3
        L.mi_dv_pixel_aspect.argtypes = [PP, u8p, ip, ip]
        L.mi_dv_date.argtypes = L.mi_dv_time.argtypes = [PP, u8p] + [ip] * 3
        L.mi_dv_timecode.argtypes = [PP, u8p] + [ip] * 4
        _host = L
    return _host


def host_audio(pi, frame, pairs):
    """mi_dv_extract_audio into `pairs` zeroed buffers -> (its return value, uint8 [pairs][PAIR_BYTES])"""
    L, bufs = host(), np.zeros((pairs, PAIR_BYTES), np.uint8)
    arr = (u8p * 4)(*[ptr(bufs[k]) if k < pairs else None for k in range(4)])
    return L.mi_dv_extract_audio(L.mi_dv_profile_at(pi), ptr(frame), arr), bufs


def host_meta(pi, frame):
    """the host readers' answers in the order of ref_meta; what a reader that found nothing is given stays untouched"""
    L, out = host(), []
    pp = L.mi_dv_profile_at(pi)
    for fn, n in ((L.mi_dv_timecode, 4), (L.mi_dv_date, 3), (L.mi_dv_time, 3)):
        v = [C.c_int(-7) for _ in range(n)]
        found = fn(pp, ptr(frame), *[C.byref(x) for x in v])
        out += [found] + [x.value if found else 0 for x in v]
        assert found or all(x.value == -7 for x in v)
    num, den = C.c_int(), C.c_int()
    L.mi_dv_pixel_aspect(pp, ptr(frame), C.byref(num), C.byref(den))
    return out + [num.value, den.value]


# ------------------------------------------------------------------ the reference's answers
def ref_profile(header):
    """480 bytes -> None (no profile) or 12 ints: frame size, image width, height, pixel format class, frame duration,
    timescale, timecode rate, timecode drop flag, pixel aspect 4:3 (num, den), 16:9 (num, den)"""
    out = np.zeros(12, np.int32)
    r = reference().mi_dvref_profile(ptr(np.ascontiguousarray(header, np.uint8)), out.ctypes.data_as(i32p))
    assert r in (1, NO_PROFILE)
    return None if r == NO_PROFILE else out.tolist()


def ref_audio_format(frame):
    """what bgav_dv_dec_init_audio leaves in a zeroed format: [samplerate (0: untouched), channels, sample format,
    interleave mode, samples per frame, fourcc]"""
    out = np.zeros(6, np.int32)
    assert reference().mi_dvref_audio_format(ptr(frame), out.ctypes.data_as(i32p)) == 1
    return out.tolist()


def ref_audio(frame, pairs):
    """(dv_extract_audio's return value, what it wrote into `pairs` zeroed buffers: uint8 [pairs][PAIR_BYTES])"""
    pcm, n = np.zeros((pairs, PAIR_BYTES), np.uint8), np.zeros(1, np.int32)
    r = reference().mi_dvref_audio(ptr(frame), pairs, ptr(pcm), n.ctypes.data_as(i32p))
    assert r == 1, f"the glue refused ({r}): a case the rules leave out was asked"
    return int(n[0]), pcm


def ref_meta(frame):
    """15 ints: timecode found, h, m, s, f; date found, y, m, d; time found, h, m, s; pixel aspect num, den"""
    out = np.zeros(15, np.int32)
    assert reference().mi_dvref_meta(ptr(frame), out.ctypes.data_as(i32p)) == 1
    return out.tolist()


def meta_fields(r, sar_wide):
    """the reference's 15 ints as fields 0-4 and 6-12 of dvmeta.extract's row (FOUND without its control bit, which the
    reference does not tell; WIDE: whether the aspect it gives is the profile's 16:9 one)"""
    row = {M.FOUND: r[0] * M.HAS_TIMECODE | r[5] * M.HAS_DATE | r[9] * M.HAS_TIME}
    row.update(zip((M.TC_H, M.TC_M, M.TC_S, M.TC_F), r[1:5]))
    row.update(zip((M.YEAR, M.MONTH, M.DAY), r[6:9]))
    row.update(zip((M.HOUR, M.MINUTE, M.SECOND), r[10:13]))
    row[M.WIDE] = int(tuple(r[13:15]) == tuple(sar_wide))
    return row


META_FIELDS = (M.FOUND, M.TC_H, M.TC_M, M.TC_S, M.TC_F, M.YEAR, M.MONTH, M.DAY, M.HOUR, M.MINUTE, M.SECOND, M.WIDE)
SAR_WIDE = {0: (40, 33), 1: (118, 81)}  # by dsf, for the profiles of 480 and 576 lines (the HD ones: 1:1 either way)


# ------------------------------------------------------------------ where the reference is defined
def audio_defined(pi, frame, pairs):
    """the rules of this file's docstring for dv_extract_audio, in its order"""
    _, _, _, _, height = PROFILES[pi]
    as_ = frame[A.PACK_AT:A.PACK_AT + 5]
    has_pack = as_[0] == 0x50
    quant, rate = int(as_[4]) & 7, (int(as_[4]) >> 3) & 7
    if has_pack and quant <= 1 and rate > 2:
        return False
    if pi == P720P50:
        return False
    first_half = height == 720 and (int(frame[1]) >> 2) & 3 == 0
    twelve = has_pack and quant == 1
    if twelve and (height == 1080 or first_half):
        return False
    if first_half and pairs < 4:
        return False
    return True


# ------------------------------------------------------------------ seeded frames
def frame_bytes(pi):
    _, _, seqs, chans, _ = PROFILES[pi]
    return chans * seqs * 12000


def noise(pi, seed, half=1):
    """random bytes that announce profile pi (DSF, APT, VAUX stype); half: (frame[1] >> 2) & 3, which only 720p reads.
    The five profiles the device knows: dvaudio.noise_frame's bytes"""
    dsf, stype, _, _, _ = PROFILES[pi]
    if pi in SYSTEM_OF:
        f = A.noise_frame(SYSTEM_OF[pi], seed, 0, 0, 0)
        f[A.PACK_AT:A.PACK_AT + 5] = np.random.default_rng(seed + 1).integers(0, 256, 5, dtype=np.uint8)
    else:
        f = np.random.default_rng(seed).integers(0, 256, frame_bytes(pi), dtype=np.uint8)
        f[3] = (f[3] & 0x7F) | dsf << 7
        f[5] = (f[5] & 0xF8) | 1
        f[80 * 5 + 48 + 3] = (f[80 * 5 + 48 + 3] & 0xE0) | stype
    f[1] = (f[1] & 0xF3) | half << 2
    if f[A.PACK_AT] == 0x50:
        f[A.PACK_AT] = 0x51
    return f


def audio_frame(pi, rate, quant, extra, half=1, stype=0):
    """noise with a source pack: the frame of one case of the enumeration (the same frame for every pair count)"""
    return A.set_pack(noise(pi, 7000 + 1000 * pi + 100 * rate + 10 * quant + extra, half), extra, rate, quant, stype)


def audio_batch_frames(system):
    """the 16 frames of one device launch: the four (rate, quantisation) modes over the extras, 14 different pairs of
    them; frame 14 has no source pack, frame 15 quantisation 2"""
    pi = PROFILE_OF[system]
    frames = [audio_frame(pi, *MODES[i % 4], EXTRAS[i % 5]) for i in range(14)]
    frames.append(noise(pi, 7900 + pi))
    frames.append(A.set_pack(noise(pi, 7950 + pi), 17, 0, 2))
    return np.stack(frames)


def wiped(pi, f):
    """no subcode packet of any channel carries one of the three pack ids (dvmeta.noise_frame's rule)"""
    _, _, seqs, chans, _ = PROFILES[pi]
    for fs in range(chans * seqs):
        for c in range(12):
            at = M.place_at(fs, c // 6, c % 6)
            if f[at] in M.PLANTED_IDS:
                f[at] = 0xFF
    return f


def control(f, byte2, apt):
    """the VAUX source control pack mi_dv_pixel_aspect reads (byte2 None: no such pack there), and the APT of byte 4"""
    f[M.CONTROL_AT] = M.PACK_CONTROL if byte2 is not None else 0x60
    if byte2 is not None:
        f[M.CONTROL_AT + 2] = byte2
    f[4] = (f[4] & 0xF8) | apt
    return f


META_NAMES = ("first", "last", "several", "last sequence", "noise", "noise, wide", "none", "off-place", "second round")


def meta_frames(pi):
    """nine frames (META_NAMES): packs at the first and the last candidates of the scan, several hits of one id, hits in
    the last sequence only, noise as it falls (twice), nothing to find, the ids where no pack begins, a hit beyond the
    64th candidate; the control pack present and absent, saying 16:9 by either rule and not, with APT 0 and not 0"""
    _, _, seqs, _, _ = PROFILES[pi]
    last, seed = 12 * seqs - 1, 9000 + 100 * pi
    rng = np.random.default_rng(seed)
    tc, date, time = M.PLANTED_IDS
    out = []

    def fresh(k, wipe=True):
        f = noise(pi, seed + 1 + k)
        return wiped(pi, f) if wipe else f

    f = fresh(0)
    for c, pid in enumerate((tc, date, time)):
        M.plant(f, *M.place_of(c), M.some_pack(pid, rng))
    out.append(control(f, 0x02, 0))
    f = fresh(1)
    for c, pid in zip((last - 2, last - 1, last), (time, tc, date)):
        M.plant(f, *M.place_of(c), M.some_pack(pid, rng))
    out.append(control(f, 0x07, 0))
    f = fresh(2)
    for c, pid in ((3, tc), (63, tc), (64, tc), (last, tc), (70, date), (5, date), (100, time)):
        M.plant(f, *M.place_of(c), M.some_pack(pid, rng))
    out.append(control(f, 0x07, 3))
    f = fresh(3)
    for k, pid in ((1, date), (6, time), (11, tc)):
        M.plant(f, *M.place_of(12 * (seqs - 1) + k), M.some_pack(pid, rng))
    out.append(control(f, None, 0))
    out.append(fresh(4, wipe=False))
    out.append(control(fresh(5, wipe=False), 0xCA, 5))
    out.append(control(fresh(6), None, 2))
    f = fresh(7)
    for q in range(seqs):
        for j in range(2):
            for p in range(80):
                if p < 3 or p >= 51 or (p - 3) % 8 != 3:
                    f[M.block_at(q, j) + p] = M.PLANTED_IDS[(q + j + p) % 3]
    out.append(control(f, 0xC8, 0))
    f = fresh(8)
    M.plant(f, *M.place_of(64), M.some_pack(date, rng))
    M.plant(f, *M.place_of(last - 12), M.some_pack(tc, rng))
    out.append(control(f, 0xFF, 1))
    assert len(out) == len(META_NAMES)
    return np.stack(out)


# ------------------------------------------------------------------ the reference's recorded answers (tests/golden/dvframe_ref.json)
FIXTURE = os.path.join(ROOT, "tests", "golden", "dvframe_ref.json")
RAW_FRAMES = {"16-bit": (0, 0, 1), "12-bit": (0, 3, 2)}  # 525/60: (system, frame of its launch, pairs) kept as bytes


def b64(a):
    import base64
    return base64.b64encode(np.ascontiguousarray(a).view(np.uint8).tobytes()).decode()


def unb64(s):
    import base64
    return np.frombuffer(base64.b64decode(s), np.uint8)


def records(audio_of, meta_of):
    """the fixture's content from two answerers: audio_of(pi, frame, pairs) -> (samples, pcm [pairs][PAIR_BYTES]) and
    meta_of(pi, frame) -> dvref.ref_meta's 15 ints.  With the reference's (ref_records) it is what the file holds; with the
    host reader's it must come out the same"""
    out = {"audio": {}, "audio_raw": {}, "meta": {}}
    for system, pi in PROFILE_OF.items():
        frames = audio_batch_frames(system)
        a = out["audio"][str(system)] = {"inputs": [sha(f) for f in frames], "pairs": {}}
        for pairs in PAIR_COUNTS:
            got = [audio_of(pi, f, pairs) for f in frames]
            a["pairs"][str(pairs)] = {"samples": [int(n) for n, _ in got], "pcm": [sha(p) for _, p in got]}
            for name, (s, k, np_) in RAW_FRAMES.items():
                if (s, np_) == (system, pairs):
                    n, pcm = got[k]
                    assert n > 0 and not pcm[:, 4 * n:].any()
                    out["audio_raw"][name] = {"system": s, "frame": k, "pairs": np_, "samples": int(n), "bytes": b64(pcm[:, :4 * n])}
        frames = meta_frames(pi)
        out["meta"][str(system)] = {"inputs": [sha(f) for f in frames], "rows": [[int(v) for v in meta_of(pi, f)] for f in frames]}
    return out


def ref_records():
    return records(lambda pi, f, pairs: ref_audio(f, pairs), lambda pi, f: ref_meta(f))


def fixture():
    import json
    with open(FIXTURE) as f:
        return json.load(f)
