"""The DV frame readers against the reference's own lib/dvframe.c, compiled as it stands into
oracle/_ref/libdvframe_ref.so (tests/dvref.py; skipped only where that library is absent): profile detection, the audio
de-shuffle, the audio format, timecode, date, time and pixel aspect of csrc/dvframe_host.c, and with them the statements
the device kernels are held to (tests/dvaudio.py, tests/dvmeta.py) and np_extract_audio of tests/test_dvframe_host.py.
Everything is integer or byte equality.  Where the reference has no defined answer (tests/dvref.py's docstring) a case is
left out by rule, and every test asserts the number of cases it did compare, worked out from the enumeration and the
rules."""
import ctypes as C

import numpy as np
import pytest

import dvaudio as A
import dvmeta as M
import dvref as R
from test_dvframe_host import np_extract_audio

pytestmark = pytest.mark.skipif(not R.have_reference(), reason="oracle/_ref/libdvframe_ref.so is not built (no reference tree)")
NPROF = len(R.PROFILES)


@pytest.fixture(scope="module")
def L():
    return R.host()


def ints(n):
    return [C.c_int(-7) for _ in range(n)]


def refs(v):
    return [C.byref(x) for x in v]


# ------------------------------------------------------------------ the profile table
def test_profile_of_every_header(L):
    compared = found = 0
    seen = set()
    for dsf in (0, 1):
        for stype in range(32):
            for apt in (0, 1):
                h = np.zeros(480, np.uint8)
                h[3], h[80 * 5 + 48 + 3], h[5] = dsf << 7, stype, apt
                want, got = R.ref_profile(h), L.mi_dv_frame_profile(R.ptr(h))
                what = f"dsf {dsf}, stype {stype:#x}, frame[5] & 7 = {apt}"
                assert (want is None) == (not got), what
                compared += 1
                if want is None:
                    continue
                found += 1
                p = got.contents
                seen.add((p.frame_size, p.width, p.height, p.pix_fmt))
                ours = [p.frame_size, p.width, p.height, p.pix_fmt, p.frame_rate_base, p.frame_rate, p.ltc_divisor,
                        int(p.frame_rate_base == 1001), p.sar[0][0], p.sar[0][1], p.sar[1][0], p.sar[1][1]]
                assert ours == want, what
    # 2 x 32 x 2 headers; with a profile: stypes 0, 4, 0x14, 0x18 of both line systems at both APT values
    assert (compared, found) == (128, 2 * 4 * 2) and len(seen) == NPROF


# ------------------------------------------------------------------ the audio de-shuffle
def host_audio(L, pi, frame, pairs):
    return R.host_audio(pi, frame, pairs)


def same_four_ways(L, pi, frame, pairs, what):
    """the reference, the host reader, np_extract_audio and (for the five systems of the device) dvaudio.extract"""
    assert L.mi_dv_frame_profile(R.ptr(frame)).contents.frame_size == R.frame_bytes(pi), what
    n, want = R.ref_audio(frame, pairs)
    got_n, got = host_audio(L, pi, frame, pairs)
    assert got_n == n, what
    if not np.array_equal(got, want):
        k, at = np.argwhere(got != want)[0]
        raise AssertionError(f"{what}: mi_dv_extract_audio differs in pair {k} at byte {at}: {got[k][at]:#x}, the reference {want[k][at]:#x}")
    if n > 0:  # (np_extract_audio has no early answers: it restates the loop)
        np_n, np_bufs = np_extract_audio(L.mi_dv_profile_at(pi).contents, frame, [k < pairs for k in range(4)])
        assert np_n == n, what
        for k in range(pairs):
            w = np_bufs[k][:R.PAIR_BYTES]
            written = w != 0xCD
            assert np.array_equal(want[k][written], w[written]) and np.isin(want[k][~written], (0, 0xCD)).all(), (what, "np_extract_audio", k)
            assert (np_bufs[k][R.PAIR_BYTES:] == 0xCD).all(), what
    if pi in R.SYSTEM_OF:
        info, pcm = A.extract(R.SYSTEM_OF[pi], frame, pairs)
        assert info[0] == n and np.array_equal(pcm, want), (what, "dvaudio.extract")
    return n, want


def halves_of(pi):
    return (0, 1) if R.PROFILES[pi][4] == 720 else (1,)


@pytest.mark.parametrize("pi", range(NPROF))
def test_audio_of_every_mode(L, pi):
    compared = 0
    for half in halves_of(pi):
        for rate in range(3):
            for quant in (0, 1):
                for extra in R.EXTRAS:
                    f = R.audio_frame(pi, rate, quant, extra, half)
                    for pairs in R.PAIR_COUNTS:
                        if not R.audio_defined(pi, f, pairs):
                            continue
                        n, pcm = same_four_ways(L, pi, f, pairs, f"profile {pi}, rate {rate}, quantisation {quant}, extra {extra}, {pairs} pairs, half {half}")
                        assert n == L.mi_dv_profile_at(pi).contents.audio_min_samples[rate] + extra and pcm.any()
                        compared += 1
    height = R.PROFILES[pi][4]
    all_modes = 3 * 2 * len(R.EXTRAS) * len(R.PAIR_COUNTS)
    # 480 and 576 lines: everything.  1080: 16-bit only.  720p60: a second half frame everything, a first half frame
    # 16-bit into four pairs only.  720p50: nothing
    want = {480: all_modes, 576: all_modes, 1080: all_modes // 2, 720: 0 if pi == R.P720P50 else all_modes + 3 * len(R.EXTRAS)}[height]
    assert compared == want


@pytest.mark.parametrize("pi", range(NPROF))
def test_audio_frames_that_answer_early(L, pi):
    """no source pack: 0; quantisation 2 and above: -1; nothing written either way"""
    compared = 0
    for half in halves_of(pi):
        frames = [R.noise(pi, 7900 + pi, half)] + [A.set_pack(R.noise(pi, 7950 + pi + q, half), 17, r, q) for q, r in ((2, 0), (7, 1), (3, 5))]
        for f, want_n in zip(frames, (0, -1, -1, -1)):
            for pairs in R.PAIR_COUNTS:
                if not R.audio_defined(pi, f, pairs):
                    continue
                n, pcm = same_four_ways(L, pi, f, pairs, f"profile {pi}, half {half}: a frame that answers {want_n}")
                assert n == want_n and not pcm.any()
                compared += 1
    # 720p50 is out; a first half frame of 720p60 only with four pairs
    assert compared == {720: 0 if pi == R.P720P50 else 4 * 3 + 4}.get(R.PROFILES[pi][4], 4 * 3)


@pytest.mark.parametrize("system", (4, 5))
def test_every_twelve_bit_code_in_both_positions(L, system):
    """pins mi_dv_audio_12to16, written from the companding law, to the reference's arithmetic: all 4096 codes, left and right"""
    f = A.all_codes_frame(system, 3, 63)
    n, pcm = same_four_ways(L, R.PROFILE_OF[system], f, 4, f"system {system}: every code")
    s = A.SOUND[system]
    t = np.arange(4096)
    c, q, j, k = t // (216 * s.seqs), t // 216 % s.seqs, t // 24 % 9, t % 24
    half = s.seqs // 2
    v = pcm.view("<u2").reshape(4, A.SLOTS)
    left = v[2 * c + q // half, s.shuffle[q % half, j] + k * s.stride]
    right = v[2 * c + q // half, s.shuffle[q % half + half, j] + k * s.stride]
    ours = np.array([0 if code == 0x800 else L.mi_dv_audio_12to16(code) for code in range(4096)], np.uint16)
    assert np.array_equal(left, ours) and np.array_equal(right, ours[(t * 2731 + 1) & 0xFFF])
    assert n == s.min_samples[2] + 63


def test_audio_format_of_every_pack(L):
    compared = 0
    for pi in range(NPROF):
        pp = L.mi_dv_profile_at(pi)
        f = R.audio_frame(pi, 0, 0, 5)
        for rate in range(3):  # (a rate above 2: left out by rule)
            for quant in range(8):
                for stype in (0, 1, 2, 3, 31):
                    f[A.PACK_AT + 3], f[A.PACK_AT + 4] = 0xC0 | stype, 0x80 | rate << 3 | quant
                    want = R.ref_audio_format(f)
                    sr, ch, mx = ints(3)
                    assert L.mi_dv_audio_format(pp, R.ptr(f), *refs((sr, ch, mx))) == 1
                    assert [sr.value, 2 * ch.value, mx.value] == [want[0], want[1], want[4]], (pi, rate, quant, stype)
                    assert want[2:4] == [3, 2 if ch.value == 1 else 1]  # S16; interleaved in all / in pairs
                    compared += 1
        f = R.noise(pi, 7900 + pi)  # no source pack: the format is left alone
        sr, ch, mx = ints(3)
        assert R.ref_audio_format(f)[:5] == [0] * 5 and L.mi_dv_audio_format(pp, R.ptr(f), *refs((sr, ch, mx))) == 0
        assert (sr.value, ch.value, mx.value) == (-7, -7, -7)
        compared += 1
    assert compared == NPROF * (3 * 8 * 5 + 1)


# ------------------------------------------------------------------ timecode, date, time, aspect
def host_meta(L, pi, frame):
    return R.host_meta(pi, frame)


def same_meta(L, pi, frame, what):
    want = R.ref_meta(frame)
    assert host_meta(L, pi, frame) == want, what
    if pi in R.SYSTEM_OF:
        row = M.extract(R.SYSTEM_OF[pi], frame)
        fields = R.meta_fields(want, R.SAR_WIDE[R.PROFILES[pi][0]])
        assert {k: int(row[k]) & ~(M.HAS_CONTROL if k == M.FOUND else 0) for k in R.META_FIELDS} == fields, (what, "dvmeta.extract")
        assert bool(row[M.FOUND] & M.HAS_CONTROL) == (frame[M.CONTROL_AT] == M.PACK_CONTROL), what
    return want


@pytest.mark.parametrize("pi", range(NPROF))
def test_meta_of_the_nine_frames(L, pi):
    rows = [same_meta(L, pi, f, f"profile {pi}: {name}") for name, f in zip(R.META_NAMES, R.meta_frames(pi))]
    assert len(rows) == 9
    by = dict(zip(R.META_NAMES, rows))
    sar = [L.mi_dv_profile_at(pi).contents.sar[k][:] for k in (0, 1)]
    # the frames are what their names say: the cases are there, whoever answers
    for name in ("first", "last", "several", "last sequence"):
        assert (by[name][0], by[name][5], by[name][9]) == (1, 1, 1), name
    assert (by["none"][0], by["none"][5], by["none"][9]) == (0, 0, 0) == (by["off-place"][0], by["off-place"][5], by["off-place"][9])
    assert (by["second round"][0], by["second round"][5], by["second round"][9]) == (1, 1, 0)
    assert [by[n][13:15] for n in ("first", "last", "noise, wide")] == [sar[1]] * 3  # 16:9 by either rule
    assert [by[n][13:15] for n in ("several", "last sequence", "none", "off-place", "second round")] == [sar[0]] * 5


@pytest.mark.parametrize("system", M.SYSTEMS)
def test_meta_of_dvmeta_s_planted_frames(L, system):
    m = M.META[system]
    last = m.places - 1
    names = ["alone 0", "alone 1", "alone 2", "alone 4", "alone 8", f"alone {last}", f"alone {last - 1}", f"alone {12 * (m.seqs - 1)}",
             "two 0 1", "two 63 64", f"two 0 {last}", f"two 70 {last}", "off-place"] + (["channel 1"] if m.chans == 2 else [])
    assert set(names) <= set(M.planted_names(system))
    found = 0
    for name in names:
        found += sum(same_meta(L, R.PROFILE_OF[system], M.planted_frame(system, name), f"system {system}: {name}")[k] for k in (0, 5, 9))
    for seed in (1, 2):  # unwiped noise
        same_meta(L, R.PROFILE_OF[system], M.noise_frame(system, seed, wiped=False), f"system {system}: noise {seed}")
    # every "alone" frame has one pack, every "two" frame its id (twice) and another: 8 + 4 * 2 hits
    assert found == 8 + 4 * 2
