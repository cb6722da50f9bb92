"""tests/golden/dvframe_ref.json — the answers of the reference's own lib/dvframe.c for the seeded frames of the device
launches (tests/dvref.py; written by tests/golden/make_dvframe_ref.py) — held to the live reference where
oracle/_ref has it, and everywhere to the host reader csrc/dvframe_host.c and to the statements tests/dvaudio.py and
tests/dvmeta.py, which is what lets tests/test_gpu_dv_reference.py compare the kernels with the file alone."""
import os

import numpy as np
import pytest

import dvaudio as A
import dvmeta as M
import dvref as R


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


@pytest.mark.skipif(not R.have_reference(), reason="oracle/_ref/libdvframe_ref.so is not built (no reference tree)")
def test_the_file_is_what_the_live_reference_answers(fx):
    assert fx == R.ref_records()


def test_the_file_is_what_the_host_reader_answers(fx):
    """input hashes included: the generators have not drifted"""
    got = R.records(R.host_audio, R.host_meta)
    for part in ("audio", "audio_raw", "meta"):
        for key in fx[part]:
            assert got[part][key] == fx[part][key], (part, key)
    assert got == fx


def test_what_the_file_holds(fx):
    assert os.path.getsize(R.FIXTURE) < 100000
    assert sorted(fx["audio"]) == sorted(fx["meta"]) == sorted(str(s) for s in A.SYSTEMS)
    for system in A.SYSTEMS:
        a, s = fx["audio"][str(system)], A.SOUND[system]
        assert len(a["inputs"]) == 16 and len(set(a["inputs"])) == 16 and sorted(a["pairs"]) == ["1", "2", "4"]
        want = [s.min_samples[R.MODES[i % 4][0]] + R.EXTRAS[i % 5] for i in range(14)] + [0, -1]
        for pairs in a["pairs"].values():
            assert pairs["samples"] == want and len(pairs["pcm"]) == 16
        assert len({(R.MODES[i % 4], R.EXTRAS[i % 5]) for i in range(14)}) == 14
        m = fx["meta"][str(system)]
        assert len(m["inputs"]) == len(m["rows"]) == 9 and all(len(r) == 15 for r in m["rows"])
    raw = fx["audio_raw"]
    assert (raw["16-bit"]["system"], raw["12-bit"]["system"]) == (0, 0) and raw["12-bit"]["pairs"] == 2
    for name, bits in (("16-bit", 0), ("12-bit", 1)):
        r = raw[name]
        assert R.MODES[r["frame"] % 4][1] == bits and R.unb64(r["bytes"]).size == r["pairs"] * 4 * r["samples"]


@pytest.mark.parametrize("system", A.SYSTEMS)
def test_the_statement_of_the_sound_answers_the_same(fx, system):
    a = fx["audio"][str(system)]
    frames = R.audio_batch_frames(system)
    assert [R.sha(f) for f in frames] == a["inputs"]
    for pairs in R.PAIR_COUNTS:
        rec = a["pairs"][str(pairs)]
        for i, f in enumerate(frames):
            info, pcm = A.extract(system, f, pairs)
            assert int(info[0]) == rec["samples"][i] and R.sha(pcm) == rec["pcm"][i], (system, pairs, i)
    for r in fx["audio_raw"].values():
        if r["system"] == system:
            _, pcm = A.extract(system, frames[r["frame"]], r["pairs"])
            assert np.array_equal(pcm[:, :4 * r["samples"]].ravel(), R.unb64(r["bytes"])) and not pcm[:, 4 * r["samples"]:].any()


@pytest.mark.parametrize("system", M.SYSTEMS)
def test_the_statement_of_the_metadata_answers_the_same(fx, system):
    m = fx["meta"][str(system)]
    pi = R.PROFILE_OF[system]
    frames = R.meta_frames(pi)
    assert [R.sha(f) for f in frames] == m["inputs"]
    for f, rec, name in zip(frames, m["rows"], R.META_NAMES):
        row = M.extract(system, f)
        want = R.meta_fields(rec, R.SAR_WIDE[R.PROFILES[pi][0]])
        assert {k: int(row[k]) & ~(M.HAS_CONTROL if k == M.FOUND else 0) for k in R.META_FIELDS} == want, (system, name)
