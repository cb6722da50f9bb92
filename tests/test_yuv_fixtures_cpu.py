"""tests/golden/yuv_ref.json — what the reference's own lib/video_yuv.c makes of the seeded packets of the GPU suite's
cases (tests/yuvref.py; written by tests/golden/make_yuv_ref.py) — held to the live reference where oracle/_ref has it and
everywhere to the statement tests/yuvraw.py, which is what lets tests/test_gpu_yuv_reference.py compare the kernels with
the file alone."""
import os

import pytest

import yuvraw as Y
import yuvref as R


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


@pytest.mark.skipif(not R.have_reference(), reason="oracle/_ref/libvideo_yuv_ref.so is not built (no reference tree)")
def test_the_file_is_what_the_live_reference_answers(fx):
    assert fx == R.ref_records()


def test_the_file_is_what_the_statement_answers(fx):
    """packet hashes included: the generator has not drifted"""
    got = R.records(Y.unpack)
    for key in fx:
        assert got[key] == fx[key], key
    assert got == fx


def test_what_the_file_holds(fx):
    assert os.path.getsize(R.FIXTURE) < 100000
    assert sorted(fx) == sorted(R.case_id(*c) for c in R.CASES) and len(fx) == 43
    raw = hashed = 0
    for codec, w, h in R.CASES:
        rec = fx[R.case_id(codec, w, h)]
        assert len(rec["packets"]) == len(rec["pictures"]) == R.PACKETS and len(set(rec["packets"])) == R.PACKETS
        small = Y.layout(codec, w, h).picture_bytes <= R.RAW_LIMIT
        assert all(("bytes" in p) == small and ("sha256" in p) != small for p in rec["pictures"]), (codec, w, h)
        raw, hashed = raw + small, hashed + (not small)
    assert raw and hashed
