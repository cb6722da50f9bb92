"""k_dv_audio_extract and k_dv_meta_extract against what the reference's own lib/dvframe.c answered for the same frames:
tests/golden/dvframe_ref.json (written from oracle/_ref/libdvframe_ref.so by tests/golden/make_dvframe_ref.py; held to the
live reference, the host reader and the statements by tests/test_dvframe_fixtures_cpu.py).  No reference build and no
reference tree is read here.  Per system one launch of 16 frames for each pair count — the four (rate, quantisation)
modes over the extras {0, 1, 31, 62, 63}, a frame without a source pack, a frame with quantisation 2 — and one launch of
the 9 metadata frames.  Byte and integer equality."""
import numpy as np
import pytest

import dvaudio as A
import dvmeta as M
import dvref as R
from test_gpu_dv_audio import dev, dv, gpu_extract  # noqa: F401  (dev, dv: the device's fixtures)
from test_gpu_dv_meta import gpu_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return R.fixture()


@pytest.fixture(scope="module")
def sound_frames():
    frames = {s: R.audio_batch_frames(s) for s in A.SYSTEMS}
    for f in frames.values():
        f.setflags(write=False)
    return frames


@pytest.mark.parametrize("pairs", R.PAIR_COUNTS)
@pytest.mark.parametrize("system", A.SYSTEMS)
def test_sound_of_sixteen_frames_equals_the_reference_s(dev, fx, sound_frames, system, pairs):
    frames, rec = sound_frames[system], fx["audio"][str(system)]
    assert [R.sha(f) for f in frames] == rec["inputs"], "the frames are not the ones the reference was given"
    rec = rec["pairs"][str(pairs)]
    info, pcm = gpu_extract(dev, system, frames, pairs)
    assert info.shape == (16, 4) and pcm.shape == (16, pairs, A.PAIR_BYTES)
    print(f"system {system}, {pairs} pairs: samples {info[:, 0].tolist()}")
    assert info[:, 0].tolist() == rec["samples"], f"system {system}, {pairs} pairs: the samples column"
    for i in range(16):
        if R.sha(pcm[i]) != rec["pcm"][i]:
            want = A.extract(system, frames[i], pairs)[1]  # (the statement equals the reference: the fixture's CPU test)
            k, at = np.argwhere(pcm[i] != want)[0]
            raise AssertionError(f"system {system}, {pairs} pairs: the PCM of frame {i} is not the reference's; pair {k} byte {at} is "
                                 f"{pcm[i][k][at]:#x}, the statement has {want[k][at]:#x} ({(pcm[i] != want).sum()} bytes differ)")
    for r in fx["audio_raw"].values():  # one 16-bit and one 12-bit 525/60 frame byte for byte
        if (r["system"], r["pairs"]) == (system, pairs):
            got = pcm[r["frame"]]
            assert np.array_equal(got[:, :4 * r["samples"]].ravel(), R.unb64(r["bytes"])) and not got[:, 4 * r["samples"]:].any()


@pytest.mark.parametrize("system", M.SYSTEMS)
def test_metadata_of_nine_frames_equals_the_reference_s(dev, fx, system):
    pi, rec = R.PROFILE_OF[system], fx["meta"][str(system)]
    frames = R.meta_frames(pi)
    assert [R.sha(f) for f in frames] == rec["inputs"], "the frames are not the ones the reference was given"
    rows = gpu_rows(dev, system, frames)
    assert rows.shape == (9, M.INTS)
    for i, name in enumerate(R.META_NAMES):
        want = R.meta_fields(rec["rows"][i], R.SAR_WIDE[R.PROFILES[pi][0]])
        got = {k: int(rows[i][k]) & ~(M.HAS_CONTROL if k == M.FOUND else 0) for k in R.META_FIELDS}
        print(f"system {system}, {name}: {got}")
        assert got == want, f"system {system}, frame {i} ({name}): fields 0-4 and 6-12"
        assert bool(rows[i][M.FOUND] & M.HAS_CONTROL) == (frames[i][M.CONTROL_AT] == M.PACK_CONTROL), name
