"""The integer statement of the DV encoder (tests/dvenc.py), checked without a GPU against code that shares nothing with
it: the float statement's bit-serial parser and frame writer (the bit layout), a numpy double transform with dvf_weight and
dvf_shift (the arithmetic), dvf_block_bits (the rate control), and both existing encoders (the quality).  The recorded
figures are tests/golden/dv_encode_bounds.json (make_dv_encode_bounds.py).  THE DROP-RULE PICTURE is dvenc.drop_picture:
on it the statement drops levels in the segments of every second DIF sequence and in no other.  PARITY UNPINNED."""
import ctypes as C
import importlib

import numpy as np
import pytest

import dvenc as E
import dvenc_check as K
import dvfloat as F
import dvlib as D
import dvsys as S

ERR_ARG = -1


# ---- the bit layout ----
@pytest.mark.parametrize("name,flags", K.FRAMES)
def test_the_float_writer_rewrites_a_statement_frame_and_its_parser_reads_what_the_statement_chose(name, flags):
    fr, rec = K.stated(name, flags)
    qno, dc, mode, cls, levels = F.parse(fr)
    assert np.array_equal(F.write_frame(qno, dc, mode, cls, levels), fr)
    assert np.array_equal(qno, np.repeat(rec["qno"], 5))
    assert np.array_equal(dc, rec["dc"]) and np.array_equal(mode, rec["mode"]) and np.array_equal(cls, rec["cls"])
    assert np.array_equal(levels[:, 1:], rec["levels"][:, 1:])


def test_a_single_segment_is_the_frames():
    """segment(), the unit, on the pixels of one segment of a frame: the same five DIF blocks"""
    fr, _ = K.stated("n8", 3)
    s = 27 * 4 + 11
    blocks = E.segment(K.picture("n8")[E.block_map()[30 * s:30 * s + 30]], 3)
    for m in range(5):
        o = D.video_block_offset(s // 27, 5 * (s % 27) + m)
        assert np.array_equal(blocks[m, 3:], fr[o + 3:o + 80])


# ---- the arithmetic ----
@pytest.mark.parametrize("name,flags", K.FRAMES)
def test_a_level_is_never_a_whole_step_off_the_closed_form(name, flags):
    worst = K.deviation(name, flags)
    print(f"{name}/{flags}: worst |level - F W / 2^s| = {worst:.4f}")
    assert worst < 1.0
    assert worst <= K.bounds()["deviation"][f"{name}/{flags}"]


def test_a_halved_multiplier_fails_the_closed_form(monkeypatch):
    mult = E.MULT.copy()
    mult[0, 9] //= 2
    monkeypatch.setattr(E, "MULT", mult)
    assert K.deviation("n8", 2) >= 1.0


# ---- rate control ----
@pytest.mark.parametrize("name,flags", K.FRAMES)
def test_every_segment_fits_and_the_next_quantisation_number_would_not(name, flags):
    fr, rec = K.stated(name, flags)
    levels = F.parse(fr)[4]
    bits = np.array([F.block_bits(lv) for lv in levels])
    assert np.array_equal(bits, E.block_bits(rec["levels"]))  # the statement counts as the float writer does
    assert bits.reshape(-1, 30).sum(axis=1).max() <= E.SEGMENT_AC_BITS
    px = K.picture(name)[E.block_map()]
    P, neg = E.products(E.transform(px, rec["mode"]), rec["mode"])
    finer = np.minimum(rec["qno"] + 1, 15)
    again = E.block_bits(E.quantise(P, neg, rec["cls"], np.repeat(finer, 30))).reshape(-1, 30).sum(axis=1)
    assert ((again > E.SEGMENT_AC_BITS) | (rec["qno"] == 15)).all()


def test_the_drop_rule_picture_drops_in_some_segments_and_not_in_all():
    _, rec = K.stated("drop", 3)
    dropping = rec["dropped"] > 0
    assert 0 < dropping.sum() < dropping.size
    assert (rec["qno"][dropping] == 0).all()
    assert np.array_equal(dropping, (np.arange(270) // 27) % 2 == 0)  # the segments of every second DIF sequence


def test_census():
    recs = [K.stated(name, flags)[1] for name, flags in K.FRAMES]
    cls, mode, qno = (np.concatenate([r[k] for r in recs]) for k in ("cls", "mode", "qno"))
    assert set(np.unique(cls)) == {0, 1, 2, 3} and set(np.unique(mode)) == {0, 1}
    assert (qno == 15).any() and (qno <= 3).any()
    # every class and both modes on dvsys.synth pictures alone
    for system in (S.SYS_625_50, S.SYS_625_50_411):
        rec = []
        E.encode(system, S.synth(system, 0, 1, 8), 3, rec)
        assert set(np.unique(np.concatenate([r["cls"] for r in rec]))) == {0, 1, 2, 3}
        assert set(np.unique(np.concatenate([r["mode"] for r in rec]))) == {0, 1}
    assert (K.stated("n8", 3)[1]["qno"] <= 3).all() and (K.stated("flat", 3)[1]["qno"] == 15).all()


# ---- quality ----
@pytest.mark.parametrize("name", K.NAMES)
def test_the_statement_is_as_good_as_the_lower_of_the_existing_encoders(name):
    p = K.psnr_525(name)
    rec = K.bounds()["psnr"][name]
    print(f"{name}: statement {p[0]:.3f} dB, oracle encoder {p[1]:.3f}, float encoder {p[2]:.3f}; recorded shortfall {rec['shortfall']}")
    assert p[0] >= min(p[1], p[2]) - rec["shortfall"]
    assert rec["shortfall"] == K.shortfall((rec["statement"], rec["oracle"], rec["float"]))


@pytest.mark.parametrize("system", [s for s in S.SYSTEMS if s != S.SYS_525_60])
def test_the_other_systems(system):
    dv = importlib.import_module("gmerlin-avdecoder_amd.dv")
    p = K.psnr_system(system)
    rec = K.bounds()["systems"][str(system)]
    print(f"system {system}: statement {p[0]:.3f} dB, oracle encoder {p[1]:.3f}, float encoder {p[2]:.3f}")
    assert p[0] >= min(p[1], p[2]) - rec["shortfall"]
    frame = S.encode(system, S.synth(system, 0, 1, 8), 3, encode525=E.encode525)
    assert dv.kind_of(frame) == system


def test_a_525_frame_announces_525():
    dv = importlib.import_module("gmerlin-avdecoder_amd.dv")
    assert dv.kind_of(K.stated("flat", 0)[0]) == S.SYS_525_60


# ---- the ABI ----
def test_the_encoder_is_exported_and_refuses_without_a_device():
    dv = importlib.import_module("gmerlin-avdecoder_amd.dv")
    L = dv.load()
    for name in ("mi_dv_encode_batch", "mi_dv_encode_frame", "mi_dv_encode_times", "mi_dv_encode_stats"):
        assert name in dv.EXPORTS and hasattr(L, name)
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    assert L.mi_dv_encode_batch(None, 0, p, 1, p + 32, 3) == ERR_ARG
    assert b"mi_dv_encode_batch" in L.mi_dv_last_error(None)
    assert L.mi_dv_encode_batch(None, 2, p, 1, p + 32, 3) == ERR_ARG
    assert b"unknown system 2" in L.mi_dv_last_error(None)
    planes = (dv.u8p * 3)(*[buf.ctypes.data_as(dv.u8p)] * 3)
    strides = (C.c_int * 3)(720, 180, 180)
    assert L.mi_dv_encode_frame(None, 0, planes, strides, buf.ctypes.data_as(dv.u8p), 120000, 3) == ERR_ARG
    assert L.mi_dv_encode_frame(None, 7, planes, strides, buf.ctypes.data_as(dv.u8p), 120000, 3) == ERR_ARG
    ms, n, hist, dropped = C.c_float(), C.c_int(), (C.c_longlong * 16)(), C.c_longlong()
    assert L.mi_dv_encode_times(None, C.byref(ms), C.byref(n)) == ERR_ARG
    assert L.mi_dv_encode_stats(None, hist, C.byref(dropped)) == ERR_ARG
