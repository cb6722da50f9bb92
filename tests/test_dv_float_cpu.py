"""The fixed-point DV statement (oracle/dv_oracle.c) against an independent floating-point statement of the same
closed form (oracle/dv_float.c through tests/dvfloat.py): restated tables, the gain of every scan position, DC, random
symbol blocks, whole frames three encoders apart, both systems — and that the recorded bounds have teeth.

PARITY UNPINNED.  These tests pin the fixed-point arithmetic (14-bit multipliers folded with a scaled transform's
factors, an 8-bit butterfly, int16 coefficients) to the closed form in dv_oracle.c's header comment.  They do not pin
the closed form to the standard, nor the bit layout to anything beyond the repository's own parsers.

The bounds are read from tests/golden/dv_float_bounds.json (generator: tests/golden/make_dv_float_bounds.py): the
oracle's measured worst case on these very inputs, rounded up to 0.25 level / 0.1 % gain / 0.01 level of mean, no margin."""
import ctypes as C

import numpy as np
import pytest

import dvfloat as F
import dvlib as D

B = F.bounds()


# ---- the restated constant data equals the oracle's ----
def test_restated_scan_orders_shifts_and_areas_are_the_oracles():
    for mode in (0, 1):
        a, b = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
        D.lib().dvo_scan(mode, D.p8(a))
        F.lib().dvf_scan(mode, D.p8(b))
        assert np.array_equal(a, b), mode
    areas = [F.lib().dvf_area(k) for k in range(64)]
    assert areas == [0] * 6 + [1] * 15 + [2] * 22 + [3] * 21
    for qno in range(16):
        for cls in range(4):
            for area in range(4):
                assert D.lib().dvo_shift(qno, cls, area) == F.lib().dvf_shift(qno, cls, area) + 1, (qno, cls, area)


def test_restated_variable_length_code_is_the_oracles_for_every_16_bits():
    ln, run, lv = C.c_int(), C.c_int(), C.c_int()
    for w in range(65536):
        eob = F.lib().dvf_vlc_lookup(w, C.byref(ln), C.byref(run), C.byref(lv))
        assert (ln.value, run.value, lv.value, bool(eob)) == D.vlc(w), w


def test_restated_placement_and_block_offsets_are_the_oracles():
    x, y, fx, fy = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    for seq in range(10):
        for slot in range(27):
            for m in range(5):
                D.lib().dvo_mb_place(seq, slot, m, C.byref(x), C.byref(y))
                F.lib().dvf_mb_place(seq, slot, m, C.byref(fx), C.byref(fy))
                assert (x.value, y.value) == (fx.value, fy.value), (seq, slot, m)
        for v in range(135):
            assert F.lib().dvf_block_offset(seq, v) == D.video_block_offset(seq, v)
    assert tuple(F.lib().dvf_area_offset(j) for j in range(6)) == D.AREA_OFF


def test_the_three_parsers_read_the_same_symbols():
    """the bit-serial parser reads back the symbols a frame was written from, and dvo_segment_coefs' reconstructed
    coefficients are zero where it read no level and nonzero where it read one of at least 4 (a smaller level at a high
    frequency can round to a zero coefficient)"""
    dif, (qno, dc, mode, cls, levels) = F.symbol_frame(F.SEEDS["symbol_frames"][0])
    q2, dc2, mode2, cls2, lv2 = F.parse(dif)
    assert np.array_equal(q2, qno) and np.array_equal(dc2, dc) and np.array_equal(mode2, mode) and np.array_equal(cls2, cls)
    assert np.array_equal(lv2, levels)
    D.lib().dvo_segment_coefs.argtypes = [D.u8p, C.c_int, C.c_int, C.POINTER(C.c_int16)]
    co = np.zeros((30, 64), np.int16)
    for s in range(0, F.SEGMENTS, 7):
        D.lib().dvo_segment_coefs(D.p8(dif), s // 27, s % 27, co.ctypes.data_as(C.POINTER(C.c_int16)))
        for i in range(30):
            sc = np.zeros(64, np.uint8)
            D.lib().dvo_scan(int(mode[30 * s + i]), D.p8(sc))
            have, lv = co[i][sc][1:] != 0, levels[30 * s + i][1:]
            assert not (have & (lv == 0)).any() and have[np.abs(lv) >= 4].all(), (s, i)
            assert co[i][0] == 4 * dc[30 * s + i] + 1024


def test_the_frame_writer_refuses_what_does_not_fit():
    _, (qno, dc, mode, cls, levels) = F.symbol_frame(F.SEEDS["symbol_frames"][0])
    big = levels.copy()
    big[30 * 5:30 * 6, 1:] = 200  # 30 blocks x 63 escapes of 16 bits
    with pytest.raises(F.DoesNotFit, match="segment 5 "):
        F.write_frame(qno, dc, mode, cls, big)
    bad = levels.copy()
    bad[0, 3] = 256
    with pytest.raises(ValueError):
        F.write_frame(qno, dc, mode, cls, bad)
    exact = np.zeros_like(levels)  # 2,680 bits exactly in every segment: 30 end-of-block words and 160 escapes
    for s in range(F.SEGMENTS):
        for n in range(160):
            exact[30 * s + n % 30, 1 + n // 30] = 100
    assert F.block_bits(exact[0]) * 10 + F.block_bits(exact[10]) * 20 == F.SEGMENT_AC_BITS
    dif = F.write_frame(qno, dc, mode, cls, exact)
    assert np.array_equal(F.parse(dif)[4], exact)
    exact[29, 63] = 1
    with pytest.raises(F.DoesNotFit, match="segment 0 "):
        F.write_frame(qno, dc, mode, cls, exact)


# ---- blocks ----
def _blame(inputs, i):
    dc, mode, cls, qno, levels = inputs
    k = np.flatnonzero(levels[i])
    return f"mode {mode[i]}, scan position(s) {k.tolist()}, class {cls[i]}, qno {qno[i]}, level(s) {levels[i][k].tolist()}, dc {dc[i]}"


def test_every_scan_positions_gain():
    """both modes x scan positions 1..63 x classes x quantisation numbers, one level each that makes the float pattern
    large but inside 0..255: pixels within the bound, least-squares gain of the oracle on the float pattern within the
    relative bound of 1.  A wrong weight is several per cent at one position; the message names it."""
    inputs = F.position_sweep()
    assert len(inputs[0]) == 2 * 63 * 4 * 16
    px, ok = F.blocks(*inputs)
    assert ok.all() and px.min() >= 128 - F.TARGET - 1e-9 and px.max() <= 128 + F.TARGET + 1e-9
    assert (np.abs(px - 128).max(axis=1) > 16).all()  # large: even the coarsest step's single level
    m = F.measure_blocks(inputs)
    print(m)
    b = B["bounds"]["blocks"]["position"]
    assert m["gain"] <= b["gain"], f"gain off by {m['gain']:.4f} at {_blame(inputs, m['gain_at'])}"
    assert m["abs"] <= b["abs"], f"{m['abs']:.3f} levels at {_blame(inputs, m['abs_at'])}"
    assert abs(m["mean"]) <= b["mean"]


def test_dc_in_both_modes():
    inputs = F.dc_sweep()
    got = F.oracle_blocks(*inputs).astype(np.float64)
    want = np.clip(128 + inputs[0] / 2.0, 0, 255)
    assert np.abs(got - want[:, None]).max() <= B["bounds"]["blocks"]["dc"]["abs"] == 0.5
    px, ok = F.blocks(*inputs)
    assert ok.all() and np.abs(px - (128 + inputs[0] / 2.0)[:, None]).max() < 1e-9  # the float statement's own DC


def test_random_symbol_blocks():
    inputs = F.random_blocks()
    nz = (inputs[4] != 0).sum(axis=1)
    assert nz.min() >= 1 and nz.max() <= 20
    m = F.measure_blocks(inputs)
    print(m)
    assert m["out_of_range"] == 0
    b = B["bounds"]["blocks"]["random"]
    assert m["abs"] <= b["abs"], f"{m['abs']:.3f} levels at {_blame(inputs, m['abs_at'])}"
    assert abs(m["mean"]) <= b["mean"], m["mean"]  # a bias shows here


# ---- whole frames, three encoders apart, both systems ----
@pytest.mark.parametrize("system", [525, 625])
@pytest.mark.parametrize("family", ["a", "b", "c"])
def test_whole_frames(system, family):
    """dvo_decode_frame against dvf_decode_frame on every block (the float decoder flags none as outside the
    fixed-point range: asserted).  a: the oracle's encoder; b: the plain encoder; c: symbol-written, class x qno x mode
    swept over the picture with overflow into passes 2 and 3."""
    b = B["bounds"]["frames"][str(system)][family]
    fin_all = np.zeros(4, np.int64)
    for i, frame in enumerate(F.frames(system, family)):
        pic, out, fin = F.float_decode_info(system, frame)
        assert out == 0, f"frame {i}: {out} blocks outside the fixed-point range"
        d = F.deviation(F.oracle_decode(system, frame), pic)
        print(system, family, i, float(np.abs(d).max()), float(d.mean()), fin)
        assert np.abs(d).max() <= b["abs"], (i, float(np.abs(d).max()), int(np.abs(d).argmax()))
        assert abs(d.mean()) <= b["mean"], (i, float(d.mean()))
        fin_all += fin
    assert fin_all[1] > 1000 and fin_all[2] > 100  # blocks that ended in pass 2 and in pass 3
    if family == "c":
        assert fin_all[2] > 2000
        _, (qno, dc, mode, cls, levels) = F.symbol_frame(F.SEEDS["symbol_frames"][0])
        combos = set(zip(np.repeat(qno, 6).tolist(), cls.tolist(), mode.tolist()))
        assert len(combos) == 16 * 4 * 2  # every class x qno x mode


@pytest.mark.parametrize("system", [525, 625])
def test_plain_encoder_round_trip_is_as_good_as_the_oracles_pair(system):
    """the first round trip whose halves are not inverses by construction: plain encoder -> float decoder, PSNR against
    the source, relative to oracle encoder -> oracle decoder on the same picture with the plain encoder's rate control
    starting at the oracle's quantisation numbers.  Both quantise the same coefficients with the same steps 2^s / W, so
    the same noise power is expected; 1 dB (a quarter more noise power) is allowed for their different mode and class
    choices and rate-control fallbacks.  A scale or weight the encoder and the float decoder disagree on costs far more."""
    pics = F.PICTURES_525 if system == 525 else F.PICTURES_625
    for (amp, flags), fa in zip(pics, F.frames(system, "a")):
        src = F.picture(system, amp)
        if system == 525:
            qa = F.segment_qnos(fa)
            fb = F.encode(src, flags, qno_start=qa)
            assert (F.segment_qnos(fb) <= qa).all()
            pic, out, _ = F.decode_info(fb)
        else:
            fb = F.encode625(src, flags)
            pic, out, _ = F.decode625_info(fb)
        assert out == 0
        mine = F.psnr(np.clip(np.rint(pic), 0, 255), src)
        pair = F.psnr(F.oracle_decode(system, fa), src)
        cross = F.psnr(F.oracle_decode(system, fb), src)  # and the oracle's decoder on the plain encoder's stream
        print(system, amp, flags, mine, pair, cross)
        assert mine >= pair - 1.0, (amp, flags, mine, pair)
        assert cross >= pair - 1.0, (amp, flags, cross, pair)


# ---- the bounds have teeth ----
# which input family has to notice which wrong model: single coefficients see every AC error, the DC sweep the DC scale
# and the exchanged fields, random blocks and the frames of the plain encoder and of the symbol writer everything; the
# oracle's own encoder gives no block of these pictures class 3, so its frames cannot see perturbation 4
MUST_NOTICE = {1: ("position", "random", "a", "b", "c"), 2: ("position", "random", "a", "b", "c"),
               3: ("position", "random", "a", "b", "c"), 4: ("position", "random", "b", "c"),
               5: ("dc", "random", "a", "b", "c"), 6: ("position", "dc", "random", "a", "b", "c")}
BLAME = {1: lambda m, k, c, q: 4 in divmod(int(_scan(m)[k]), 8) or (m == 1 and divmod(int(_scan(m)[k]), 8)[0] >> 1 == 2),
         3: lambda m, k, c, q: k == 6, 4: lambda m, k, c, q: c == 3, 6: lambda m, k, c, q: m == 1}


def _scan(mode):
    sc = np.zeros(64, np.uint8)
    F.lib().dvf_scan(mode, D.p8(sc))
    return sc


@pytest.mark.parametrize("which", sorted(F.PERTURBATIONS))
def test_a_wrong_float_model_exceeds_the_bound(which):
    """the perturbation is applied to the float model, never to the code under test; same inputs, same bounds"""
    block_inputs = {"position": F.position_sweep(), "dc": F.dc_sweep(), "random": F.random_blocks()}
    with F.perturbed(which):
        for fam in MUST_NOTICE[which]:
            if fam in block_inputs:
                m = F.measure_blocks(block_inputs[fam])
                print(which, fam, m)
                assert m["abs"] > B["bounds"]["blocks"][fam]["abs"], (which, fam, m)
                if fam == "position":
                    assert m["gain"] > B["bounds"]["blocks"]["position"]["gain"]
                    mode, k, cls, qno = (int(a[m["gain_at"]]) for a in F.sweep_index())
                    if which in BLAME:  # the position it blames is one the perturbation touches
                        assert BLAME[which](mode, k, cls, qno), (mode, k, cls, qno)
            else:
                worst = max(float(np.abs(F.deviation(F.oracle_decode(525, f), F.decode(f))).max()) for f in F.frames(525, fam))
                print(which, fam, worst)
                assert worst > B["bounds"]["frames"]["525"][fam]["abs"], (which, fam, worst)
    assert F.measure_blocks(block_inputs["dc"])["abs"] < 0.5 + 1e-9  # and the model is itself again


def test_the_bounds_file_records_these_inputs():
    assert B["seeds"] == F.SEEDS and B["target"] == F.TARGET
    assert [tuple(p) for p in B["pictures_525"]] == F.PICTURES_525 and [tuple(p) for p in B["pictures_625"]] == F.PICTURES_625
    for k, m in B["measured"]["blocks"].items():
        assert m["abs"] <= B["bounds"]["blocks"][k]["abs"] < m["abs"] + B["step"]["abs"] + 1e-9
    for s in ("525", "625"):
        for fam, m in B["measured"]["frames"][s].items():
            assert m["abs"] <= B["bounds"]["frames"][s][fam]["abs"] < m["abs"] + B["step"]["abs"] + 1e-9
