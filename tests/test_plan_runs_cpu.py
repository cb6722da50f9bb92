"""Plans with runs, without a GPU: the entry point is exported, and the run rule the device implements
(include/mi_rtjpeg.h, mi_rtj_plan_set_runs) equals the reference's in-order decode, checked on the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import rtjlib as R
import runlib as RL
from pkg import P


def test_set_runs_and_its_queries_are_exported():
    L = C.CDLL(P.binding.lib_path())
    for name in ("mi_rtj_plan_set_runs", "mi_rtj_plan_run_times", "mi_rtj_plan_run_stats"):
        assert hasattr(L, name), name


def test_set_runs_refuses_a_missing_plan():
    L = P.binding.load()
    lens = (C.c_int * 1)(1)
    assert L.mi_rtj_plan_set_runs(None, 1, lens) == -3


def _prev(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, RL.frame_bytes(w, h), dtype=np.uint8)


@pytest.mark.parametrize("w,h,Q,key_rate,lm,cm", [(160, 128, 200, 4, 2, 2), (64, 48, 90, 1, 0, 0),
                                                  (96, 64, 255, 255, 16, 16), (48, 32, 30, 3, 6, 1)])
def test_rule_equals_in_order_decode_on_encoder_streams(w, h, Q, key_rate, lm, cm):
    pkts = RL.stream_packets(w, h, Q, 13, key_rate, lm, cm, seed=w + Q)
    assert sum(int((p[12:] == 255).sum()) for p in pkts) > 0
    for runs in ([13], [1, 12], [5, 1, 7], [1] * 13):
        prev = [_prev(w, h, r) for r in range(len(runs))]
        want = RL.oracle_in_order(pkts, runs, prev)
        got = RL.oracle_by_rule(pkts, runs, prev)
        for i, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a, b), (runs, i)


def test_rule_equals_in_order_decode_on_adversarial_packets():
    """0xFF at every position: block starts, raw bytes, run tokens, past the packet's end."""
    from golden.make_golden import adversarial_packet
    rng = np.random.default_rng(77)
    for Q in (1, 31, 129, 255):
        _, _, lb8, cb8, _, _ = R.oracle_tables(Q)
        for (w, h) in ((48, 32), (160, 16)):
            pkts = [adversarial_packet(rng, w, h, Q, lb8, cb8, skip_prob=float(rng.choice([0.1, 0.5, 0.9])))
                    for _ in range(5)]
            pkts += [RL.skip_heavy_packet(rng, w, h, Q) for _ in range(5)]
            pkts.append(RL.skip_heavy_packet(rng, w, h, Q, n=0))  # header only: every block reads zeros
            perm = rng.permutation(len(pkts))
            pkts = [pkts[i] for i in perm]
            runs = [len(pkts)]
            prev = [_prev(w, h, Q)]
            want = RL.oracle_in_order(pkts, runs, prev)
            got = RL.oracle_by_rule(pkts, runs, prev)
            for i, (a, b) in enumerate(zip(got, want)):
                assert np.array_equal(a, b), (Q, w, h, i)


def test_block_geometry_of_the_model():
    """A block's stream number maps to the 8x8 region the reference writes (lib/RTjpeg.c:2701-2745)."""
    w, h = 48, 32
    pic = np.zeros(RL.frame_bytes(w, h), np.uint8)
    y, u, v = RL._block_planes(pic, w, h)
    plane, by, bx = RL._block_coords(w, h)
    # macroblock 4 (second row, second column): Y3 is rows 24..31, columns 24..31; V is rows 8..15 of V, columns 8..15
    b = 4 * 6
    (y if plane[b + 3] == 0 else None)[by[b + 3], bx[b + 3]] = 1
    v[by[b + 5], bx[b + 5]] = 2
    Y = pic[:w * h].reshape(h, w)
    assert Y[24:32, 24:32].min() == 1 and Y.sum() == 64
    V = pic[w * h * 5 // 4:].reshape(h // 2, w // 2)
    assert V[8:16, 8:16].min() == 2 and V.sum() == 128
