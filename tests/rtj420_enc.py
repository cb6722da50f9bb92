"""What the 4:2:0 encoder tests share: the inter streams, the settings they are coded with, and the rule their packets
obey (tests/test_rtj420_encode_cpu.py holds the oracle's packets to it, tests/test_gpu_rtj420_encode.py the device's).

Only tests/ imports this."""
import numpy as np

import rtjfmt as F
import rtjfmt_enc as E
import rtjlib as R

INTER_SHAPES = [(48, 32), (176, 48), (528, 16)]
INTER_SETTINGS = ((1, 255), (3, 128), (255, 224), (3, 1))  # (key_rate, Q)
MASKS = ((0, 0), (2, 2), (16, 16), (2, 5))


def inter_pictures(w, h, seed):
    """six pictures of one stream (rtjfmt_enc.make_stream: a new top third each time, inverted in every odd one), each
    followed by itself: twelve"""
    return [p for q in E.make_stream(F.FMT_420, w, h, 6, seed=seed, amp=8) for p in (q, q.copy())]


def oracle_packets(w, h, Q, pics, key=0, lmask=0, cmask=0):
    enc = R.OracleEncoder(w, h, Q, key, lmask, cmask)
    return [enc.encode(p) for p in pics]


def block_kinds(pkt):
    """(unchanged blocks, coded blocks): an unchanged block is the byte 0xFF, a coded block has at least two bytes and
    never starts with 0xFF (its first byte is clamped to 254)"""
    offs = R.OracleDecoder().block_offsets(pkt).astype(np.int64)  # from the packet's first byte
    assert offs[0] == 12 and offs[-1] == pkt.size
    first, length = pkt[offs[:-1]], np.diff(offs)
    unchanged = first == 0xFF
    assert np.all(length[unchanged] == 1) and np.all(length[~unchanged] >= 2)
    return int(np.count_nonzero(unchanged)), int(np.count_nonzero(~unchanged))


def assert_skip_rule(what, pkts, key, Q, lmask, cmask):
    """the packets of inter_pictures(): the key byte counts and wraps; a repeated picture is nothing but 0xFF; a key frame
    has coded blocks (and without masks no other); every other packet after the first has both kinds (the new top third, the rest unchanged).
    Quality 1 with masks of 2 or more codes no block at all (rtjfmt_enc.all_blocks_forced_unchanged)."""
    assert [int(p[11]) for p in pkts] == [i % (key + 1) for i in range(len(pkts))], what
    kinds = [block_kinds(p) for p in pkts]
    nb = sum(kinds[0])
    for i, (p, (unchanged, coded)) in enumerate(zip(pkts, kinds)):
        if E.all_blocks_forced_unchanged(Q, lmask, cmask):
            assert coded == 0, (what, i, kinds)
        elif i & 1:  # the picture before it again, and at these key rates never a key frame
            assert p[11] != 0 and p.size == 12 + nb and np.all(p[12:] == 0xFF), (what, i, kinds)
        elif p[11] == 0:
            # the store was cleared, so a block is unchanged only where all it quantises to lies within the mask of zero:
            # with no mask and a quantiser finer than quality 1's, no block of these pictures (their DC is not zero)
            assert coded > 0 and (unchanged == 0 or Q == 1 or max(lmask, cmask) > 0), (what, i, kinds)
        else:
            assert unchanged > 0 and coded > 0, (what, i, kinds)
