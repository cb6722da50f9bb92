"""The content of the 4:2:0 inter encoder tests, checked with the oracle alone: its packets of the chosen streams obey
the rule tests/test_gpu_rtj420_encode.py then holds the device to (coded and unchanged blocks in one packet, repeated
pictures all 0xFF, nothing coded at quality 1 with masks of 2)."""
import pytest

import rtj420_enc as T


@pytest.mark.parametrize("w,h", T.INTER_SHAPES)
def test_the_oracles_packets_of_the_inter_streams_obey_the_skip_rule(w, h):
    for key, Q in T.INTER_SETTINGS:
        for lmask, cmask in T.MASKS:
            pkts = T.oracle_packets(w, h, Q, T.inter_pictures(w, h, seed=key + lmask), key, lmask, cmask)
            T.assert_skip_rule((w, h, key, Q, lmask, cmask), pkts, key, Q, lmask, cmask)
