"""The statement of the uncompressed YUV family (tests/yuvraw.py, what libmi_yuv.so is held to) against the reference's own
lib/video_yuv.c, compiled as it stands into oracle/_ref/libvideo_yuv_ref.so (tests/yuvref.py; skipped only where that
library is absent): every codec at every shape of the GPU suite and at its smallest accepted size, three seeded packets
each, plane by plane and row by row within the row widths of yuvraw.layout.  Byte equality.

Only sizes libmi_yuv accepts are compared.  At the others the reference is not wrong so much as careless, which is noted
here and tested nowhere: an odd width loses its last pixel in the 4:2:2 and 4:2:0 codecs (w/2 pairs a row), an odd height
its last row in yv12, YV12 and yuv4, YVU9 takes (h/4) chroma rows, and a v210 row of a width that is no multiple of 6
reads a whole last group of 16 bytes, which lies within the row only because its stride is padded to 48 pixels."""
import numpy as np
import pytest

import yuvraw as Y
import yuvref as R

pytestmark = pytest.mark.skipif(not R.have_reference(), reason="oracle/_ref/libvideo_yuv_ref.so is not built (no reference tree)")
SHAPES = R.CASES + [(c, *R.SMALLEST[c]) for c in Y.CODECS if R.SMALLEST[c] not in R.SHAPES[c]]
HANDED_ON = ("2vuy", "VYUY", "yv12", "YVU9")  # decoders that set s->vframe: their planes are the packet's own bytes


def test_the_eleven_decoders_are_the_statement_s_codecs():
    assert R.decoders() == list(Y.CODECS)
    assert all(c in R.SHAPES and R.SMALLEST[c] == min(R.SHAPES[c]) for c in Y.CODECS)  # the GPU suite's shapes begin at the smallest
    for c in Y.CODECS:  # and one step below the smallest the library refuses
        w, h = R.SMALLEST[c]
        for bad in ((w - 1, h), (w, h - 1)):
            with pytest.raises(ValueError):
                Y.layout(c, *bad)


@pytest.mark.parametrize("codec,w,h", SHAPES, ids=[f"{c}-{w}x{h}" for c, w, h in SHAPES])
def test_the_statement_equals_the_reference(codec, w, h):
    lay = Y.layout(codec, w, h)
    compared = 0
    for k, packet in enumerate(R.packets(codec, w, h)):
        assert packet.size == lay.packet_bytes
        want, strides = R.decode(codec, w, h, packet)
        got = Y.planes_of(codec, w, h, Y.unpack(codec, w, h, packet))
        assert len(got) == len(want) == len(lay.planes), (codec, "planes")
        for i, (pw, ph, bps) in enumerate(lay.planes):
            assert want[i].shape[0] >= ph and want[i].shape[1] >= pw * bps, (codec, "plane", i, want[i].shape)
            for r in range(ph):
                assert np.array_equal(got[i][r], want[i][r, :pw * bps]), f"{codec} {w} x {h}, packet {k}: plane {i} row {r}"
            assert want[i].shape == (ph, pw * bps)  # and the reference's plane is no larger than the statement's
        if codec in HANDED_ON:  # the strides it reads the packet at are the statement's
            assert tuple(strides) == tuple(s for s in lay.packet_strides if s), codec
        compared += 1
    assert compared == R.PACKETS == 3


def test_the_number_of_shapes():
    # the GPU suite's 43 shapes; every codec's smallest size is among its shapes already
    assert len(R.CASES) == 43 and len(SHAPES) == 43 and {c for c, _, _ in SHAPES} == set(Y.CODECS)


def test_a_packet_of_no_bytes_is_skipped():
    out = np.zeros(64, np.uint8)
    info = np.zeros(14, np.int32)
    import ctypes as C
    n = R.reference().mi_yuvref_decode(R.fourcc("v308"), 2, 2, None, 0, out.ctypes.data, out.size, info.ctypes.data_as(C.POINTER(C.c_int32)))
    assert n == 0 and not out.any()
