"""Makes tests/golden/rtjfmt_golden.npz with the reference's own lib/RTjpeg.c (oracle/_ref/librtjpeg_ref.so, built by
oracle/Makefile where the reference tree is present): 4:2:2 and greyscale packets from RTjpeg_compress after
RTjpeg_set_format, and the planes RTjpeg_decompress makes of them.  Data only.

    python tests/golden/make_rtjfmt_golden.py

A case is one stream: its packets are decoded in order by one reference decoder whose planes start as 77, so the
unchanged (0xFF) blocks of inter streams (RTjpeg_set_intra 3, 2, 2) keep what the packet before left.
    cases          rows of (case, format, width, height, quality, key rate, packets)
    c<i>_pkt<n>    packet n of case i
    c<i>_out<n>    the contiguous planes after packet n"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import rtjfmt as F  # noqa: E402
import rtjlib as R  # noqa: E402

# (format, width, height, quality, noise amplitude, key rate, packets)
CASES = [
    (F.FMT_422, 48, 24, 255, 64, 0, 1),
    (F.FMT_422, 48, 24, 128, 8, 3, 3),
    (F.FMT_422, 48, 24, 1, 8, 0, 1),
    (F.FMT_422, 176, 40, 224, 8, 0, 1),
    (F.FMT_422, 176, 40, 192, 0, 3, 2),
    (F.FMT_GREY, 24, 8, 255, 64, 0, 1),
    (F.FMT_GREY, 24, 8, 1, 8, 0, 1),
    (F.FMT_GREY, 136, 72, 224, 8, 0, 1),
    (F.FMT_GREY, 136, 72, 128, 0, 3, 2),
]


def main():
    assert R.have_reference(), "oracle/_ref/librtjpeg_ref.so is missing: build the oracle where the reference tree is"
    out = {}
    rows = []
    for ci, (fmt, w, h, Q, amp, key, n) in enumerate(CASES):
        enc = F.RefFmt(fmt)
        enc.setup_encoder(w, h, Q, key, 2, 2)
        dec = F.RefFmt(fmt)
        planes = np.full(F.plane_bytes(fmt, w, h), 77, np.uint8)
        pics = F.make_stream(fmt, w, h, n, seed=10 + ci, amp=amp)  # (inter streams: some blocks change, the others stay)
        for i in range(n):
            pkt = enc.encode(pics[i])
            dec.decode(pkt, planes)
            out[f"c{ci}_pkt{i}"] = pkt
            out[f"c{ci}_out{i}"] = planes.copy()
        rows.append((ci, fmt, w, h, Q, key, n))
    out["cases"] = np.array(rows, np.int32)
    np.savez_compressed(F.GOLDEN_NPZ, **out)
    print(F.GOLDEN_NPZ, os.path.getsize(F.GOLDEN_NPZ), "bytes")


if __name__ == "__main__":
    main()
