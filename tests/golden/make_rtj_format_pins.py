#!/usr/bin/env python3
"""Writes tests/golden/rtj_format_pins.json: what the library answers where only a picture format's geometry decides.

    bound     mi_rtj_encode_bound(w, h, n, align) and mi_rtj_encode_bound_fmt(fmt, w, h, n, align) over the grids below
              (pure host code: no device needed)
    refusals  over fmt x w x h with one picture: return code and, where it is not 0, the full mi_rtj_last_error text of
              mi_rtj_encode_frames_fmt, of mi_rtj_encode_stream_fmt, and of mi_rtj_set_format followed by the decode of
              a packet that is nothing but a header of that size (needs a device; a refused call launches nothing)

The file was first written from the library before its formats were described by one table (MI_RTJ_LIB pointed at that
build), so it pins the table to the per-call-site arithmetic and texts it replaced."""
import functools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from pkg import P  # noqa: E402

B = P.binding
PINS = os.path.join(HERE, "rtj_format_pins.json")
FMTS = (-1, 0, 1, 2, 3)
SIZES = (0, 8, 16, 24, 40, 48, 1920, 1088)
COUNTS = (0, 1, 257)
ALIGNS = (0, 1, 64)


def bounds():
    """{"fmt": [[fmt, w, h, n, align, bytes] ...], "plain": [[w, h, n, align, bytes] ...]}"""
    L = P.load()
    grid = [(w, h, n, a) for w in SIZES for h in SIZES for n in COUNTS for a in ALIGNS]
    return {"plain": [[w, h, n, a, L.mi_rtj_encode_bound(w, h, n, a)] for w, h, n, a in grid],
            "fmt": [[f, w, h, n, a, L.mi_rtj_encode_bound_fmt(f, w, h, n, a)] for f in FMTS for w, h, n, a in grid]}


@functools.lru_cache(None)
def refusals():
    """[[fmt, w, h, [rc, text] of encode_frames_fmt, of encode_stream_fmt, of set_format + decode] ...]"""
    out = []
    big = max(SIZES) * max(SIZES)
    enc = P.MiRtj()
    d_fr, d_st = enc.alloc(2 * big), enc.alloc(12 + 2 * big * 2 + 64)  # the largest picture and its worst-case packet
    enc.memset(d_fr, 100, 2 * big)
    po, pl = np.zeros(1, np.uint64), np.zeros(1, np.uint32)
    pop, plp = po.ctypes.data_as(B.u64p), pl.ctypes.data_as(B.u32p)

    def answer(dev, rc):
        return [rc, dev.L.mi_rtj_last_error(dev.h).decode() if rc != 0 else ""]

    for fmt in FMTS:
        dec = P.MiRtj()
        set_rc = dec.L.mi_rtj_set_format(dec.h, fmt)
        set_answer = answer(dec, set_rc)
        for w in SIZES:
            for h in SIZES:
                frames = answer(enc, enc.L.mi_rtj_encode_frames_fmt(enc.h, fmt, w, h, 128, 1, d_fr, d_st, 1, pop, plp))
                stream = answer(enc, enc.L.mi_rtj_encode_stream_fmt(enc.h, fmt, w, h, 128, 3, 2, 2, 1, d_fr, d_st, 1, pop, plp))
                if set_rc != 0:
                    decode = set_answer
                else:
                    hdr = np.array([12, 0, 0, 0, 12, 0, w & 255, w >> 8, h & 255, h >> 8, 128, 0], np.uint8)
                    decode = answer(dec, dec.L.mi_rtj_decode(dec.h, hdr.ctypes.data_as(B.u8p), hdr.size, None, None, 0, 0))
                out.append([fmt, w, h, frames, stream, decode])
        dec.close()
    enc.free(d_fr)
    enc.free(d_st)
    enc.close()
    return out


def text(pins):
    """one row per line"""
    rows = lambda key, v: '"%s": [\n%s\n]' % (key, ",\n".join(json.dumps(r) for r in v))
    return '{"bound": {\n%s,\n%s\n},\n%s\n}\n' % (rows("plain", pins["bound"]["plain"]), rows("fmt", pins["bound"]["fmt"]),
                                                  rows("refusals", pins["refusals"]))


def main():
    with open(sys.argv[1] if len(sys.argv) > 1 else PINS, "w") as f:
        f.write(text({"bound": bounds(), "refusals": refusals()}))


if __name__ == "__main__":
    main()
