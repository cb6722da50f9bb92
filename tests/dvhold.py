"""Test statement of held macroblocks (include/mi_dv.h: mi_dv_decode_batch_held, mi_dv_decode_frame_held) on top of
tests/dvsys.py and dvlib.  TEST INFRASTRUCTURE ONLY: the product never imports it.  UNPINNED like everything about DV
here: which STA values mean "error" is this repository's reading of IEC 61834-2 from memory (the default mask below).

Byte 3 of a DIF block is STA | QNO.  A macroblock is flagged when bit STA (the high nibble) is set in a 16-bit mask.
Macroblock mb = 5 (27 seq + slot) + m of a frame (seq counts the frame's sequences in byte order) covers the picture bytes
Layout.block gives for its place (Layout.place) over the areas the system shows (Layout.shown): written here from the
layouts alone, independently of csrc/dv_common.h.  hold() decodes every frame with dvsys.decode, which ignores STA as the
oracle does, and then, in stream order, overwrites flagged macroblocks from the running picture."""
import functools
import hashlib

import numpy as np

import dvlib as D
import dvsys as S

STA_ERRORS = 0x8080  # STA 0111 and 1111: "error exists"
ERROR_NIBBLES = (0x7, 0xF)
OTHER_NIBBLES = tuple(v for v in range(16) if v not in ERROR_NIBBLES)


def macroblocks(system):
    """(seq, slot, m) in macroblock order"""
    g = S.geometry(system)
    return [(seq, slot, m) for seq in range(g.frame_seqs) for slot in range(27) for m in range(5)]


@functools.lru_cache(None)
def offsets(system):
    """[macroblock, pixel]: the picture byte offsets of every macroblock (384 each; 256 in 4:2:2)"""
    g = S.geometry(system)
    a = np.stack([np.concatenate([g.block(g, *g.place(g, seq, slot, m), j) for j in g.shown])
                  for seq, slot, m in macroblocks(system)])
    a.setflags(write=False)
    return a


@functools.lru_cache(None)
def sta_offsets(system):
    """the frame byte that holds STA | QNO, per macroblock"""
    a = np.array([D.video_block_offset(seq, 5 * slot + m) + 3 for seq, slot, m in macroblocks(system)])
    a.setflags(write=False)
    return a


@functools.lru_cache(None)
def column22(system):
    """per macroblock: it lies in 4:1:1's right-edge column (16 x 16, split chroma halves); nowhere in the other systems"""
    g = S.geometry(system)
    a = np.array([g.k411 and g.place(g, seq, slot, m)[0] == 22 for seq, slot, m in macroblocks(system)])
    a.setflags(write=False)
    return a


def flags(system, frame, mask=STA_ERRORS):
    """per macroblock: its STA nibble is a set bit of the mask"""
    sta = np.asarray(frame, np.uint8)[sta_offsets(system)] >> 4
    return ((mask >> sta.astype(np.uint32)) & 1).astype(bool)


def stamp(system, frame, nibbles):
    """a copy of the frame with these STA nibbles (one per macroblock); QNO stays"""
    f = np.array(frame, np.uint8)
    at = sta_offsets(system)
    f[at] = (f[at] & 0x0F) | (np.asarray(nibbles, np.uint8) << 4)
    return f


def nibbles(system, rng, flagged):
    """STA nibbles: an error value where `flagged` (per macroblock), any of the 14 others elsewhere"""
    flagged = np.asarray(flagged, bool)
    return np.where(flagged, rng.choice(ERROR_NIBBLES, flagged.size), rng.choice(OTHER_NIBBLES, flagged.size)).astype(np.uint8)


_DECODED = {}


def decoded(system, frame):
    """dvsys.decode of the frame, made once for all frames that differ in their STA nibbles only (the decode ignores them:
    tests/test_gpu_dv.py holds the kernel and the oracle to that)"""
    plain = stamp(system, frame, np.zeros(sta_offsets(system).size, np.uint8))
    key = (system, hashlib.sha1(plain.tobytes()).digest())
    if key not in _DECODED:
        pic = S.decode(system, plain)
        pic.setflags(write=False)
        _DECODED[key] = pic
    return _DECODED[key]


def hold_stream(system, frames, mask=STA_ERRORS):
    """the one-frame path: every frame is a run of one picture whose prev is the picture made of the frame before — the
    whole picture, also where that frame's macroblock was flagged itself and kept its decode; the first frame has no
    prev -> (pictures, per picture the macroblocks taken)"""
    out, taken, prev = [], [], None
    for f in np.asarray(frames, np.uint8).reshape(-1, S.geometry(system).frame_bytes):
        pic, t = hold(system, f, [1], prev, mask)
        prev = pic
        out.append(pic[0])
        taken.append(int(t[0]))
    return np.stack(out), np.array(taken)


def hold(system, frames, runs=None, prev=None, mask=STA_ERRORS):
    """frames (n x frame bytes) in runs of consecutive frames of one stream each (None: one run), prev: one picture per
    run or None -> (pictures n x picture bytes, per picture the macroblocks taken from the running picture).  A flagged
    macroblock the running picture has no source for (flagged in every picture of the run so far, and no prev) keeps the
    decode."""
    g = S.geometry(system)
    frames = np.asarray(frames, np.uint8).reshape(-1, g.frame_bytes)
    runs = list(runs) if runs else [frames.shape[0]]
    assert sum(runs) == frames.shape[0] and min(runs) > 0
    off = offsets(system)
    out = np.empty((frames.shape[0], g.picture_bytes), np.uint8)
    taken = np.zeros(frames.shape[0], np.int64)
    k = 0
    for r, length in enumerate(runs):
        running = None if prev is None else np.asarray(prev, np.uint8).reshape(len(runs), g.picture_bytes)[r]
        have = np.full(off.shape[0], prev is not None)  # per macroblock: the running picture holds a source
        for _ in range(length):
            pic = decoded(system, frames[k]).copy()
            fl = flags(system, frames[k], mask)
            take = fl & have
            if take.any():
                at = off[take].ravel()
                pic[at] = running[at]
            taken[k] = take.sum()
            have |= ~fl
            running = out[k] = pic
            k += 1
    return out, taken
