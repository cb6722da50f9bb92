"""Edge segments for the DV encoder: named video segments built to reach the branches of the statement tests/dvenc.py (and
so of k_dv_encode) that natural-looking pictures do not, and the pictures of any system made of them.  TEST
INFRASTRUCTURE ONLY.  PARITY UNPINNED like everything DV here.

A segment is [30][64] pixels, macroblock-major, Y0 Y1 Y2 Y3 Cr Cb: what dvenc.encode_blocks takes.  segments() is the list;
picture(system) scatters it cyclically over the system's video segments (segment S of the frame is entry S mod L), through
dvenc.block_map() for 525/60 and through dvsys.maps(system) from 525/60 carrier pictures for the other four, so column 22
of the 4:1:1 systems and its split chroma halves take part.  L is odd: a wave of the kernel encodes segments 2p and 2p + 1,
and with every repetition of the list the partners change, so each entry meets its successor and its predecessor.

The 4:2:2 systems code areas 1 and 3 of a macroblock as flat 128.  Every entry but `ties` and `drops` is flat 128 there
anyway and carries its case in SLOTS (areas 0, 2, 4 and 5), so it is the same segment in all five systems.

The entries:
  clip        a vertical half-and-half of 0 / 255, its transpose and a checkerboard among flat blocks.  The segment stays at
              quantisation number 15; in class 0 (flags 0 and 1) levels pass 255 and are clipped, and the 1111111 aaaaaaaa
              word is written with amplitude 255.  With flags bit 1 the blocks take class 3 and nothing is clipped.
  ext0..15    the 0 / 255 sign pattern of every AC basis function of both transforms (2 x 63 blocks, eight a segment):
              the input that drives one coefficient as far as pixels can.  The pattern is made for a mode; which mode the
              block then takes is the statement's rule's business (census: `modes`).  Then an all-0 and an all-255 block:
              c00 = 512 (p - 128), so their DC (c00 + 128) >> 8 is -256 and 254.  127 is the most a pixel has above the
              offset, so DC 255 cannot occur and the upper DC clip is dead code by arithmetic.
  run16, run32  128 + A basis(7, 7), A = 16 and 32, alone among flat blocks.  In 8-8 the only level is scan position 63: a
              bare run of 62 (1111110 111101) and then the amplitude.  With flags bit 0 the block goes 2-4-8 and its levels
              land late in that scan, behind a long run.
  mode        two flat blocks with one column set: d1 = 2 d2 + 64 (stays 8-8) and d1 = 2 d2 + 65 (goes 2-4-8).
  class       six blocks of one horizontal basis pattern with big = max P >> 20 of 11, 12, 35, 36, 143 and 144: both sides of
              every class limit.  Horizontal only, so d1 = 0 and the mode is 8-8 under every flag.
  q15..q0     one segment per quantisation number, chosen at flags 3 with nothing dropped: loud blocks among quiet ones.
  fit-*, next-*   per flags, a segment whose chosen number q > 0 needs exactly 2,680 bits, and one that needs exactly 2,681
              at q + 1.
  flat-a, ties, flat-b   ties is 30 copies of one random tile: every block has the same bit count and the overflow rule
              takes levels in round-robin order, each step a tie.  Its neighbours are flat (number 15): the wave partners
              are 15 numbers apart, in each order.
  drops       30 different 0 / 255 binary-noise blocks: the longest overflow loop the statement is known to need.

What is searched (class amplitudes, the seeds of q*, fit-* and next-*) is searched by tests/golden/make_dv_encode_edges.py
and recorded in tests/golden/dv_encode_edges.json; this module only rebuilds from the record."""
import contextlib
import functools
import json
import os

import numpy as np

import dvenc as E
import dvlib as D
import dvsys as S

FIXTURE = os.path.join(D.ROOT, "tests", "golden", "dv_encode_edges.json")
SLOTS = np.array([6 * m + j for m in range(5) for j in (0, 2, 4, 5)])  # the 20 blocks of a segment that every system shows
EXT_SLOTS = SLOTS[[0, 5, 10, 15, 2, 7, 12, 17]]                        # eight of them: every area, every macroblock
GRADIENT = (3 * np.arange(8)[:, None] + 2 * np.arange(8)[None, :] + 100).ravel()
CLASS_TARGETS = (11, 12, 35, 36, 143, 144)
TIES_SEED, DROPS_SEED = 11, 12
MODE_COLUMNS = ((0, 22, 0, 22, 0, 22, 24, 22), (0, 23, 0, 23, 0, 23, 27, 23))  # d1 = 112 = 2 24 + 64; d1 = 119 = 2 27 + 65


# ---- builders: [30][64] int64 ----
def flat():
    return np.full((30, 64), 128, np.int64)


def _cos(n, k):
    return np.cos((2 * np.arange(n) + 1) * k * np.pi / (2 * n))


def basis(mode, r, h):
    """the 8 x 8 picture whose only coefficient is natural position (r, h) of the mode's transform (dvenc.transform: in
    2-4-8 rows 2v / 2v + 1 are frequency v of the line pairs' sums / differences)"""
    if mode == 0:
        return np.outer(_cos(8, r), _cos(8, h))
    v, diff = divmod(r, 2)
    lines = np.repeat(_cos(4, v), 2) * (np.tile([1.0, -1.0], 4) if diff else 1.0)
    return np.outer(lines, _cos(8, h))


def extremal_blocks():
    """[128][64]: for each mode and AC position the 0 / 255 sign pattern of its basis function, then all 0 and all 255"""
    out = [np.where(basis(mode, i // 8, i % 8) >= 0, 255, 0).ravel() for mode in (0, 1) for i in range(1, 64)]
    return np.array(out + [np.zeros(64, np.int64), np.full(64, 255)], np.int64)


def with_blocks(blocks, slots):
    px = flat()
    px[np.asarray(slots)] = blocks
    return px


def clip_segment():
    half = np.zeros((8, 8), np.int64)
    half[:, 4:] = 255
    checker = np.indices((8, 8)).sum(0) % 2 * 255
    return with_blocks([half.ravel(), half.T.ravel(), checker.ravel()], SLOTS[[0, 5, 10]])


def run_segment(amp):
    return with_blocks([np.rint(128 + amp * basis(0, 7, 7)).astype(np.int64).ravel()], SLOTS[[0]])


def mode_segment():
    blocks = np.full((2, 8, 8), 128, np.int64)
    for b, col in zip(blocks, MODE_COLUMNS):
        b[:, 3] = 100 + np.array(col)
    return with_blocks(blocks.reshape(2, 64), SLOTS[[0, 5]])


def class_block(h, quarters):
    """128 + quarters / 4 times the horizontal basis function h, rounded"""
    return np.rint(128 + quarters / 4.0 * basis(0, 0, h)).astype(np.int64).ravel()


def class_segment(found):
    """found: {target big: (h, quarters)}"""
    return with_blocks([class_block(*found[str(t)]) for t in CLASS_TARGETS], SLOTS[[0, 5, 10, 15, 2, 7]])


def noisy_segment(seed, amp, k):
    """the gradient in SLOTS, k of them with uniform noise of +-amp on it"""
    rng = np.random.default_rng(seed)
    px = with_blocks(GRADIENT, SLOTS)
    idx = SLOTS[rng.permutation(20)[:k]]
    px[idx] = np.clip(GRADIENT + rng.integers(-amp, amp + 1, (k, 64)), 0, 255)
    return px


def binary_segment(seed, lo, k):
    """k of SLOTS with random lo / 255 - lo pixels, on flat 128"""
    rng = np.random.default_rng(seed)
    idx = SLOTS[rng.permutation(20)[:k]]
    return with_blocks(np.where(rng.integers(0, 2, (k, 64)) == 1, 255 - lo, lo), idx)


def searched_segment(p):
    """a recorded parameter list: ['noise', seed, amp, k] or ['binary', seed, lo, k]"""
    return {"noise": noisy_segment, "binary": binary_segment}[p[0]](*p[1:])


def ties_segment():
    return np.tile(np.random.default_rng(TIES_SEED).integers(0, 256, 64), (30, 1)).astype(np.int64)


def drops_segment():
    return np.where(np.random.default_rng(DROPS_SEED).integers(0, 2, (30, 64)) == 1, 255, 0).astype(np.int64)


# ---- the list ----
@functools.lru_cache(None)
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def build(params):
    """(names, [L][30][64]) from the searched parameters; L is odd"""
    ext = extremal_blocks()
    out = [("clip", clip_segment())]
    out += [(f"ext{i}", with_blocks(ext[8 * i:8 * i + 8], EXT_SLOTS)) for i in range(16)]
    out += [("run16", run_segment(16)), ("run32", run_segment(32)), ("mode", mode_segment()), ("class", class_segment(params["class"]))]
    out += [(f"q{q}", searched_segment(params["qno"][str(q)])) for q in range(15, -1, -1)]
    seen = []
    for kind in ("fit", "next"):
        for flags in range(4):
            p = params["exact"][f"{kind}/{flags}"]
            if p not in seen:  # one segment may serve several flags
                seen.append(p)
                out.append((f"{kind}-{flags}", searched_segment(p)))
    out += [("flat-a", flat()), ("ties", ties_segment()), ("flat-b", flat()), ("drops", drops_segment())]
    if len(out) % 2 == 0:
        out.append(("flat-c", flat()))
    names = tuple(n for n, _ in out)
    assert len(set(names)) == len(names) and len(names) % 2 == 1 and 2 * len(names) <= E.SEGMENTS
    segs = np.array([s for _, s in out], np.int64)
    assert segs.min() >= 0 and segs.max() <= 255
    return names, segs


@functools.lru_cache(None)
def segments():
    names, segs = build(fixture()["params"])
    segs.setflags(write=False)
    return names, segs


def entry_of(system, reverse=False):
    """which entry of the list each video segment of a system's frame holds"""
    L = len(segments()[0])
    at = np.arange(S.geometry(system).segments) % L
    return L - 1 - at if reverse else at


def name_at(system, seg, reverse=False):
    return segments()[0][entry_of(system, reverse)[seg]]


def where(system, name, reverse=False):
    """the video segments of a system's frame that hold the named entry"""
    return np.flatnonzero(entry_of(system, reverse) == segments()[0].index(name))


def _carriers(system, pic):
    """the 525/60 pictures the statement encodes for a system's picture (dvsys.encode)"""
    if system == S.SYS_525_60:
        return pic.reshape(1, D.PICTURE_BYTES)
    g = S.geometry(system)
    src, dst, _, _ = S.maps(system)
    pics = np.full(g.hosts * D.PICTURE_BYTES, 128, np.uint8)
    pics[src] = pic[dst]
    return pics.reshape(g.hosts, D.PICTURE_BYTES)


def blocks_of(system, pic):
    """[30 segments][64]: the pixels of every block of a system's picture as the statement encodes them, in frame order"""
    return np.concatenate([c[E.block_map()] for c in _carriers(system, pic)])[:30 * S.geometry(system).segments].astype(np.int64)


@functools.lru_cache(None)
def picture(system, reverse=False):
    """THE EDGE PICTURE of a system (reverse: with the list back to front, so that every wave has the other partner order)"""
    g = S.geometry(system)
    px = segments()[1][entry_of(system, reverse)].reshape(-1, 64)
    carriers = np.full((g.hosts, D.PICTURE_BYTES), 128, np.uint8)
    for i in range(g.hosts):
        part = px[8100 * i:8100 * (i + 1)]
        carriers[i][E.block_map()[:part.shape[0]]] = part
    if system == S.SYS_525_60:
        pic = carriers[0]
    else:
        src, dst, _, _ = S.maps(system)
        pic = np.empty(g.picture_bytes, np.uint8)
        pic[dst] = carriers.reshape(-1)[src]
    pic.setflags(write=False)
    return pic


# ---- the census ----
@contextlib.contextmanager
def recording_mul():
    """dvenc._mul records the largest |x| it is given into the list this yields (the constants are 13 bits)"""
    seen, plain = [0], E._mul

    def mul(x, c):
        seen[0] = max(seen[0], int(np.abs(x).max()))
        return plain(x, c)
    E._mul = mul
    try:
        yield seen
    finally:
        E._mul = plain


def census(px, rec, flags):
    """what the statement did on blocks px [30 s][64], from its record: a dict of plain integers and lists (the fixture's
    census), and the arrays the conditions are asserted on"""
    mode, cls, levels = rec["mode"], rec["cls"], rec["levels"].astype(np.int64)
    qno, dropped = rec["qno"], rec["dropped"]
    with recording_mul() as operand:
        c = E.transform(px, mode)
    P, neg = E.products(c, mode)
    n = E.FRAC + E.shift_of(np.repeat(qno, 30), cls)
    raw = (P + (1 << (n - 1))) >> n
    raw[:, 0] = 0
    wl, run = E.word_lengths(levels)
    nz = levels != 0
    bits = E.block_bits(levels).reshape(-1, 30)
    total = bits.sum(axis=1)
    nxt = E.block_bits(E.quantise(P, neg, cls, np.repeat(np.minimum(qno + 1, 15), 30))).reshape(-1, 30).sum(axis=1)
    big = P[:, 1:].max(axis=1) >> E.FRAC
    p = px.reshape(-1, 8, 8)
    d1 = np.abs(p[:, 0:6] - p[:, 1:7]).sum(axis=(1, 2))
    d2 = np.abs(p[:, 0:6] - p[:, 2:8]).sum(axis=(1, 2))
    q2, dr2 = qno.reshape(-1, 2), dropped.reshape(-1, 2)
    arrays = {"big": big, "d1": d1, "d2": d2, "total": total, "next": nxt, "raw": raw, "run": np.where(nz, run, -1), "P": P}
    out = {
        "clipped": int((raw > 255).sum()),
        "largest_amplitude": int(np.abs(levels).max()),
        "longest_run": int(run[nz].max()),
        "runs_of_62": int((run[nz] == 62).sum()),
        "longest_word": int(wl.max()),
        "qno": np.bincount(qno, minlength=16).tolist(),
        "dropped": int(dropped.sum()),
        "most_dropped_in_a_segment": int(dropped.max()),
        "modes": np.bincount(mode, minlength=2).tolist(),
        "classes": np.bincount(cls, minlength=4).tolist(),
        "big_at": {str(t): int((big == t).sum()) for t in CLASS_TARGETS},
        "mode_at": {"64": int((d1 == 2 * d2 + 64).sum()), "65": int((d1 == 2 * d2 + 65).sum())},
        "fit_exactly": int(((total == E.SEGMENT_AC_BITS) & (qno > 0) & (dropped == 0)).sum()),
        "next_one_over": int(((nxt == E.SEGMENT_AC_BITS + 1) & (qno < 15)).sum()),
        "waves_15_then_0": int((q2[:, 0] - q2[:, 1] >= 15).sum()),
        "waves_0_then_15": int((q2[:, 1] - q2[:, 0] >= 15).sum()),
        "waves_dropping_then_15": int(((dr2[:, 0] > 0) & (q2[:, 1] == 15)).sum()),
        "waves_15_then_dropping": int(((dr2[:, 1] > 0) & (q2[:, 0] == 15)).sum()),
        "P_bits": int(P[:, 1:].max()).bit_length(),  # the 63 AC products: the kernel forms no other
        "mul_operand_bits": operand[0].bit_length(),
    }
    return out, arrays


_STATED = {}


def stated(system, flags, reverse=False):
    """(the statement's frame of the edge picture, its record over the frame's segments, the census, the census's arrays),
    made once.  The record is dvenc.encode_blocks' with the carriers joined and cut to the system's segments"""
    key = (system, flags, reverse)
    if key not in _STATED:
        g = S.geometry(system)
        recs = []
        fr = E.encode(system, picture(system, reverse), flags, recs)
        fr.setflags(write=False)
        rec = {k: np.concatenate([r[k] for r in recs])[:g.segments * (1 if k in ("qno", "dropped") else 30)] for k in recs[0]}
        rec["levels"] = rec["levels"].astype(np.int16)
        cen, arrays = census(blocks_of(system, picture(system, reverse)), rec, flags)
        arrays = {k: arrays[k] for k in ("big", "d1", "d2", "total", "next")}
        _STATED[key] = (fr, rec, cen, arrays)
    return _STATED[key]


# ---- the statement with one rule swapped ----
def _last_of_most(b):
    return len(b) - 1 - b[::-1].index(max(b))


def _shift_row_17():
    t = E.QUANT_SHIFT.copy()
    t[17] = (1, 1, 1, 1)  # the row of (number 11, class 0) and (number 14, class 1) and of nothing else
    return t


def _limits(i):
    return tuple(v + (k == i) for k, v in enumerate(E.CLASS_LIMITS))


# name -> (what to set in dvenc, the entry named for it, the flags at which that entry must notice)
VARIANTS = {
    "fit <": (lambda: {"fits": lambda total: total < E.SEGMENT_AC_BITS}, "fit", range(4)),
    "mode >=": (lambda: {"mode_rule": lambda d1, d2: d1 >= 2 * d2 + 64}, "mode", (1, 3)),
    "no clip": (lambda: dict(zip(("PAIR_VAL", "PAIR_LEN"), E._words(512)[:2]), clip_level=lambda lv: lv), "clip", (0, 1)),
    "tie to the last": (lambda: {"most_bits": _last_of_most}, "ties", range(4)),
    "class limit 12 + 1": (lambda: {"CLASS_LIMITS": _limits(0)}, "class", (2, 3)),
    "class limit 36 + 1": (lambda: {"CLASS_LIMITS": _limits(1)}, "class", (2, 3)),
    "class limit 144 + 1": (lambda: {"CLASS_LIMITS": _limits(2)}, "class", (2, 3)),
    "shift row 17": (lambda: {"QUANT_SHIFT": _shift_row_17()}, "q11", (3,)),
}
# what the four older pictures (dvenc.PICTURES) let through: conditions, not measurements.  The tie-break is not among
# them: the drop-rule picture's noise has accidental ties (the fixture records where each variant is noticed)
OLD_PICTURES_MUST_NOT_NOTICE = ("fit <", "mode >=", "shift row 17")
OLD_FLAGS = (0, 3)


@contextlib.contextmanager
def variant(name):
    new = VARIANTS[name][0]()
    old = {k: getattr(E, k) for k in new}
    for k, v in new.items():
        setattr(E, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(E, k, v)


def named_for(name, flags):
    """the entry a variant is named for (fit: the one searched for these flags, whatever name it got)"""
    entry = VARIANTS[name][1]
    if entry != "fit":
        return entry
    p = fixture()["params"]["exact"]
    first = next(f for f in range(4) if p[f"fit/{f}"] == p[f"fit/{flags}"])
    return f"fit-{first}"


def old_records():
    """{'picture/flags': dvenc.encode_blocks of it} for the four 525/60 pictures of dvenc.PICTURES at flags 0 and 3.  The
    record determines the frame"""
    return {f"{w}/{flags}": E.encode_blocks(E.picture(S.SYS_525_60, w)[E.block_map()], flags)
            for w in E.PICTURES for flags in OLD_FLAGS}


def noticed_by(plain, swapped):
    """the keys at which two old_records() differ"""
    return [key for key in plain if not all(np.array_equal(plain[key][k], swapped[key][k]) for k in plain[key])]
