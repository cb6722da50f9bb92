"""The packets the suite builds to break the transform's arithmetic, as module functions that return packets, so that
every form of the batch transform can be given them (tests/test_gpu_split_edges.py) and not only the form a handful of
small pictures gets by default.  Each builder draws from its generator in a fixed order: with the seeds of the tests
they were lifted from they build the same bytes as before (tests/golden/edge_packet_pins.json, taken from those tests,
tests/test_edge_packets_cpu.py)."""
import os
import re

import numpy as np

import rtjlib as R

CSRC = os.path.join(R.ROOT, "gmerlin-avdecoder_amd", "csrc")

# zig-zag slot -> natural index (row-major 8x8)
ZZ = [0, 8, 1, 2, 9, 16, 24, 17, 10, 3, 4, 11, 18, 25, 32, 40, 33, 26, 19, 12, 5, 6, 13, 20, 27, 34, 41, 48, 56, 49,
      42, 35, 28, 21, 14, 7, 15, 22, 29, 36, 43, 50, 57, 58, 51, 44, 37, 30, 23, 31, 38, 45, 52, 59, 60, 53, 46, 39,
      47, 54, 61, 62, 55, 63]
LOW3 = [k for k in range(64) if (ZZ[k] >> 3) < 3 and (ZZ[k] & 7) < 3]  # slots of rows 0-2 x columns 0-2
LOW4 = [k for k in range(64) if (ZZ[k] >> 3) < 4 and (ZZ[k] & 7) < 4]  # slots of rows 0-3 x columns 0-3


def header(w, h, Q, total):
    return bytes([total & 255, (total >> 8) & 255, (total >> 16) & 255, (total >> 24) & 255, 12, 0,
                  w & 255, w >> 8, h & 255, h >> 8, Q, 0])


def packet_from_body(w, h, Q, body):
    return np.frombuffer(header(w, h, Q, 12 + len(body)) + bytes(body), dtype=np.uint8).copy()


def packet_from_blocks(w, h, Q, blocks):
    return packet_from_body(w, h, Q, b"".join(bytes(b) for b in blocks))


def packet_size(p):
    return int(p[6]) | (int(p[7]) << 8), int(p[8]) | (int(p[9]) << 8)


# --------------------------------------------------------------------------- arbitrary token streams
def adversarial_packet(rng, w, h, Q, lb8, cb8, skip_prob=0.0):
    nblk = (w // 16) * (h // 16) * 6
    body = bytearray()
    for b in range(nblk):
        if rng.random() < skip_prob:
            body.append(255)
            continue
        bt8 = lb8 if (b % 6) < 4 else cb8
        blk = [int(rng.integers(0, 255))] + [int(x) for x in rng.integers(0, 256, bt8)]
        co = bt8 + 1
        while co < 64:
            if rng.random() < 0.3:
                run = int(rng.integers(1, 64 - co + 1))
                blk.append(63 + run)
                co += run
            else:
                blk.append(int(rng.integers(-64, 64)) & 0xFF)
                co += 1
        body += bytes(blk)
    total = 12 + len(body)
    hdr = bytes([total & 255, (total >> 8) & 255, (total >> 16) & 255, (total >> 24) & 255, 12, 0,
                 w & 255, w >> 8, h & 255, h >> 8, Q, 0])
    return np.frombuffer(hdr + bytes(body), dtype=np.uint8).copy()


ADVERSARIAL_QUALITIES = (1, 2, 3, 8, 31, 129, 192, 255)  # where the int16 narrowing of RTjpeg_s2b and DESCALE shows


def adversarial_packets(seed=2025):
    """(packets, their qualities): random bytes, random runs, some 0xFF, two geometries per quality"""
    rng = np.random.default_rng(seed)
    pkts, qs = [], []
    for Q in ADVERSARIAL_QUALITIES:
        _, _, lb8, cb8, _, _ = R.oracle_tables(Q)
        for (w, h) in ((48, 32), (160, 16)):
            pkts.append(adversarial_packet(rng, w, h, Q, lb8, cb8, skip_prob=0.1))
            qs.append(Q)
    return pkts, qs


# --------------------------------------------------------------------------- the chunked index: long, skipped, mixed blocks
CHUNK_CASES = [(255, "long"), (255, "skip"), (255, "mix"), (100, "long"), (100, "mix"), (255, "runs")]


def chunk_boundary_packets(seed=77, w=1024, h=256, cases=CHUNK_CASES, pattern=(16, 16, 4, 2)):
    """maximal 64-byte blocks (no zero runs), minimal 1-byte (0xFF) blocks, and mixtures, so macroblocks straddle every
    chunk boundary differently (1024x256: long-block packets span ~110 chunks).  pattern: the format's unit as (width,
    height, luma blocks, chroma blocks) — 4:2:0's Y Y Y Y Cb Cr unless said otherwise; lb8 / cb8 raw bytes by block type"""
    rng = np.random.default_rng(seed)
    uw, uh, nluma, nchroma = pattern
    nblk = (w // uw) * (h // uh) * (nluma + nchroma)
    pkts = []
    for Q, mode in cases:
        _, _, lb8, cb8, _, _ = R.oracle_tables(Q)
        body = bytearray()
        for b in range(nblk):
            bt8 = lb8 if (b % (nluma + nchroma)) < nluma else cb8
            kind = mode if mode != "mix" else ["long", "skip", "short", "runs"][int(rng.integers(0, 4))]
            if kind == "skip":
                body.append(255)
                continue
            blk = [int(rng.integers(0, 255))] + [int(x) for x in rng.integers(0, 256, bt8)]
            left = 63 - bt8
            if kind == "long":      # every remaining coefficient spelled out
                blk += [int(x) & 0xFF for x in rng.integers(-64, 64, left)]
            elif kind == "short":   # one run to the end
                blk.append(63 + left)
            else:                   # unit runs: many weight-1 run tokens (byte 64)
                while left > 0:
                    r = int(rng.integers(1, min(left, 3) + 1))
                    blk.append(63 + r)
                    left -= r
            body += bytes(blk)
        pkts.append(packet_from_body(w, h, Q, body))
    return pkts


# the same for the serial walker of the other two formats (MI_RTJ_FMT_*: 1 = 4:2:2, Y Y Cb Cr; 2 = greyscale, luma only),
# at sizes where it stores its gathered offsets more than once and the last store is partial: 132 and 153 blocks
FORMAT_BOUNDARY_SHAPES = {1: (176, 24, (16, 8, 2, 2)), 2: (136, 72, (8, 8, 1, 0))}


def format_boundary_packets(fmt, seed=78):
    """CHUNK_CASES' six packets (long, skip, mix and runs at Q 255; long and mix at Q 100) in the format's block pattern"""
    w, h, pattern = FORMAT_BOUNDARY_SHAPES[fmt]
    return chunk_boundary_packets(seed=seed, w=w, h=h, pattern=pattern)


# --------------------------------------------------------------------------- the low-4x4 forms and their boundary
LOW_4X4_QUALITIES = (255, 200, 150, 3)
LOW_4X4_SHAPES = ((512, 64, "one"), (1024, 32, "flat_then_busy"), (512, 32, "dc_only"), (1024, 48, "three_then_four"))


def low_4x4_packets(seed=99, qualities=LOW_4X4_QUALITIES, shapes=LOW_4X4_SHAPES):
    """Whole waves qualify for the four-input transform, whole waves do not, a wave stops qualifying from one macroblock
    group to the next, and the single coefficient sits on every one of the 63 AC slots (inside, on the edge of and
    outside the 4x4) with values where the int16 narrowing shows."""
    rng = np.random.default_rng(seed)
    pkts = []
    for Q in qualities:
        _, _, lb8, cb8, _, _ = R.oracle_tables(Q)
        for (w, h, mode) in shapes:
            nmb = (w // 16) * (h // 16)
            blocks = []
            for mb in range(nmb):
                for k in range(6):
                    bt8 = lb8 if k < 4 else cb8
                    blk = [int(rng.integers(0, 255))] + [0] * bt8  # DC, raw bytes zero unless chosen below
                    if mode == "one":
                        slot = 1 + (mb * 6 + k) % 63          # the one AC coefficient: every slot in turn
                    elif mode == "flat_then_busy":
                        slot = int(rng.integers(1, 4)) if mb < nmb // 2 else int(rng.integers(1, 64))
                    elif mode == "three_then_four":
                        # zig-zag slots inside the low 3x3 (the three-input transform), then, from the second
                        # third of the picture on, slots on row 3 or column 3 of the low 4x4 as well (the
                        # four-input one), then one block per macroblock group anywhere (the full one)
                        in3 = (1, 2, 3, 4, 5, 7, 8, 12)
                        edge4 = (6, 9, 11, 13, 17, 18, 24)
                        if mb < nmb // 3:
                            slot = in3[int(rng.integers(0, len(in3)))]
                        elif mb < 2 * nmb // 3:
                            slot = edge4[int(rng.integers(0, len(edge4)))] if rng.random() < 0.1 else in3[int(rng.integers(0, len(in3)))]
                        else:
                            slot = int(rng.integers(1, 64)) if (mb % 32 == 5 and k == 2) else in3[int(rng.integers(0, len(in3)))]
                    else:
                        slot = 0
                    val = int(rng.integers(-128, 64)) & 0xFF if slot else 0
                    if slot and slot <= bt8:
                        blk[slot] = val
                        blk.append(63 + 63 - bt8)             # one run over all token slots
                    elif slot:
                        before = slot - bt8 - 1
                        if before:
                            blk.append(63 + before)
                        blk.append(val if val < 64 or val > 127 else 1)
                        after = 63 - slot
                        if after:
                            blk.append(63 + after)
                    else:
                        blk.append(63 + 63 - bt8)
                    blocks.append(blk)
            pkts.append(packet_from_blocks(w, h, Q, blocks))
    return pkts


# --------------------------------------------------------------------------- DC-only blocks the encoder never writes
DC_SPELLING_QUALITIES = (255, 192, 128, 60)


def dc_spelling_packets(seed=12, w=512, h=64, qualities=DC_SPELLING_QUALITIES):
    """DC followed by zero coefficients written out, by several short runs, by a run that overshoots, or with a
    non-zero raw byte: none is the encoder's "DC, zeros, one run" form; mixed with blocks that are."""
    rng = np.random.default_rng(seed)
    nblk = (w // 16) * (h // 16) * 6
    pkts = []
    for Q in qualities:
        _, _, lb8, cb8, _, _ = R.oracle_tables(Q)
        body = bytearray()
        for b in range(nblk):
            bt8 = lb8 if (b % 6) < 4 else cb8
            left = 63 - bt8
            kind = int(rng.integers(0, 7))
            dc = int(rng.integers(0, 255))
            if kind <= 2:    # the encoder's form
                blk = [dc] + [0] * bt8 + [63 + left]
            elif kind == 3:  # zeros spelled out, then a shorter run
                k = int(rng.integers(1, min(left, 6)))
                blk = [dc] + [0] * bt8 + [0] * k + ([63 + left - k] if left - k else [])
            elif kind == 4:  # two runs
                k = int(rng.integers(1, left)) if left > 1 else 1
                blk = [dc] + [0] * bt8 + [63 + k] + ([63 + left - k] if left - k else [])
            elif kind == 5:  # a run that overshoots the block
                blk = [dc] + [0] * bt8 + [127]
            else:            # one non-zero coefficient
                blk = [dc] + [0] * bt8 + [3, 63 + left - 1] if left > 1 else [dc] + [0] * bt8 + [3]
                if bt8:
                    blk[1 + int(rng.integers(0, bt8))] = int(rng.integers(1, 256)) if rng.random() < 0.5 else 0
            body += bytes(x & 0xFF for x in blk)
        pkts.append(packet_from_body(w, h, Q, body))
    return pkts


# --------------------------------------------------------------------------- the packed passes' 16-bit budget
class Budget:
    """The constants of the packed passes' range test, read from csrc/rtj_idct_pk.h, and the kernel's own sum."""

    def __init__(self, csrc=CSRC):
        hdr = open(os.path.join(csrc, "rtj_idct_pk.h")).read()
        slack, dc4 = (int(v) for v in re.search(r"kPkBudget = 4 \* \(32767 - (\d+) - (\d+)\)", hdr).groups())
        classw = [int(v) for v in re.search(r"kPkClassW\[8\] = \{([^}]*)\}", hdr).group(1).split(",")]
        rowk = [int(v) for v in re.search(r"rowk\[8\] = \{([^}]*)\}", hdr).group(1).split(",")]
        cls = [[int(v) for v in row.split(",")] for row in re.findall(r"^\s*\{(\d, \d, \d, \d)\},", hdr, re.M)]
        self.budget = 4 * (32767 - slack - dc4)  # kPkBudget
        self.budget3 = self.budget // 4          # the three-input form's: weight 1 per coefficient
        self.wnat = np.array([classw[cls[rowk[n >> 3]][(n & 7) >> 1]] for n in range(64)], np.int64)

    @staticmethod
    def coefficients(tok, q):
        """dequantised coefficients per zig-zag slot as the kernel stores them (int16); q: natural order"""
        return (((tok.astype(np.int64) * q[ZZ].astype(np.int64)) + 32768) % 65536) - 32768

    def weighted(self, tok, q):  # the kernel's sum for a block given its token values per zig-zag slot (slot 0: DC byte)
        return int((self.wnat[ZZ] * np.abs(self.coefficients(tok, q))).sum())


def block_bytes(tok, bt8):
    out = [int(tok[0])] + [int(tok[k]) & 0xFF for k in range(1, bt8 + 1)]
    run = 0
    for k in range(bt8 + 1, 64):
        if tok[k] == 0:
            run += 1
            continue
        if run:
            out.append(63 + run)
            run = 0
        out.append(int(tok[k]) & 0xFF)
    if run:
        out.append(63 + run)
    return out


def budget_block(rng, B, q, bt8, slots, kind):
    """kind: target position of the block's sum relative to the budget.  Returns (token values, the sum)."""
    budget, wnat, zz, weighted = B.budget, B.wnat, ZZ, B.weighted
    tok = np.zeros(64, np.int64)
    tok[0] = rng.integers(0, 255)
    n = int(rng.integers(1, min(len(slots), 24) + 1))
    pick = rng.choice(slots, n, replace=False)
    tok[pick] = rng.integers(1, 64, n) * rng.choice([-1, 1], n)
    tok[0] = max(int(tok[0]), 0)
    target = {"in": 0.4, "edge_in": 1.0, "edge_out": 1.0, "out": 2.5}[kind] * budget
    for _ in range(40):  # scale the AC tokens towards the target (token range -128..63; 64..127 are runs)
        s = weighted(tok, q)
        ac = s - int(wnat[0]) * abs(((int(tok[0]) * int(q[0]) + 32768) % 65536) - 32768)
        if ac <= 0:
            break
        f = (target - (s - ac)) / ac
        new = np.clip(np.round(tok[1:] * f), -128, 63)
        new[(tok[1:] != 0) & (new == 0)] = 1
        if np.array_equal(new, tok[1:]):
            break
        tok[1:] = new
    if kind.startswith("edge"):
        k = int(pick[np.argmin(wnat[[zz[p] for p in pick]] * q[[zz[p] for p in pick]])])  # the finest step available
        step = 1 if tok[k] > 0 else -1
        for _ in range(400):
            s = weighted(tok, q)
            if kind == "edge_in" and s > budget and abs(tok[k]) > 1:
                tok[k] -= step
            elif kind == "edge_in" and s <= budget and -128 < tok[k] + step < 64 and weighted(np.where(np.arange(64) == k, tok + step, tok), q) <= budget:
                tok[k] += step
            elif kind == "edge_out" and s <= budget and -128 < tok[k] + step < 64:
                tok[k] += step
            elif kind == "edge_out" and s > budget and abs(tok[k]) > 1 and weighted(np.where(np.arange(64) == k, tok - step, tok), q) > budget:
                tok[k] -= step
            else:
                break
    return tok, weighted(tok, q)


BUDGET_QUALITIES = (255, 120)
BUDGET_MIXES = ((1024, 64, "mixed"), (512, 32, "all_in"), (1024, 32, "one_out_per_group"))


def budget_packets(seed=2024, qualities=BUDGET_QUALITIES, mixes=BUDGET_MIXES, strict_in=False):
    """Blocks built from token values so that the kernel's own weighted sum lands well inside, just inside (the largest
    sum not above the budget that stepping one token reaches), just outside and well outside the budget, with sparse and
    dense coefficient patterns and both signs; most waves hold blocks of several kinds, some are all inside.  Chroma
    blocks get the same treatment with coefficients in the low 3x3 only and anywhere.  (Stepping one token does not
    always reach the inside: a few "just inside" blocks of the mix "all_in" end up above the budget.  strict_in draws
    such a block again until it is inside — other packets than the pinned ones, and a mix that is what its name says.)

    Returns (packets, seen, meta): seen counts the blocks inside, outside and within 2 % of the budget; meta[i] says of
    packet i its mix, and per block (macroblock-major, six to a macroblock) its sum and whether a dequantised
    coefficient lies outside rows 0-3 x columns 0-3."""
    B = Budget()
    rng = np.random.default_rng(seed)
    outside4 = np.array([k not in LOW4 for k in range(64)])
    pkts, meta, seen = [], [], {"in": 0, "out": 0, "near": 0}
    for Q in qualities:
        liqt, ciqt, lb8, cb8, _, _ = R.oracle_tables(Q)
        for (w, h, mix) in mixes:
            nmb = (w // 16) * (h // 16)
            blocks, sums, beyond = [], [], []
            for mb in range(nmb):
                for k in range(6):
                    q, bt8 = (liqt, lb8) if k < 4 else (ciqt, cb8)
                    slots = list(range(1, 64)) if (k < 4 or mb % 3) else LOW3[1:]
                    if mix == "all_in":
                        kind = ("in", "edge_in")[int(rng.integers(0, 2))]
                    elif mix == "one_out_per_group":
                        kind = ("edge_out" if k in (1, 4) else "out") if mb % 32 == 7 else "in"
                    else:
                        kind = ("in", "edge_in", "edge_out", "out")[int(rng.integers(0, 4))]
                    tok, s = budget_block(rng, B, q, bt8, slots, kind)
                    while strict_in and mix == "all_in" and s > B.budget:
                        tok, s = budget_block(rng, B, q, bt8, slots, kind)
                    seen["in" if s <= B.budget else "out"] += 1
                    seen["near"] += abs(s - B.budget) < B.budget // 50
                    sums.append(s)
                    beyond.append(bool((B.coefficients(tok, q)[outside4] != 0).any()))
                    blocks.append(block_bytes(tok, bt8))
            pkts.append(packet_from_blocks(w, h, Q, blocks))
            meta.append(dict(mix=mix, Q=Q, w=w, h=h, budget=B.budget, sums=np.array(sums, np.int64),
                             beyond_low4=np.array(beyond)))
    return pkts, seen, meta


def pinned_sets():
    """name -> packets, as the tests that build them do (their seeds): what tests/golden/edge_packet_pins.json pins"""
    return {"low4x4": low_4x4_packets(), "budget": budget_packets()[0], "chunks": chunk_boundary_packets(),
            "dc_spellings": dc_spelling_packets(), "adversarial": adversarial_packets()[0]}
