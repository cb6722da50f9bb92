"""Test-side model of runs on 4:2:2 and greyscale plans (include/mi_rtjpeg.h, mi_rtj_plan_set_runs_fmt): the in-order
decode of a run by the restatement of tests/rtjfmt.py, and — independently — the run rule on top of per-packet decodes,
with a statement of every block's rectangle in the format's stream order.  A helper, not a test; runlib.py is the 4:2:0
one."""
import numpy as np

import rtjfmt as F
import rtjfmt_enc as E
import rtjlib as R

FILL = 0x5A  # slots of pictures k > 0 start as this: an unchanged block that nobody copies shows


def dims(pkt):
    return F.header_of(pkt)[:2]


def block_rects(fmt, w, h):
    """(plane, y0, x0) of every block's 8x8 rectangle in stream order.  Planes: 0 Y (w x h), 1 Cb, 2 Cr (w/2 x h).
    4:2:2 (lib/RTjpeg.c:2639-2686): per 16x8 macroblock Y left, Y right, Cb, Cr; greyscale (:2751-2772): raster order."""
    if fmt == F.FMT_422:
        per_row = w // 16
        b = np.arange(per_row * (h // 8) * 4)
        mb, k = b // 4, b % 4
        i, j = mb // per_row, mb % per_row
        plane = np.where(k < 2, 0, k - 1)
        x0 = np.where(k < 2, 16 * j + 8 * k, 8 * j)
        return plane, 8 * i, x0
    assert fmt == F.FMT_GREY
    per_row = w // 8
    b = np.arange(per_row * (h // 8))
    return np.zeros(b.size, np.int64), 8 * (b // per_row), 8 * (b % per_row)


def plane_views(fmt, pic, w, h):
    """2-D views of the planes of one contiguous picture: [Y] or [Y, Cb, Cr]"""
    y, cb, cr = F.split(fmt, pic, w, h)
    if fmt == F.FMT_GREY:
        return [y.reshape(h, w)]
    return [y.reshape(h, w), cb.reshape(h, w // 2), cr.reshape(h, w // 2)]


def _block_views(fmt, pic, w, h):
    """the planes as [block row, block column, 8, 8]"""
    return [p.reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).transpose(0, 2, 1, 3) for p in plane_views(fmt, pic, w, h)]


def coded_blocks(fmt, pkt):
    """coded flag per block: a block of index length 1 is the byte 0xFF (unchanged)"""
    return np.diff(E.block_offsets(fmt, pkt)) != 1


def has_both_kinds(fmt, pkts, runs):
    """True if some picture k > 0 of some run has unchanged blocks and coded blocks (what a test's input must hold)"""
    i = 0
    for n in runs:
        for k in range(n):
            c = coded_blocks(fmt, pkts[i + k])
            if k > 0 and c.any() and not c.all():
                return True
        i += n
    return False


def apply_run_rule(fmt, pics, coded, w, h):
    """pics: the run's pictures, each decoded on its own into its slot (picture 0's slot prefilled with the stream's
    previous picture); coded: [len, nblocks] bool.  Returns (the pictures after the rule, blocks copied): an unchanged
    block of picture k > 0 is that block of the nearest earlier picture that codes it, else of picture 0's slot."""
    out = [p.copy() for p in pics]
    plane, y0, x0 = block_rects(fmt, w, h)
    by, bx = y0 // 8, x0 // 8
    last = np.zeros(coded.shape[1], np.int64)
    copied = 0
    for k in range(1, len(out)):
        dst = _block_views(fmt, out[k], w, h)
        miss = ~coded[k]
        copied += int(miss.sum())
        for s in np.unique(last[miss]):
            src = _block_views(fmt, out[s], w, h)
            for pl in range(len(dst)):
                sel = miss & (last == s) & (plane == pl)
                dst[pl][by[sel], bx[sel]] = src[pl][by[sel], bx[sel]]
        last[coded[k]] = k
    return out, copied


def in_order(fmt, pkts, runs, prev, make=F.Restated):
    """The reference's decode: each run's packets in order, by one decoder per run, into ONE picture that starts as
    prev[r]; returns every picture.  make: F.Restated, or F.RefFmt where oracle/_ref was built."""
    outs, i = [], 0
    for r, n in enumerate(runs):
        dec, frame = make(fmt), prev[r].copy()
        for _ in range(n):
            dec.decode(pkts[i], frame)
            outs.append(frame.copy())
            i += 1
    return outs


def by_rule(fmt, pkts, runs, prev, fill=FILL):
    """The run rule on the CPU: every packet decoded on its own (picture 0 into prev[r], the others into slots of
    `fill`), blocks classified by their index lengths, then apply_run_rule.  Returns (pictures, blocks copied)."""
    outs, copied, i = [], 0, 0
    for r, n in enumerate(runs):
        w, h = dims(pkts[i])
        dec, pics, coded = F.Restated(fmt), [], []
        for k in range(n):
            slot = prev[r].copy() if k == 0 else np.full(F.plane_bytes(fmt, w, h), fill, np.uint8)
            coded.append(coded_blocks(fmt, pkts[i]))
            dec.decode(pkts[i], slot)
            pics.append(slot)
            i += 1
        got, c = apply_run_rule(fmt, pics, np.array(coded), w, h)
        outs += got
        copied += c
    return outs, copied


def independent(fmt, pkts, prev_first, runs, fill=FILL):
    """A plan without runs: every packet into its own slot (picture 0 of what were the runs: prev[r], the others `fill`);
    one decoder sees the headers in plan order."""
    dec, outs, i = F.Restated(fmt), [], 0
    for r, n in enumerate(runs):
        w, h = dims(pkts[i])
        for k in range(n):
            slot = prev_first[r].copy() if k == 0 else np.full(F.plane_bytes(fmt, w, h), fill, np.uint8)
            dec.decode(pkts[i], slot)
            outs.append(slot)
            i += 1
    return outs


def header(w, h, Q, total):
    return np.array([total & 255, (total >> 8) & 255, (total >> 16) & 255, (total >> 24) & 255, 12, 0,
                     w & 255, w >> 8, h & 255, h >> 8, Q, 0], np.uint8)


def is_luma(fmt, b):
    return fmt == F.FMT_GREY or (b % 4) < 2


def crafted_run(fmt, n, w, h, Q=100, seed=0):
    """Packets of 0xFF and coded blocks by a pattern, in the format's block order: block 0 coded only in picture 0,
    block 1 only in the last, block 2 never, block 3 every 64th picture, the rest at random.  (24 x 8 greyscale has the
    first three of them.)"""
    rng = np.random.default_rng([seed, fmt, n])
    _, _, lb8, cb8, _, _ = R.oracle_tables(Q)
    nblk = F.nblocks(fmt, w, h)
    pkts = []
    for k in range(n):
        body = bytearray()
        for b in range(nblk):
            coded = {0: k == 0, 1: k == n - 1, 2: False, 3: k % 64 == 0}.get(b, rng.random() < 0.3)
            if not coded:
                body.append(255)
                continue
            bt8 = lb8 if is_luma(fmt, b) else cb8
            body += bytes([int(rng.integers(0, 255))] + [int(x) for x in rng.integers(0, 4, bt8)] + ([126 - bt8] if bt8 < 63 else []))
        pkts.append(np.concatenate([header(w, h, Q, 12 + len(body)), np.frombuffer(bytes(body), np.uint8)]))
    return pkts


def rand_pic(fmt, w, h, seed):
    return np.random.default_rng([seed, fmt, w, h]).integers(0, 256, F.plane_bytes(fmt, w, h), dtype=np.uint8)
