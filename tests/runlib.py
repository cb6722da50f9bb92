"""Test-side model of plans with runs (include/mi_rtjpeg.h, mi_rtj_plan_set_runs): the run rule stated in numpy, the
in-order oracle decode it must equal, and packet makers for streams with unchanged blocks."""
import numpy as np

import rtjlib as R


def dims(pkt):
    return int(pkt[6]) | (int(pkt[7]) << 8), int(pkt[8]) | (int(pkt[9]) << 8)


def frame_bytes(w, h):
    return w * h * 3 // 2


def coded_blocks(offs):
    """Block-start offsets (nblocks + 1 entries) -> coded flag per block: a block of length 1 is the byte 0xFF."""
    return np.diff(offs.astype(np.int64)) != 1


def _block_planes(pic, w, h):
    """8x8 block views [by, bx, 8, 8] of the Y, U and V planes of one contiguous picture."""
    ysz, csz = w * h, w * h // 4
    y = pic[:ysz].reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)
    u = pic[ysz:ysz + csz].reshape(h // 16, 8, w // 16, 8).transpose(0, 2, 1, 3)
    v = pic[ysz + csz:ysz + 2 * csz].reshape(h // 16, 8, w // 16, 8).transpose(0, 2, 1, 3)
    return y, u, v


def _block_coords(w, h):
    """(plane, by, bx) of every block in stream order: per macroblock Y0 Y1 Y2 Y3 U V (lib/RTjpeg.c:2701-2745)."""
    mbw = w // 16
    b = np.arange((w // 16) * (h // 16) * 6)
    mb, k = b // 6, b % 6
    mbx, mby = mb % mbw, mb // mbw
    plane = np.where(k < 4, 0, k - 3)
    by = np.where(k < 4, 2 * mby + (k >> 1), mby)
    bx = np.where(k < 4, 2 * mbx + (k & 1), mbx)
    return plane, by, bx


def apply_run_rule(pics, coded, w, h):
    """pics: the run's pictures, each decoded on its own into its slot (picture 0's slot prefilled with the stream's
    previous picture); coded: [len, nblocks] bool.  Returns the pictures after the rule: an unchanged block of picture
    k > 0 is that block of the nearest earlier picture that codes it, else of picture 0's slot."""
    out = [p.copy() for p in pics]
    plane, by, bx = _block_coords(w, h)
    last = np.zeros(coded.shape[1], np.int64)
    for k in range(1, len(out)):
        dst = _block_planes(out[k], w, h)
        miss = ~coded[k]
        for s in np.unique(last[miss]):
            src = _block_planes(out[s], w, h)
            for pl in range(3):
                sel = miss & (last == s) & (plane == pl)
                dst[pl][by[sel], bx[sel]] = src[pl][by[sel], bx[sel]]
        last[coded[k]] = k
    return out


def oracle_in_order(pkts, runs, prev, dec=None):
    """The reference's decode: each run's packets in order into ONE frame that starts as prev[r]; returns every
    picture.  One decoder walks all packets in plan order (the header state a plan applies)."""
    dec = dec or R.OracleDecoder()
    outs, i = [], 0
    for r, n in enumerate(runs):
        frame = prev[r].copy()
        for _ in range(n):
            dec.decode(pkts[i], frame)
            outs.append(frame.copy())
            i += 1
    return outs


def oracle_by_rule(pkts, runs, prev, fill=0x5A, dec=None):
    """The run rule on the CPU: every packet decoded on its own (picture 0 into prev[r], the others into slots of
    `fill`), blocks classified by the oracle's block offsets, then apply_run_rule."""
    dec = dec or R.OracleDecoder()
    outs, i = [], 0
    for r, n in enumerate(runs):
        w, h = dims(pkts[i])
        pics, coded = [], []
        for k in range(n):
            slot = prev[r].copy() if k == 0 else np.full(frame_bytes(w, h), fill, np.uint8)
            coded.append(coded_blocks(dec.block_offsets(pkts[i])))
            dec.decode(pkts[i], slot)
            pics.append(slot)
            i += 1
        outs += apply_run_rule(pics, np.array(coded), w, h)
    return outs


def header(w, h, Q, total):
    return np.array([total & 255, (total >> 8) & 255, (total >> 16) & 255, (total >> 24) & 255, 12, 0,
                     w & 255, w >> 8, h & 255, h >> 8, Q, 0], np.uint8)


def skip_heavy_packet(rng, w, h, Q, n=None):
    """Arbitrary bytes dominated by 0xFF, so that the marker lands at every kind of position (block start, raw byte,
    token, past the packet's end)."""
    nblk = (w // 16) * (h // 16) * 6
    n = int(rng.integers(0, nblk * 40)) if n is None else n
    body = rng.choice(np.array([0xFF, 0xFF, 0xFF, 0x10, 0x7F, 0x41, 0x00], np.uint8), n)
    return np.concatenate([header(w, h, Q, 12 + n), body])


def stream_packets(w, h, Q, n, key_rate, lm, cm, seed=5, amp=3, hold=3):
    """An in-order stream of the oracle encoder with unchanged-block detection; content repeats every `hold` pictures
    so that blocks go unchanged."""
    enc = R.OracleEncoder(w, h, Q, key_rate, lm, cm)
    return [enc.encode(R.synth_frame(w, h, i // hold, seed=seed, amp=amp)) for i in range(n)]
