#!/usr/bin/env python3
"""Writes tests/golden/dv_encode_edges.json: the searched parameters of the edge segments of tests/dvenc_edges.py and what
the statement tests/dvenc.py does on the edge pictures made of them.  Nothing here is a tolerance somebody chose.
  params      class: per target big = max P >> 20 (11, 12, 35, 36, 143, 144) the horizontal basis function and the amplitude
              in quarters that give it, the first found.  qno: per quantisation number the first seeded segment that
              chooses it at flags 3 with nothing dropped (noisy blocks on a gradient; binary blocks on flat 128 where
              those find none).  exact: per flags the first seeded noise segment whose chosen number q > 0 needs exactly
              2,680 bits (fit) and the first that needs exactly 2,681 at q + 1 (next).
  census      per system and flags, dvenc_edges.census of the edge picture.
  deviation   per flags, the largest |level - F W / 2^s| on the 525/60 edge frame where the level is not clipped
              (dvenc_check.deviation), rounded up to 0.01.  The test's condition is "below 1" whatever this file says.
  old_pictures_notice   per variant of the statement (dvenc_edges.VARIANTS), which of the four pictures of dvenc.PICTURES
              (525/60, 'picture/flags' at flags 0 and 3) are encoded differently under it."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dvenc as E  # noqa: E402
import dvenc_check as K  # noqa: E402
import dvenc_edges as X  # noqa: E402
import dvfloat as F  # noqa: E402
import dvsys as S  # noqa: E402

CANDIDATES = 1500


def search_class():
    cand = [(h, a) for h in range(1, 8) for a in range(1, 509)]
    px = np.array([X.class_block(h, a) for h, a in cand])
    for flags in range(4):
        assert not E.choose_mode(px, flags).any()
    mode = np.zeros(len(cand), np.int64)
    P, _ = E.products(E.transform(px, mode), mode)
    big = P[:, 1:].max(axis=1) >> E.FRAC
    return {str(t): list(cand[int(np.flatnonzero(big == t)[0])]) for t in X.CLASS_TARGETS}


def candidates(kind, master, lo, hi, kmax):
    rng = np.random.default_rng(master)
    return [[kind, seed, int(rng.integers(lo, hi)), int(rng.integers(1, kmax + 1))] for seed in range(CANDIDATES)]


def search_qno():
    found = {}
    for cand in (candidates("noise", 6, 15, 128, 20), candidates("binary", 8, 0, 100, 20)):
        r = E.encode_blocks(np.concatenate([X.searched_segment(p) for p in cand]), 3)
        for q in range(16):
            hit = np.flatnonzero((r["qno"] == q) & (r["dropped"] == 0))
            if str(q) not in found and hit.size:
                found[str(q)] = cand[int(hit[0])]
    return found


def search_exact():
    cand = candidates("noise", 5, 1, 41, 20)
    px = np.concatenate([X.searched_segment(p) for p in cand])
    found = {}
    for flags in range(4):
        r = E.encode_blocks(px, flags)
        P, neg = E.products(E.transform(px, r["mode"]), r["mode"])
        q = r["qno"]
        total = E.block_bits(r["levels"]).reshape(-1, 30).sum(axis=1)
        nxt = E.block_bits(E.quantise(P, neg, r["cls"], np.repeat(np.minimum(q + 1, 15), 30))).reshape(-1, 30).sum(axis=1)
        fit = np.flatnonzero((total == E.SEGMENT_AC_BITS) & (q > 0) & (r["dropped"] == 0))
        one_over = np.flatnonzero((nxt == E.SEGMENT_AC_BITS + 1) & (q < 15))
        print(f"flags {flags}: {fit.size} segments fit exactly, {one_over.size} are one bit over at the next number")
        found[f"fit/{flags}"], found[f"next/{flags}"] = cand[int(fit[0])], cand[int(one_over[0])]
    return found


def old_pictures_notice():
    out = {}
    plain = X.old_records()
    for name in X.VARIANTS:
        with X.variant(name):
            out[name] = X.noticed_by(plain, X.old_records())
    return out


def main():
    params = {"class": search_class(), "qno": search_qno(), "exact": search_exact()}
    out = {"params": params}
    with open(X.FIXTURE, "w") as f:  # dvenc_edges builds from the file
        json.dump(out, f)
    X.fixture.cache_clear()
    X.segments.cache_clear()
    out["entries"] = list(X.segments()[0])
    out["census"] = {f"{s}/{flags}": X.stated(s, flags)[2] for s in S.SYSTEMS for flags in range(4)}
    out["step"] = {"deviation": K.STEP_DEVIATION}
    out["deviation"] = {str(flags): F.up(K.deviation("edges", flags), K.STEP_DEVIATION) for flags in range(4)}
    out["old_pictures_notice"] = old_pictures_notice()
    def lines(d, depth):  # one line per entry down to the second level
        pad = " " * depth
        return "{\n" + ",\n".join(f"{pad}{json.dumps(k)}: {lines(v, depth + 1) if depth < 2 and isinstance(v, dict) else json.dumps(v)}"
                                  for k, v in d.items()) + "\n" + pad[1:] + "}"
    text = lines(out, 1) + "\n"
    assert json.loads(text) == json.loads(json.dumps(out))
    with open(X.FIXTURE, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
