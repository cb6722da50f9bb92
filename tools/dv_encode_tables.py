"""Derives the DV encoder's constant tables (tests/dvenc.py and csrc/dv_encode_tables.h hold them as integer literals).

    python tools/dv_encode_tables.py            # prints both spellings

The encoder's forward transform is a scaled butterfly: output (r, h) of a block is ratio(mode, r, h) times the orthonormal
transform's.  The ratio is measured here by pushing every basis picture through the butterfly in real arithmetic; the
quantiser's multiplier for scan position k is round(2^20 W / ratio) with the closed-form weight W of oracle/dv_oracle.c's
header comment (w(h) w(v) / 2, v = r in 8-8 and 2 (r >> 1) in 2-4-8).  tests/test_dv_encode_cpu.py pins what the literals
make of a picture to the closed form, so a wrong entry here fails there."""
import math

import numpy as np

SCAN88 = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
          62, 63]
SCAN248 = [0, 8, 1, 9, 16, 24, 2, 10, 17, 25, 32, 40, 48, 56, 33, 41, 18, 26, 3, 11, 4, 12, 19, 27, 34, 42, 49, 57, 50, 58, 35,
           43, 20, 28, 5, 13, 6, 14, 21, 29, 36, 44, 51, 59, 52, 60, 37, 45, 22, 30, 7, 15, 23, 31, 38, 46, 53, 61, 54, 62, 39,
           47, 55, 63]
FRAC = 20      # fractional bits of a multiplier
PRESCALE = 8   # pixels enter the butterfly times this
# cos(pi/4), sin(pi/8), sqrt(2) sin(pi/8), sqrt(2) cos(pi/8): as 12-bit fractions 2896, 1567, 2217, 5352
C707, C383, C541, C1307 = (math.cos(math.pi / 4), math.sin(math.pi / 8), math.sqrt(2) * math.sin(math.pi / 8),
                           math.sqrt(2) * math.cos(math.pi / 8))


def fdct8(x):
    """the scaled 8-point forward butterfly along the last axis, real arithmetic"""
    t0, t7 = x[..., 0] + x[..., 7], x[..., 0] - x[..., 7]
    t1, t6 = x[..., 1] + x[..., 6], x[..., 1] - x[..., 6]
    t2, t5 = x[..., 2] + x[..., 5], x[..., 2] - x[..., 5]
    t3, t4 = x[..., 3] + x[..., 4], x[..., 3] - x[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    z1 = (t12 + t13) * C707
    o = [None] * 8
    o[0], o[4], o[2], o[6] = t10 + t11, t10 - t11, t13 + z1, t13 - z1
    t10, t11, t12 = t4 + t5, t5 + t6, t6 + t7
    z5 = (t10 - t12) * C383
    z2, z4, z3 = t10 * C541 + z5, t12 * C1307 + z5, t11 * C707
    z11, z13 = t7 + z3, t7 - z3
    o[5], o[3], o[1], o[7] = z13 + z2, z13 - z2, z11 + z4, z11 - z4
    return np.stack(o, -1)


def fdct4(x):
    """its even half: a scaled 4-point transform"""
    t10, t13, t11, t12 = x[..., 0] + x[..., 3], x[..., 0] - x[..., 3], x[..., 1] + x[..., 2], x[..., 1] - x[..., 2]
    z1 = (t12 + t13) * C707
    return np.stack([t10 + t11, t13 + z1, t10 - t11, t13 - z1], -1)


def butterfly(px, mode):
    t = fdct8(px * PRESCALE)                      # along the lines
    t = np.swapaxes(t, -1, -2)                    # [h][y]
    if not mode:
        return np.swapaxes(fdct8(t), -1, -2)
    s, d = t[..., 0::2] + t[..., 1::2], t[..., 0::2] - t[..., 1::2]
    out = np.empty_like(t)
    out[..., 0::2], out[..., 1::2] = fdct4(s), fdct4(d)
    return np.swapaxes(out, -1, -2)


def dmat(n):
    return np.array([[math.sqrt((1 if k == 0 else 2) / n) * math.cos((2 * i + 1) * k * math.pi / (2 * n)) for i in range(n)]
                     for k in range(n)])


def orthonormal(px, mode):
    D8, D4 = dmat(8), dmat(4)
    t = px @ D8.T
    if not mode:
        return D8 @ t
    out = np.empty((8, 8))
    out[0::2] = D4 @ (t[0::2] + t[1::2]) / math.sqrt(2)
    out[1::2] = D4 @ (t[0::2] - t[1::2]) / math.sqrt(2)
    return out


def tables():
    cs = [math.cos(m * math.pi / 16) for m in range(8)]
    w = [1, cs[4] / (4 * cs[7] * cs[2]), cs[4] / (2 * cs[6]), 1 / (2 * cs[5]), 7 / 8, cs[4] / cs[3], cs[4] / cs[2], cs[4] / cs[1]]
    rng = np.random.default_rng(1)
    mult = []
    for mode in (0, 1):
        px = rng.uniform(-128, 127, (8, 8))
        got, want = butterfly(px, mode), orthonormal(px, mode)
        ratio = np.empty(64)
        # the orthonormal transform as a matrix; solving with it gives the picture of one coefficient
        cols = np.array([orthonormal(e.reshape(8, 8), mode).ravel() for e in np.eye(64)]).T
        for nat in range(64):
            basis = np.zeros(64)
            basis[nat] = 1.0
            p = np.linalg.solve(cols, basis).reshape(8, 8)
            out = butterfly(p, mode).ravel()
            ratio[nat] = out[nat]
            out[nat] = 0
            assert np.abs(out).max() < 1e-9
        assert np.allclose(got.ravel() / ratio, want.ravel())
        m = []
        for nat in range(64):
            r, h = nat >> 3, nat & 7
            v = 2 * (r >> 1) if mode else r
            m.append(int(math.floor((1 << FRAC) * (w[h] * w[v] / 2) / ratio[nat] + 0.5)))
        mult.append(m)
    return mult


def main():
    mult = tables()
    inv = [[s.index(nat) for nat in range(64)] for s in (SCAN88, SCAN248)]
    print("# tests/dvenc.py")
    for name, t in (("MULT_NAT", mult), ("POS_NAT", inv)):
        print(f"{name} = (")
        for row in t:
            print("    (" + ", ".join(str(x) for x in row) + "),")
        print(")")
    print("// csrc/dv_encode_tables.h")
    for name, t in (("kEncMult", mult), ("kEncPos", inv)):
        print(f"constexpr uint32_t {name}[2][64] = {{")
        for row in t:
            print("    {" + ", ".join(str(x) for x in row) + "},")
        print("};")


if __name__ == "__main__":
    main()
