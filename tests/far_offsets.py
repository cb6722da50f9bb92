"""Where the objects of a test lie in a buffer that crosses byte 2^31 and byte 2^32: one layout helper for the tests of
far offsets (tests/test_gpu_far_offsets.py, tests/test_gpu_dv_far_offsets.py; tests/test_far_offsets_cpu.py holds the
helper itself to its rules).

The kernels add 32-bit lane offsets to a 64-bit wave-uniform base.  A base narrowed to 32 bits is invisible below 4 GiB,
and so is a frame index multiplied in 32 bits.  The buffers here are 2^32 + 2^26 bytes; `hipMalloc` touches none of it,
and only the windows a layout names are ever set, uploaded or read back.

A layout places k objects (pictures of an output buffer, or packets of a stream buffer) by role, for each line L in
(2^31, 2^32):

  straddle L   the object starts below L and ends above it (packets: with the 12-byte header across L, or the data)
  at L         the object starts exactly at L
  above L      the object lies wholly above L, and not at it
  near         the object lies below 2^31

One object straddling a line and another starting at it would share the byte at the line, and so would two packets that
straddle it with different parts.  So a layout comes in VARIANTS: pictures "straddle" and "at", packets "header", "data"
and "at"; every variant has the near and the above objects, and a test runs all variants of its kind.

Every object has a guard of GUARD bytes on both sides.  An object that reaches above 2^32 has an ALIAS window, 2^32 below
the part of it that lies above: where a store or a load through an offset narrowed to 32 bits lands.  It is inside the
buffer, so a wrong kernel writes wrong bytes in bounds.  No alias window meets an object or a guard."""
import numpy as np

LINES = (1 << 31, 1 << 32)
WRAP = 1 << 32
BUFFER_BYTES = (1 << 32) + (1 << 26)
GUARD = 256
WINDOW_BUDGET = 64 << 20  # bytes of all windows of one buffer: what a test may set, upload and read back

NEAR_BASE = 1 << 30          # near objects lie from here on: clear of the alias windows, which lie below 2^26
REGION_GAP = 1 << 24         # "above L" objects start this far above L: clear of what straddles L or starts at it
MAX_OBJECT = 1 << 23

PICTURE_VARIANTS = ("straddle", "at")
PACKET_VARIANTS = ("header", "data", "at")


def variants(kind):
    return PICTURE_VARIANTS if kind == "pictures" else PACKET_VARIANTS


def roles_for(k, variant):
    """role of each of k objects, in plan order: far and near mixed, the line objects not first"""
    on = (lambda L: ("at", L)) if variant == "at" else (lambda L: ("straddle", L))
    lo, hi = LINES
    first = [("above", lo), on(hi), ("near", 0), on(lo), ("above", hi)]
    more = [("above", hi), ("near", 0), ("above", lo)]
    assert k >= len(first), f"{k} objects cannot take the {len(first)} roles of a layout"
    return first + [more[i % len(more)] for i in range(k - len(first))]


def line_name(L):
    return {1 << 31: "2^31", 1 << 32: "2^32"}[L]


class Layout:
    """offsets: uint64 array; sizes; roles; windows: merged [start, end) the test sets and reads back (objects with their
    guards, and the alias windows); alias[i]: (start, end) of object i's alias window or None."""

    def __init__(self, kind, variant, sizes, roles, offsets):
        self.kind, self.variant, self.sizes, self.roles = kind, variant, [int(s) for s in sizes], roles
        self.offsets = np.array(offsets, np.uint64)
        self.total = BUFFER_BYTES
        self.spans = [(int(o), int(o) + s) for o, s in zip(offsets, self.sizes)]
        self.guarded = [(a - GUARD, b + GUARD) for a, b in self.spans]
        self.alias = [(max(a - WRAP, 0), b - WRAP) if b > WRAP else None for a, b in self.spans]
        self.windows = merge(self.guarded + [w for w in self.alias if w])

    def describe(self, i):
        role, L = self.roles[i]
        a, b = self.spans[i]
        where = "below 2^31" if role == "near" else f"{role} {line_name(L)}" if role != "straddle" else f"across {line_name(L)}"
        return f"[{a:#x}, {b:#x}) {where}"

    def window_bytes(self):
        return sum(b - a for a, b in self.windows)


def merge(spans):
    out = []
    for a, b in sorted(spans):
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


def layout(sizes, kind, variant):
    """kind "pictures": offsets are multiples of 16, and in every region every other one is no multiple of 256 (the
    contract of mi_rtj_plan_create is 16).  kind "packets": alignment 1; variant "header" puts the 12-byte header of the
    straddling packets across the line, "data" their data.  (Objects of one size at multiples of it, as DV frames and
    pictures are, need no layout: tests/test_gpu_dv_far_offsets.py asserts their arithmetic itself.)"""
    assert kind in ("pictures", "packets") and variant in variants(kind)
    roles = roles_for(len(sizes), variant)
    cursor = {("near", 0): NEAR_BASE, ("above", LINES[0]): LINES[0] + REGION_GAP, ("above", LINES[1]): LINES[1] + REGION_GAP}
    placed = {key: 0 for key in cursor}
    offsets = []
    for i, (s, (role, L)) in enumerate(zip(sizes, roles)):
        s = int(s)
        assert (14 if kind == "packets" else 64) <= s <= MAX_OBJECT, f"object {i} of {s} bytes"
        if role == "at":
            off = L
        elif role == "straddle":
            if kind == "pictures":
                off = (L - s // 2) // 16 * 16  # a multiple of 16 that is none of 256
                if off % 256 == 0:
                    off -= 16
            elif variant == "header":
                off = L - 5            # bytes 0 .. 4 of the header below the line, 5 .. 11 above
            else:
                off = L - 12 - (s - 12) // 2
            assert off < L < off + s
        else:
            cur = cursor[(role, L)] + GUARD
            if kind == "pictures":
                cur = (cur + 255) // 256 * 256
                if placed[(role, L)] % 2 == 0:
                    cur += 16 * (1 + (i % 15))
            else:
                cur += 1 + (7 * i) % 61  # packets start at arbitrary byte addresses
            off = cur
            cursor[(role, L)] = cur + s + GUARD
            placed[(role, L)] += 1
        offsets.append(off)
    return Layout(kind, variant, sizes, roles, offsets)


def near_layout(sizes, kind):
    """every object below 2^31, from byte GUARD of the buffer on: the near side of a placement whose other buffer is far
    (packets at arbitrary byte addresses, pictures as layout() aligns them)"""
    cur, offsets = 0, []
    for i, s in enumerate(sizes):
        cur += GUARD
        if kind == "pictures":
            cur = (cur + 255) // 256 * 256 + (16 * (1 + i % 15) if i % 2 else 0)
        else:
            cur += 1 + (7 * i) % 61
        offsets.append(cur)
        cur += int(s) + GUARD
    return Layout(kind, "near", sizes, [("near", 0)] * len(sizes), offsets)


def alternating_layout(sizes, kind="pictures"):
    """consecutive objects on alternating sides of 2^32 (even ones below 2^31, odd ones above 2^32): what a run of
    pictures needs for its copies to go from below to above and from above to below"""
    cursor = [NEAR_BASE, LINES[1] + REGION_GAP]
    offsets, roles = [], []
    for i, s in enumerate(sizes):
        side = i & 1
        cur = (cursor[side] + GUARD + 255) // 256 * 256 + (16 * (1 + i % 15) if (i >> 1) & 1 else 0)
        if kind == "packets":
            cur += 1 + (7 * i) % 13
        offsets.append(cur)
        cursor[side] = cur + int(s) + GUARD
        roles.append(("above", LINES[1]) if side else ("near", 0))
    return Layout(kind, "alternating", sizes, roles, offsets)


def check_layout(lay):
    """every rule of the module docstring that holds for one layout, asserted; returns the roles it has"""
    spans, n = lay.spans, len(lay.spans)
    assert all(0 <= a - GUARD and b + GUARD <= BUFFER_BYTES for a, b in spans), "an object or its guard leaves the buffer"
    order = sorted(range(n), key=lambda i: spans[i][0])
    for x, y in zip(order, order[1:]):
        assert spans[x][1] + 2 * GUARD <= spans[y][0], f"objects {x} and {y}: less than a guard on each side between them"
    for i, w in enumerate(lay.alias):
        assert (w is not None) == (spans[i][1] > WRAP)
        if w:
            assert 0 <= w[0] < w[1] <= BUFFER_BYTES and w[1] - w[0] == spans[i][1] - max(spans[i][0], WRAP)
            for j, (a, b) in enumerate(lay.guarded):
                assert w[1] <= a or b <= w[0], f"alias window of object {i} meets object {j} or its guard"
    if lay.kind == "pictures":
        assert all(a % 16 == 0 for a, _ in spans) and any(a % 256 for a, _ in spans)
    have = set()
    for (role, L), (a, b) in zip(lay.roles, spans):
        if role == "near":
            assert b + GUARD <= LINES[0]
        elif role == "at":
            assert a == L
        elif role == "above":
            assert a - GUARD > L
        else:
            assert a < L < b
            if lay.kind == "packets":
                assert (a < L < a + 12) if lay.variant == "header" else (a + 12 <= L < b)
        have.add((role, L) if role != "near" else "near")
    covered = sorted(merge(lay.windows))
    assert covered == lay.windows
    for a, b in lay.guarded + [w for w in lay.alias if w]:
        assert any(wa <= a and b <= wb for wa, wb in lay.windows)
    assert lay.window_bytes() < WINDOW_BUDGET
    return have


def required_roles(variant):
    on = "at" if variant == "at" else "straddle"
    return {"near"} | {(r, L) for L in LINES for r in (on, "above")}


# ------------------------------------------------------------------ windows on a device buffer
def fill_windows(dev, d_buf, lay, fill):
    """set every window of the layout to `fill` (a byte, or a function of the absolute offsets that returns bytes)"""
    for a, b in lay.windows:
        if callable(fill):
            dev.h2d(d_buf, fill(np.arange(a, b, dtype=np.uint64)), offset=a)
        else:
            dev.memset(d_buf, fill, b - a, offset=a)


def read_windows(dev, d_buf, lay):
    return [dev.d2h(d_buf, b - a, offset=a) for a, b in lay.windows]


def cut(lay, wins, span):
    """the bytes [span) out of the windows read back"""
    a, b = span
    for (wa, wb), data in zip(lay.windows, wins):
        if wa <= a and b <= wb:
            return data[a - wa:b - wa]
    raise AssertionError(f"[{a:#x}, {b:#x}) lies in no window")


def outside_objects(lay, wins, fill):
    """(absolute offset, value, count, in an alias window?) of the first byte outside every object that is not as it
    was filled, or None"""
    for (wa, wb), data in zip(lay.windows, wins):
        keep = np.ones(wb - wa, bool)
        for a, b in lay.spans:
            lo, hi = max(a, wa), min(b, wb)
            if lo < hi:
                keep[lo - wa:hi - wa] = False
        want = fill(np.arange(wa, wb, dtype=np.uint64)) if callable(fill) else fill
        bad = np.nonzero(keep & (data != want))[0]
        if bad.size:
            at = wa + int(bad[0])
            in_alias = any(w and w[0] <= at < w[1] for w in lay.alias)
            return at, int(data[bad[0]]), int(bad.size), in_alias
    return None


def alias_report(lay, wins, i, want, fill):
    """what the alias window of object i says when object i came back wrong: how many of its bytes are no longer the
    fill, and how many of them are the bytes the object should have had at the same place"""
    w = lay.alias[i]
    if not w:
        return f"object {i} {lay.describe(i)} has no alias window (it ends below 2^32)"
    got = cut(lay, wins, w)
    a = max(lay.spans[i][0], WRAP) - lay.spans[i][0]
    part = np.asarray(want)[a:a + got.size]
    f = fill(np.arange(w[0], w[1], dtype=np.uint64)) if callable(fill) else fill
    changed = got != f
    return (f"object {i} {lay.describe(i)}: its alias window [{w[0]:#x}, {w[1]:#x}) has {int(changed.sum())} bytes that are not "
            f"the fill, {int((changed & (got == part)).sum())} of them the bytes the object should have: "
            + ("a store through an offset narrowed to 32 bits" if changed.any() else "nothing was stored there"))
