"""mi_rgb_unpack_batch with packets and pictures above byte 2^31 and byte 2^32 of their buffers, against the statement
(tests/rgbraw.py), byte for byte.

All kernels find packet i and picture i as a 64-bit wave-uniform base, `blockIdx.y * stride`, plus a 32-bit lane offset;
a base narrowed to 32 bits, or an index multiplied in 32 bits, passes every test of a few small frames.  One codec of each
kernel kind runs over buffers of far_offsets.BUFFER_BYTES: AVI24 at 64 x 16 (k_rgb_move: padded rows in reverse; packets
and pictures of 3,072 bytes), QT32 at 48 x 16 (k_rgb_move with a byte permute; 3,072 and 3,072) and QT1 at 264 x 32
(k_rgb_palette: three chunks, rows that end inside a lane's 16 pixels, the palette index of a slot read at blockIdx.y;
packets of 1,088 and pictures of 25,344 bytes).

Slots of one stride S from one base cannot both start at a line L and lie across it, so a launch comes in two VARIANTS,
and each buffer has a stride and a base of its own for each:

  "at-straddle"   2^31 mod S = r, base r: slot 2^31 // S starts at 2^31, slot 2 (2^31 // S) starts r below 2^32
  "straddle-at"   2^31 mod S = S - r, base S - 2r: slot 2^31 // S starts r below 2^31, slot 2^32 // S starts at 2^32

with (size + guard) / 2 <= r < size: the slot r below a line lies across it, and the ALIAS window of a slot above 2^32
(2^32 below it: where a store or a load through an address narrowed to 32 bits lands) falls between two slots near the
buffer's start, a guard away from both, on bytes no slot of the launch owns.  The strides are a little above 2^16, so that about 65,400 slots reach past 2^32.
Only the windows of the slots around the lines, of the first and the last slot, and the alias windows are set and read
back (far_offsets.WINDOW_BUDGET a buffer); the other slots unpack whatever the memory holds and are not judged.  The
alias windows of the pictures must keep their fill; those of the packets hold other bytes than the packets."""
import importlib

import numpy as np
import pytest

import far_offsets as FO
import rgbraw as R

pytestmark = pytest.mark.gpu

LO, HI = FO.LINES
GUARD, FILL = FO.GUARD, 0xA5
CASES = (("AVI24", 64, 16), ("QT32", 48, 16), ("QT1", 264, 32))
VARIANTS = ("at-straddle", "straddle-at")


def placements(size, variant):
    """every (stride, base) of a buffer's slots for the variant with a stride from 65,792 to 98,560, a multiple of 16, the
    residue the module docstring asks for and a base that is no multiple of 256"""
    out = []
    for S in range(65792, 65792 + (1 << 15), 16):
        r = LO % S if variant == "at-straddle" else S - LO % S
        base = r if variant == "at-straddle" else S - 2 * r
        if size + GUARD <= 2 * r and r < size and base % 256 and base >= GUARD:
            out.append((S, base))
    return out


def role_of(a, b):
    for L in (HI, LO):
        if a == L:
            return ("at", L)
        if a < L < b:
            return ("straddle", L)
        if a > L:
            return ("above", L)
    return ("near", 0)


class Plan:
    """one launch: strides, bases and n, the judged slots, and each buffer's far_offsets.Layout over them"""

    def __init__(self, codec, w, h, variant):
        lay = R.layout(codec, w, h)
        self.sizes = (lay.packet_bytes, lay.picture_bytes)
        # two different strides as close to each other as there are: both buffers reach past 2^32 with one n
        self.place = min(((p, q) for p in placements(self.sizes[0], variant) for q in placements(self.sizes[1], variant) if p[0] != q[0]),
                         key=lambda pq: (abs(pq[0][0] - pq[1][0]), pq))
        self.n = max(HI // S for S, _ in self.place) + 4
        judged = {0, self.n - 1}
        for S, base in self.place:
            for L in FO.LINES:
                k = (L - base) // S
                judged |= {k - 1, k, k + 1}
        self.judged = sorted(judged)
        self.layouts = []
        for (S, base), size in zip(self.place, self.sizes):
            offsets = [base + k * S for k in self.judged]
            self.layouts.append(FO.Layout("pictures", variant, [size] * len(offsets), [role_of(o, o + size) for o in offsets], offsets))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("codec,w,h", CASES, ids=[c for c, _, _ in CASES])
def test_the_arithmetic_of_the_layout(codec, w, h, variant):
    p = Plan(codec, w, h, variant)
    assert 1 <= p.n <= 65535
    on_lo, on_hi = ("at", "straddle") if variant == "at-straddle" else ("straddle", "at")
    for (S, base), size, lay in zip(p.place, p.sizes, p.layouts):
        assert S % 16 == 0 and base % 16 == 0 and S >= size and base + (p.n - 1) * S + size + GUARD <= FO.BUFFER_BYTES
        have = FO.check_layout(lay)
        assert {"near", (on_lo, LO), ("above", LO), (on_hi, HI), ("above", HI)} <= have, have
        aliases = [x for x in lay.alias if x]
        assert len(aliases) >= 3
        for a, b in aliases:  # no slot of the launch, judged or not, owns a byte of an alias window
            first = max((a - base) // S, 0)
            assert all(b <= base + k * S or base + k * S + size <= a for k in (first, first + 1)), (a, b)
    assert (R.layout("AVI24", 64, 16).packet_bytes, R.layout("AVI24", 64, 16).picture_bytes) == (3072, 3072)
    assert (R.layout("QT32", 48, 16).packet_bytes, R.layout("QT32", 48, 16).picture_bytes) == (3072, 3072)
    assert (R.layout("QT1", 264, 32).packet_bytes, R.layout("QT1", 264, 32).picture_bytes) == (1088, 25344)
    assert 264 * 32 > 2 * 4096 and 264 % 16  # more than one chunk of the palette kernel; rows end inside a lane's 16 pixels


@pytest.fixture(scope="module")
def far():
    rgb = importlib.import_module("gmerlin-avdecoder_amd.rgb")
    dev = rgb.MiRgb(0)
    d_packets, d_pics = dev.alloc(FO.BUFFER_BYTES), dev.alloc(FO.BUFFER_BYTES)
    yield dev, d_packets, d_pics
    dev.free(d_packets)
    dev.free(d_pics)
    dev.close()


def noise(offsets):
    """bytes that depend on where they lie: what an alias window of the packets holds differs from the packet above it"""
    return ((offsets * np.uint64(2654435761)) >> np.uint64(13)).astype(np.uint8)


def fill(offsets):
    return np.full(offsets.size, FILL, np.uint8)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("codec,w,h", CASES, ids=[c for c, _, _ in CASES])
def test_unpack_batch_slots_across_at_and_above_the_lines(far, codec, w, h, variant):
    dev, d_packets, d_pics = far
    p = Plan(codec, w, h, variant)
    (ps, pbase), (qs, qbase) = p.place
    lay_p, lay_q = p.layouts
    rng = np.random.default_rng(31 + VARIANTS.index(variant))
    packets = [R.random_packet(codec, w, h, rng) for _ in p.judged]
    # palettised: two palettes, and the slots alternate between them: a slot's index is read at blockIdx.y, far up too
    palettes = palette_of = None
    if R.layout(codec, w, h).palette_entries:
        palettes = np.stack([R.random_palette(codec, rng) for _ in range(2)])
        palette_of = (np.arange(p.n) % 2).astype(np.uint16)
    FO.fill_windows(dev, d_packets, lay_p, noise)
    for (a, _), packet in zip(lay_p.spans, packets):
        dev.h2d(d_packets, packet, offset=a)
    before = FO.read_windows(dev, d_packets, lay_p)
    FO.fill_windows(dev, d_pics, lay_q, fill)
    dev.times()
    dev.unpack_batch(codec, w, h, d_packets + pbase, ps, p.n, d_pics + qbase, qs, palettes, palette_of)
    dev.sync()
    assert dev.times()[1] == 1
    wins = FO.read_windows(dev, d_pics, lay_q)
    for i, (k, packet) in enumerate(zip(p.judged, packets)):
        got = FO.cut(lay_q, wins, lay_q.spans[i])
        want = R.unpack(codec, w, h, packet, None if palettes is None else palettes[k % 2])
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{codec} slot {k}: packet {lay_p.describe(i)}, picture {lay_q.describe(i)}: {bad.size} bytes differ "
                                 f"from the statement's, first at byte {int(bad[0])}; " + FO.alias_report(lay_q, wins, i, want, fill))
    stray = FO.outside_objects(lay_q, wins, fill)
    assert stray is None, f"byte {stray[0]:#x} outside every judged picture is {stray[1]:#x} ({stray[2]} such bytes; in an alias window: {stray[3]})"
    after = FO.read_windows(dev, d_packets, lay_p)
    assert all(np.array_equal(x, y) for x, y in zip(before, after)), "the packets were written"
    print("FAR-OFFSETS RGB", codec, variant, f"1 launch over {p.n} slots: packets at stride {ps} from {pbase}, pictures at stride {qs} "
          f"from {qbase}; judged slots {p.judged}", flush=True)
