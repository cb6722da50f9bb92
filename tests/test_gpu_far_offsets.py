"""Every RTjpeg device entry point with buffers that cross byte 2^31 and byte 2^32: batch plans in every form of the
transform and every index path, plans with runs in all three formats, the host's checks of far numbers, the encoder's
output and input side, the generators and the colour stage.

The kernels add 32-bit lane offsets to a 64-bit wave-uniform base (csrc/rtj_decode_kernels.h, "no 64-bit vector
arithmetic"); a base, a frame stride or a picture index narrowed to 32 bits passes every test whose buffers end below
4 GiB.  Here small objects lie on both sides of the two lines (tests/far_offsets.py places them and names the windows),
in buffers of 2^32 + 2^26 bytes of which only those windows are ever set, uploaded or read back.  An object above 2^32 has
an alias window 2^32 below it, inside the buffer: a store through a narrowed offset lands there, in bounds, and the
failure text says so.  Integer work throughout: byte-for-byte equality with the oracle or restatement the other tests of
each entry point use, no tolerance.

What cannot be placed: mi_rtj_encode_* lays packets out itself, at multiples of `align`, so with small pictures a
packet can start exactly at a line (align 2^30) or lie above it, never straddle it; pictures of one size at multiples
of it (the generators' and the encoder's input) straddle the lines and lie above them, never start at one.

Tests with buffers of their own (colour stage, encoder) come first and free them; the two shared buffers of the plan
tests are allocated at their first use and freed at the module's end, so that no more than about 12 GB is held at once."""
import numpy as np
import pytest

import far_offsets as FO
import launch_shapes as LS
import rtj420_enc as T420
import rtjfmt as F
import rtjfmt_enc as E
import rtjlib as R
import runlib as RL
import runlib_fmt as RF
import test_gpu_launch_shapes as GL
import test_gpu_parity as T
import test_gpu_rtjfmt_encode as GE
import test_gpu_spec_runs as SR
import test_gpu_verify_runs as VR
from pkg import P

pytestmark = pytest.mark.gpu

S = LS.Shapes()
ST_FILL = 0x11   # what the windows of the stream buffer hold outside the packets
GIB = 1 << 30


def position_fill(offsets):
    """a byte that depends on where it lies: a byte taken from a neighbour shows"""
    return ((offsets * np.uint64(131)) & np.uint64(255)).astype(np.uint8)


def report(*a):
    print("FAR-OFFSETS", *a, flush=True)


# =========================================================================== (g) colour stage
COLOUR = [("420", f) for f in range(5)] + [("422", 2)]


def colour_sizes(kind, fmt, w, h):
    bpp = R.RGB_BPP[fmt]
    fsz = w * h * 3 // 2 if kind == "420" else 2 * w * h
    return fsz, w * bpp + 32  # (planes of a picture, a row pitch with 32 bytes the kernel must leave alone)


def colour_run(dev, kind, fmt, w, h, n, d_in, in_stride, d_out, pitch, out_stride, planes):
    """n pictures at multiples of the strides, the output prefilled by position with a guard on both sides; returns
    nothing, asserts every picture and every guard"""
    fsz, _ = colour_sizes(kind, fmt, w, h)
    osz = pitch * h
    for i in range(n):
        dev.h2d(d_in, planes[i], offset=i * in_stride)
        a = max(i * out_stride - FO.GUARD, 0)
        dev.h2d(d_out, position_fill(np.arange(a, i * out_stride + osz + FO.GUARD, dtype=np.uint64)), offset=a)
    if kind == "420":
        dev.to_rgb(fmt, w, h, n, d_in, in_stride, d_out, pitch, out_stride)
    else:
        dev.to_rgb422(w, h, n, d_in, in_stride, d_out, pitch, out_stride)
    dev.sync()
    for i in range(n):
        a = max(i * out_stride - FO.GUARD, 0)
        got = dev.d2h(d_out, i * out_stride + osz + FO.GUARD - a, offset=a)
        want = position_fill(np.arange(a, a + got.size, dtype=np.uint64))
        pic = want[i * out_stride - a:i * out_stride - a + osz]
        if kind == "420":
            R.oracle_to_rgb(fmt, w, h, planes[i], pic, pitch)
        else:
            F.yuv422_to_rgb24(w, h, planes[i], pic, pitch)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (f"colour {kind} format {fmt}, {w}x{h}, picture {i} at input byte {i * in_stride:#x}, output byte "
                               f"{i * out_stride:#x}: {bad.size} bytes differ, first at output byte {a + int(bad[0]):#x} "
                               f"(byte {a + int(bad[0]) - i * out_stride} of the picture): got {int(got[bad[0]])} want {int(want[bad[0]])}")


@pytest.mark.parametrize("place", ["straddle", "at"])
def test_colour_stage_frame_strides_across_the_lines(place):
    """six 64x32 pictures a frame stride apart.  "straddle": in_frame_stride 2^30 - 512 and out_frame_stride 2^30 - 1024,
    so that picture 2 lies across 2^31 and picture 4 across 2^32 in the input and in the output; "at": both strides 2^30,
    pictures 2 and 4 start exactly at the lines.  Pictures 3 and 5 lie wholly above them, 0 and 1 below."""
    w, h, n = 64, 32, 6
    in_stride, out_stride = (GIB - 512, GIB - 1024) if place == "straddle" else (GIB, GIB)
    dev = P.MiRtj()
    biggest_in = max(colour_sizes(k, f, w, h)[0] for k, f in COLOUR)
    biggest_out = max(colour_sizes(k, f, w, h)[1] * h for k, f in COLOUR)
    d_in = dev.alloc((n - 1) * in_stride + biggest_in)
    d_out = dev.alloc((n - 1) * out_stride + biggest_out + FO.GUARD)
    try:
        for kind, fmt in COLOUR:
            fsz, pitch = colour_sizes(kind, fmt, w, h)
            osz = pitch * h
            for stride, size in ((in_stride, fsz), (out_stride, osz)):
                if place == "straddle":
                    assert 2 * stride < FO.LINES[0] < 2 * stride + size and 4 * stride < FO.LINES[1] < 4 * stride + size
                else:
                    assert 2 * stride == FO.LINES[0] and 4 * stride == FO.LINES[1]
                assert stride + size < FO.LINES[0] < 3 * stride and 3 * stride + size < FO.LINES[1] < 5 * stride
            rng = np.random.default_rng([fmt, kind == "422", place == "at"])
            planes = [rng.integers(0, 256, fsz, dtype=np.uint8) for _ in range(n)]
            colour_run(dev, kind, fmt, w, h, n, d_in, in_stride, d_out, pitch, out_stride, planes)
    finally:
        dev.free(d_in)
        dev.free(d_out)
        dev.close()


@pytest.mark.parametrize("kind,fmt", COLOUR, ids=[f"{k}-{f}" for k, f in COLOUR])
def test_colour_stage_second_trip_of_the_tile_loop(kind, fmt):
    """the grid is capped at 2,048 workgroups of 256 tiles: a picture of more than 524,288 tiles sends every thread round
    its loop a second time (near offsets, one picture)"""
    w, h = (8192, 1040) if kind == "420" else (4096, 1032)
    tiles = (w // 8) * (h // 2) if kind == "420" else (w // 8) * h
    assert 2048 * 256 < tiles < 2 * 2048 * 256
    fsz, pitch = colour_sizes(kind, fmt, w, h)
    dev = P.MiRtj()
    d_in, d_out = dev.alloc(fsz), dev.alloc(pitch * h + 2 * FO.GUARD)
    try:
        planes = [np.random.default_rng([fmt, w]).integers(0, 256, fsz, dtype=np.uint8)]
        # (the picture starts one guard into the output buffer: stride 0 is never multiplied, the base carries it)
        colour_run(dev, kind, fmt, w, h, 1, d_in, 0, d_out + FO.GUARD, pitch, 0, planes)
    finally:
        dev.free(d_in)
        dev.free(d_out)
        dev.close()


# =========================================================================== (f) generators and encoder, input side
@pytest.mark.parametrize("gen", ["synth", "synth_lcg"])
def test_generator_and_encoder_input_above_4_gib(gen):
    """1,400 pictures of 1920x1088 are 4.39 GB: picture 685 lies across 2^31, picture 1,370 across 2^32, the pictures
    behind it above.  Pictures read back must be the generator's numpy twin's, their packets the oracle encoder's."""
    w, h, Q, n = 1920, 1088, 255, 1400
    fsz = T.frame_bytes(w, h)
    assert 685 * fsz < FO.LINES[0] < 686 * fsz and 1370 * fsz < FO.LINES[1] < 1371 * fsz and n * fsz > FO.LINES[1]
    check = [684, 685, 686, 1369, 1370, 1371, 1372, 1373]
    dev = P.MiRtj()
    d_fr = dev.alloc(n * fsz)
    d_st = None
    try:
        twin = R.synth_frame if gen == "synth" else R.synth_frame_lcg
        (dev.synth if gen == "synth" else dev.synth_lcg)(w, h, 0, n, seed=99, amp=8, dptr=d_fr)
        dev.sync()
        want = T.pmap(lambda i: twin(w, h, i, seed=99, amp=8), check)
        for i, wp in zip(check, want):
            d = T.first_diff(dev.d2h(d_fr, fsz, offset=i * fsz), wp)
            assert d is None, f"{gen}: picture {i} at byte {i * fsz:#x} differs from its twin: (byte, got, want, count) = {d}"
        d_st, po, pl = dev.encode(w, h, Q, n, d_fr)
        dev.sync()
        pk = T.pmap(lambda wp: R.OracleEncoder(w, h, Q).encode(wp), want)
        for i, p in zip(check, pk):
            assert int(pl[i]) == p.size, (gen, i, int(pl[i]), p.size)
            d = T.first_diff(dev.d2h(d_st, p.size, offset=int(po[i])), p)
            assert d is None, f"{gen}: packet {i} (picture at byte {i * fsz:#x}) differs from the oracle encoder's: {d}"
        report(f"(f) {gen}: k_{gen}, k_encode_fmt<4:2:0> read pictures up to byte {n * fsz:#x}; stream ends at byte "
               f"{int(po[-1]) + int(pl[-1]):#x}")
    finally:
        dev.free(d_fr)
        if d_st:
            dev.free(d_st)
        dev.close()


# =========================================================================== (e) encoder, output side
ENC_FMTS = (F.FMT_420, F.FMT_422, F.FMT_GREY)


def far_decode_of_device_packets(dev, fmt, w, h, d_st, po, pl, pkts, d_out, runs, want):
    """the encoder's packets where it left them, through a plan into far pictures"""
    fsz = F.plane_bytes(fmt, w, h)
    for variant in FO.PICTURE_VARIANTS:
        lay = FO.layout([fsz] * len(pkts), "pictures", variant)
        FO.fill_windows(dev, d_out, lay, 0x5A)
        if runs:
            dev.h2d(d_out, np.zeros(fsz, np.uint8), offset=int(lay.offsets[0]))
        plan = dev.plan(np.stack([p[:12] for p in pkts]), po, pl, lay.offsets)
        if runs:
            plan.set_runs_fmt(runs)
        plan.decode(d_st, d_out)
        dev.sync()
        wins = FO.read_windows(dev, d_out, lay)
        plan.close()
        check_pictures(lay, wins, want, 0x5A, f"encoder chain format {fmt} {'stream' if runs else 'frames'} pictures {variant}")


@pytest.mark.parametrize("fmt", ENC_FMTS)
def test_encoder_packets_a_gib_apart_and_the_chain_into_far_pictures(fmt):
    """six 176x48 pictures encoded with align 2^30: packet i starts at i * 2^30 — packet 2 exactly at 2^31, packet 4 exactly
    at 2^32, packets 3 and 5 above the lines — then the same buffer and offsets go to a plan that decodes into far
    pictures: the chain the benchmark runs."""
    w, h, n, Q, align = 176, 48, 6, 200, GIB
    dev = P.MiRtj()
    dev.set_format(fmt)
    bound = dev.encode_bound(w, h, n, align, fmt=fmt)
    assert bound >= (n - 1) * align + 12 + 64 * F.nblocks(fmt, w, h)
    d_st, d_out = dev.alloc(bound), dev.alloc(FO.BUFFER_BYTES)
    try:
        for key in (0, 3):
            if key:
                pics = T420.inter_pictures(w, h, seed=5)[:n] if fmt == F.FMT_420 else GE.inter_pictures(fmt, w, h, seed=5)
                want = (T420.oracle_packets(w, h, Q, pics, key, 2, 2) if fmt == F.FMT_420
                        else E.encode_all(fmt, w, h, Q, pics, key, 2, 2))
            else:
                pics = [F.make_picture(fmt, w, h, i, seed=7, amp=(0, 8, 64)[i % 3]) for i in range(n)]
                want = T420.oracle_packets(w, h, Q, pics) if fmt == F.FMT_420 else E.encode_all(fmt, w, h, Q, pics)
            room = max(p.size for p in want) + FO.GUARD
            for i in range(n):  # a guard in front of every packet and room for it behind
                a = max(i * align - FO.GUARD, 0)
                dev.memset(d_st, GE.PREFILL, i * align + room - a, offset=a)
            d_fr = GE.upload(dev, pics)
            _, po, pl = dev.encode(w, h, Q, n, d_fr, align=align, key_rate=key, lmask=2, cmask=2, d_stream=d_st, fmt=fmt)
            dev.sync()
            dev.free(d_fr)
            assert [int(x) for x in po] == [i * align for i in range(n)], (fmt, key, po)
            assert int(po[2]) == FO.LINES[0] and int(po[4]) == FO.LINES[1]
            pkts = [dev.d2h(d_st, int(pl[i]), offset=int(po[i])) for i in range(n)]
            GE.assert_stream_equals((fmt, key, "align 2^30"), want, pkts, po, pl, align)
            for i in range(n):
                a = max(i * align - FO.GUARD, 0)
                front = dev.d2h(d_st, i * align - a, offset=a)
                behind = dev.d2h(d_st, room - pkts[i].size, offset=i * align + pkts[i].size)
                assert np.all(front == GE.PREFILL) and np.all(behind == GE.PREFILL), \
                    f"format {fmt} key rate {key}: bytes around packet {i} at {i * align:#x} were written"
            # back through a plan of the format, from where the encoder left them
            if fmt == F.FMT_420:
                back = RL.oracle_in_order(pkts, [n] if key else [1] * n,
                                          [np.zeros(F.plane_bytes(fmt, w, h), np.uint8)] if key else
                                          [np.full(F.plane_bytes(fmt, w, h), 0x5A, np.uint8)] * n)
            else:
                back = RF.in_order(fmt, pkts, [n], [np.zeros(F.plane_bytes(fmt, w, h), np.uint8)]) if key else \
                    RF.independent(fmt, pkts, [np.full(F.plane_bytes(fmt, w, h), 0x5A, np.uint8)] * n, [1] * n, fill=0x5A)
            far_decode_of_device_packets(dev, fmt, w, h, d_st, po, pl, pkts, d_out, [n] if key else None, back)
            report(f"(e) format {fmt} key rate {key}: k_encode_pack wrote packets at {[hex(int(x)) for x in po]}")
    finally:
        dev.free(d_st)
        dev.free(d_out)
        dev.close()


# =========================================================================== the shared far buffers of the plan tests
class Far:
    def __init__(self):
        self.devs = {}
        self.dev = self.of(F.FMT_420)
        # an allocation failure raises MiRtjError: the tests that need the buffers fail, they do not skip
        self.d_st = self.dev.alloc(FO.BUFFER_BYTES)
        self.d_out = self.dev.alloc(FO.BUFFER_BYTES)

    def of(self, fmt):
        if fmt not in self.devs:
            self.devs[fmt] = P.MiRtj()
            if fmt != F.FMT_420:
                self.devs[fmt].set_format(fmt)
        return self.devs[fmt]

    def close(self):
        self.dev.free(self.d_st)
        self.dev.free(self.d_out)
        for d in self.devs.values():
            d.close()


@pytest.fixture(scope="module")
def far():
    f = Far()
    yield f
    f.close()


def stream_alias_verdict(st_lay, i, pkt, got, prefill, fmt):
    """if picture i is what the fill of the stream buffer's alias window decodes to, say so: the signature of a packet
    offset narrowed to 32 bits"""
    a, b = st_lay.spans[i]
    if a + 12 < FO.WRAP:
        return f"packet {i} {st_lay.describe(i)}: its data starts below 2^32, no alias window of the stream buffer to read from"
    w = st_lay.alias[i]
    fake = np.concatenate([pkt[:12], np.full(pkt.size - 12, ST_FILL, np.uint8)])
    alt = np.full(got.size, prefill, np.uint8)
    if fmt == F.FMT_420:
        R.OracleDecoder().decode(fake, alt)
    else:
        F.Restated(fmt).decode(fake, alt)
    same = np.array_equal(alt, got)
    return (f"packet {i} {st_lay.describe(i)}: the picture is {'exactly' if same else 'not'} what the fill of the stream "
            f"buffer's alias window [{w[0]:#x}, {w[1]:#x}) decodes to"
            + (": a load through a packet offset narrowed to 32 bits" if same else ""))


def check_pictures(lay, wins, wants, fill, what, explain=None):
    """every picture of the layout against `wants`, then every byte of every window outside the pictures against the
    fill.  explain(i, got, want): more text for the first wrong picture."""
    for i, want in enumerate(wants):
        got = FO.cut(lay, wins, lay.spans[i])
        if np.array_equal(got, want):
            continue
        d = np.nonzero(got != want)[0]
        text = (f"{what}: picture {i} {lay.describe(i)}: {d.size} bytes differ, first at byte {int(d[0])}: got {int(got[d[0]])} "
                f"want {int(want[d[0]])}; alias window of the output buffer: {FO.alias_report(lay, wins, i, want, fill)}")
        if explain:
            text += "; " + explain(i, got, want)
        raise AssertionError(text)
    bad = FO.outside_objects(lay, wins, fill)
    assert bad is None, (f"{what}: byte {bad[0]:#x} of the output buffer, outside every picture, was written: {bad[1]} "
                         f"({bad[2]} such bytes in its window); it lies in "
                         + ("an alias window: a store through an offset narrowed to 32 bits" if bad[3] else "a guard"))


def far_plan_decode(far, fmt, pkts, st_lay, out_lay, prefill, wants, what, env=None, monkeypatch=None, runs=None, prev=None,
                    expect_form=None, want_index=None, shapes=None):
    """One plan over packets at st_lay's places into pictures at out_lay's; returns what the plan says about the launch.
    Pictures, guards, alias windows and the block index are held to `wants` / `want_index`."""
    dev = far.of(fmt)
    FO.fill_windows(dev, far.d_st, st_lay, ST_FILL)
    for p, o in zip(pkts, st_lay.offsets):
        dev.h2d(far.d_st, p, offset=int(o))
    FO.fill_windows(dev, far.d_out, out_lay, prefill)
    if runs:
        i = 0
        for r, m in enumerate(runs):
            dev.h2d(far.d_out, prev[r], offset=int(out_lay.offsets[i]))
            i += m
    dev.sync()
    hdrs = np.zeros((len(pkts), 12), np.uint8)
    for i, p in enumerate(pkts):
        hdrs[i, :min(12, p.size)] = p[:12]
    pl = np.array([p.size for p in pkts], np.uint32)
    with monkeypatch.context() as m:
        for k in ("MI_RTJ_ROTATE", "MI_RTJ_SPLIT", "MI_RTJ_DEC_SLOTS", "MI_RTJ_INDEX", "MI_RTJ_EMIT", "MI_RTJ_SPEC",
                  "MI_RTJ_SPEC_RUN", "MI_RTJ_SERIAL_MIN", "MI_RTJ_OVERLAP"):
            m.delenv(k, raising=False)
        for k, v in (env or {}).items():
            m.setenv(k, v)
        plan = dev.plan(hdrs, st_lay.offsets, pl, out_lay.offsets)
    if runs:
        (plan.set_runs if fmt == F.FMT_420 else plan.set_runs_fmt)(runs)
    plan.decode(far.d_st, far.d_out)
    dev.sync()
    rep = dict(form=plan.decode_form()[0], listed=plan.decode_form()[2], copied=plan.run_copied())
    rep["proven"], rep["chunks"] = plan.spec_stats()
    rep["repaired"] = plan.repaired
    idx = plan.read_index()
    plan.close()
    wins = FO.read_windows(dev, far.d_out, out_lay)
    if expect_form is not None:
        assert rep["form"] == expect_form, f"{what}: the plan ran form {rep['form']}, not {expect_form}"

    def explain(i, got, want):
        text = stream_alias_verdict(st_lay, i, pkts[i], got, prefill, fmt) if not runs else f"packet {i} {st_lay.describe(i)}"
        if shapes and not runs:
            w, h = T.packet_size(pkts[i])
            off = int(np.nonzero(got != want)[0][0])
            text += "; " + S.describe_byte(w, h, off, shapes, frame=i, frames=len(pkts))
        return text

    check_pictures(out_lay, wins, wants, prefill, what, explain)
    k = 0
    for i, p in enumerate(pkts):
        wi = want_index[i]
        gi = idx[k:k + wi.size].astype(np.int64)
        k += wi.size
        bad = np.nonzero(gi != wi)[0]
        assert bad.size == 0, (f"{what}: block index of packet {i} {st_lay.describe(i)}: first mismatch at block {bad[0]}: "
                               f"got {gi[bad[0]]} want {wi[bad[0]]} ({bad.size} wrong of {wi.size})")
    st_bad = FO.outside_objects(st_lay, FO.read_windows(dev, far.d_st, st_lay), ST_FILL)
    assert st_bad is None, f"{what}: byte {st_bad[0]:#x} of the stream buffer was written"
    return rep


def placements(pkts, sizes):
    """(name, stream layout, output layout) of the three placements in every variant: packets near and pictures far,
    packets far and pictures near, both far"""
    plen = [p.size for p in pkts]
    out = []
    for v in FO.PICTURE_VARIANTS:
        out.append(("packets-near-pictures-far", FO.near_layout(plen, "packets"), FO.layout(sizes, "pictures", v)))
    for v in FO.PACKET_VARIANTS:
        out.append(("packets-far-pictures-near", FO.layout(plen, "packets", v), FO.near_layout(sizes, "pictures")))
    for k, v in enumerate(FO.PACKET_VARIANTS):
        out.append(("both-far", FO.layout(plen, "packets", v), FO.layout(sizes, "pictures", FO.PICTURE_VARIANTS[k % 2])))
    return out


def index_420(pkts):
    dec = R.OracleDecoder()
    return [dec.block_offsets(p).astype(np.int64) - 12 for p in pkts]


# --------------------------------------------------------------------------- (a) every form of the transform
def far_geometries():
    """one picture size with fewer macroblocks per row than a group has, one with at least as many: the two arms of the
    split form's luma block offset (decode_wave<kSuper>, csrc/rtj_decode_kernels.h).  Both from the launch-shape sweep."""
    narrow = max(((n, w, h) for n, w, h in GL.CLASSES if 2 <= w // 16 < S.kMbPerGroup and h > 16), key=lambda c: S.groups(c[1], c[2]))
    wide = next((n, w, h) for n, w, h in GL.CLASSES if n == "640x368")
    assert narrow[1] // 16 < S.kMbPerGroup <= wide[1] // 16
    return [narrow, wide]


GEOMETRIES = far_geometries()
PLACEMENTS = ("packets-near-pictures-far", "packets-far-pictures-near", "both-far")
_made = {}


def packets_and_wants(w, h):
    if (w, h) not in _made:
        pkts = GL.make_packets(w, h)
        _made[(w, h)] = (pkts, {f: GL.oracle_pictures(pkts, f) for f in GL.PREFILLS}, index_420(pkts))
    return _made[(w, h)]


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("cls,w,h", GEOMETRIES, ids=[f"{w}x{h}" for _, w, h in GEOMETRIES])
def test_every_form_of_the_transform_at_far_offsets(far, monkeypatch, cls, w, h, placement):
    pkts, wants, want_index = packets_and_wants(w, h)
    sizes = [T.frame_bytes(w, h)] * len(pkts)
    groups = S.groups(w, h)
    seen = set()
    for name, st_lay, out_lay in placements(pkts, sizes):
        if name != placement:
            continue
        for form, (env, expect) in GL.forms(groups).items():
            for prefill in GL.PREFILLS:
                what = (f"{w}x{h} ({groups} groups), {name} (packets {st_lay.variant}, pictures {out_lay.variant}), form {form}, "
                        f"prefill {prefill:#04x}")
                model = "split" if form.startswith("split") else "classic" if form.startswith("classic") else "span1"
                rep = far_plan_decode(far, F.FMT_420, pkts, st_lay, out_lay, prefill, wants[prefill], what, env, monkeypatch,
                                      expect_form=expect, want_index=want_index, shapes=model)
                seen.add((form, rep["form"], rep["listed"] > 0, rep["proven"] > 0))
    report(f"(a) {w}x{h} {placement}: (form, decode_form, k_decode_list had parts, speculative index proved packets) = {sorted(seen)}")


# --------------------------------------------------------------------------- (b) the index paths
INDEX_PATHS = [("serial", dict(MI_RTJ_INDEX="serial")), ("emit-walk", dict(MI_RTJ_EMIT="walk")),
               ("spec0", dict(MI_RTJ_SPEC="0")), ("spec1", dict(MI_RTJ_SPEC="1")), ("spec3", dict(MI_RTJ_SPEC="3")),
               ("spec4", dict(MI_RTJ_SPEC="4")), ("spec1-run1", dict(MI_RTJ_SPEC="1", MI_RTJ_SPEC_RUN="1")),
               ("spec1-run4", dict(MI_RTJ_SPEC="1", MI_RTJ_SPEC_RUN="4")),
               ("spec1-serial-min-1", dict(MI_RTJ_SPEC="1", MI_RTJ_SERIAL_MIN="1"))]
REPAIRS = ("spec1", "spec1-run1", "spec1-run4")  # the short lead, no policy: the noisy packets need repairs


def repair_packets():
    """640x368: the noisy packets of tests/test_gpu_spec_runs.py, which tests/test_gpu_verify_runs.py repairs at every
    run length, its zero-padded packets (last runs of every length at S = 4), and two packets that mix coded and
    unchanged blocks: walkers inside one-byte blocks keep the phase they assumed, such packets are refused by the
    proof and make up the to-do list of the exact kernels"""
    if "repair" not in _made:
        enc = R.OracleEncoder(640, 368, 200, 6, 3, 3)
        pics = [R.synth_frame(640, 368, 0, seed=9, amp=2) for _ in range(3)]
        k = pics[0].size // 3  # a new top third over an unchanged rest
        pics[1][:k] = 255 - pics[0][:k]
        pics[2][:k] = R.synth_frame(640, 368, 40, seed=9, amp=8)[:k]
        mixed = [enc.encode(p) for p in pics][1:]
        assert all((p[12:] == 255).any() and not (p[12:] == 255).all() for p in mixed)
        pkts = list(SR.noisy_packets()) + VR.last_run_cases(640, 368, 255, 4) + mixed
        pre = 0x3C
        _made["repair"] = (pkts, [SR.wanted(p, pre)[0] for p in pkts], index_420(pkts), pre)
    return _made["repair"]


@pytest.mark.parametrize("path,env", INDEX_PATHS, ids=[p for p, _ in INDEX_PATHS])
def test_every_index_path_at_far_offsets(far, monkeypatch, path, env):
    pkts, wants, want_index, prefill = repair_packets()
    sizes = [T.frame_bytes(640, 368)] * len(pkts)
    for name, st_lay, out_lay in placements(pkts, sizes):
        if name != "both-far":
            continue
        what = f"index path {path}, both far (packets {st_lay.variant}, pictures {out_lay.variant})"
        rep = far_plan_decode(far, F.FMT_420, pkts, st_lay, out_lay, prefill, wants, what, env, monkeypatch,
                              want_index=want_index, shapes="split")
        report(f"(b) {path} packets {st_lay.variant}: form {rep['form']}, proven {rep['proven']} of {len(pkts)}, chunks "
               f"{rep['chunks']}, repaired {rep['repaired']}")
        if path in REPAIRS:
            assert rep["repaired"] >= 1, f"{what}: k_spec_repair did not run"
        if path == "spec1-serial-min-1":  # a packet the proof refuses: the to-do list is not empty, the serial walker takes it
            assert 0 < rep["proven"] < len(pkts), (what, rep)


# --------------------------------------------------------------------------- (c) runs of unchanged blocks
RUN_CASES = [(F.FMT_420, 176, 48), (F.FMT_422, 48, 24), (F.FMT_GREY, 24, 8)]


def run_layouts(plen, sizes):
    """consecutive pictures on alternating sides of 2^32 (the run kernels copy below -> above and above -> below), then
    the line placements in every variant"""
    out = [("alternating", FO.alternating_layout(plen, "packets"), FO.alternating_layout(sizes))]
    for k, v in enumerate(FO.PACKET_VARIANTS):
        out.append((f"lines-{v}", FO.layout(plen, "packets", v), FO.layout(sizes, "pictures", FO.PICTURE_VARIANTS[k % 2])))
    return out


@pytest.mark.parametrize("fmt,w,h", RUN_CASES, ids=["420", "422", "grey"])
def test_runs_copy_across_the_lines(far, monkeypatch, fmt, w, h):
    """twelve packets of one inter stream (key rate 3, masks 2 / 2) as one run"""
    n, Q = 12, 200
    if fmt == F.FMT_420:
        pkts = T420.oracle_packets(w, h, Q, T420.inter_pictures(w, h, seed=4), 3, 2, 2)
        prev = [np.random.default_rng(4).integers(0, 256, T.frame_bytes(w, h), dtype=np.uint8)]
        wants = RL.oracle_in_order(pkts, [n], prev)
        want_index = index_420(pkts)
        copied = sum(int((~RL.coded_blocks(o + 12)).sum()) for o in want_index[1:])
    else:
        pkts = F.make_packets(fmt, w, h, Q, n, seed=3, key_rate=3, lmask=2, cmask=2)
        assert RF.has_both_kinds(fmt, pkts, [n])
        prev = [RF.rand_pic(fmt, w, h, 4)]
        wants = RF.in_order(fmt, pkts, [n], prev)
        copied = RF.by_rule(fmt, pkts, [n], prev)[1]
        want_index = [E.block_offsets(fmt, p) for p in pkts]
    assert len(pkts) == n and copied > 0
    sizes = [F.plane_bytes(fmt, w, h)] * n
    for name, st_lay, out_lay in run_layouts([p.size for p in pkts], sizes):
        if name == "alternating":
            sides = [int(o) > FO.WRAP for o in out_lay.offsets]
            assert sides == [bool(i & 1) for i in range(n)]
        what = f"run of {n}, format {fmt}, {w}x{h}, layout {name}"
        rep = far_plan_decode(far, fmt, pkts, st_lay, out_lay, RF.FILL, wants, what, None, monkeypatch, runs=[n], prev=prev,
                              want_index=want_index)
        assert rep["copied"] == copied, (what, rep["copied"], copied)
        report(f"(c) format {fmt} {name}: run kernels copied {rep['copied']} blocks, form {rep['form']}")


# --------------------------------------------------------------------------- (d) the host's checks with far numbers
def test_host_checks_with_far_numbers(far, monkeypatch):
    dev = far.dev
    w, h, Q = 64, 48, 90
    fsz = T.frame_bytes(w, h)
    pkts = RL.stream_packets(w, h, Q, 2, 4, 2, 2, seed=2)
    prev = [np.random.default_rng(1).integers(0, 256, fsz, dtype=np.uint8)]
    wants = RL.oracle_in_order(pkts, [2], prev)
    st_lay = FO.near_layout([p.size for p in pkts], "packets")
    x = (1 << 24) + 16
    # two pictures of a run exactly 2^32 apart: each lies in the other's alias window, and they do not overlap
    apart = FO.Layout("pictures", "2^32 apart", [fsz, fsz], [("near", 0), ("above", FO.LINES[1])], [x, x + FO.WRAP])
    assert int(apart.offsets[1]) - int(apart.offsets[0]) == FO.WRAP and int(apart.offsets[1]) + fsz + FO.GUARD <= FO.BUFFER_BYTES
    dev.memset(far.d_out, RF.FILL, fsz + 2 * FO.GUARD, offset=x - FO.GUARD)
    dev.memset(far.d_out, RF.FILL, fsz + 2 * FO.GUARD, offset=x + FO.WRAP - FO.GUARD)
    dev.h2d(far.d_out, prev[0], offset=x)
    for p, o in zip(pkts, st_lay.offsets):
        dev.h2d(far.d_st, p, offset=int(o))
    hdrs = np.stack([p[:12] for p in pkts])
    pl = np.array([p.size for p in pkts], np.uint32)
    plan = dev.plan(hdrs, st_lay.offsets, pl, apart.offsets)
    plan.set_runs([2])
    plan.decode(far.d_st, far.d_out)
    dev.sync()
    for i in range(2):
        got = dev.d2h(far.d_out, fsz + 2 * FO.GUARD, offset=int(apart.offsets[i]) - FO.GUARD)
        assert T.first_diff(got[FO.GUARD:-FO.GUARD], wants[i]) is None, (i, T.first_diff(got[FO.GUARD:-FO.GUARD], wants[i]))
        assert np.all(got[:FO.GUARD] == RF.FILL) and np.all(got[-FO.GUARD:] == RF.FILL), i
    # two that overlap by 16 bytes above 2^32
    over = np.array([FO.WRAP + x, FO.WRAP + x + fsz - 16], np.uint64)
    bad = dev.plan(hdrs, st_lay.offsets, pl, over)
    with pytest.raises(P.MiRtjError, match="overlap"):
        bad.set_runs([2])
    bad.close()
    # an out_offset above 2^32 that is no multiple of 16
    with pytest.raises(P.MiRtjError, match="multiple of 16"):
        dev.plan(hdrs, st_lay.offsets, pl, np.array([x, FO.WRAP + 8], np.uint64))
    # ... and the plan made before still decodes
    dev.memset(far.d_out, RF.FILL, fsz, offset=x + FO.WRAP)
    dev.h2d(far.d_out, prev[0], offset=x)
    plan.decode(far.d_st, far.d_out)
    dev.sync()
    for i in range(2):
        assert T.first_diff(dev.d2h(far.d_out, fsz, offset=int(apart.offsets[i])), wants[i]) is None, i
    plan.close()
