"""What a pooling chroma wave of k_decode_split decides for one round of three macroblock groups, restated from
csrc/rtj_decode_chroma.h (chroma_pool_wave), and directed packets that reach every one of those decisions.

The model works on the oracle's block offsets and the packet's bytes alone.  Per group of a round it restates which
lanes have a block (`valid`), whether the group is left to k_decode_list before anything is parsed (`gslow`: a block
longer than eight bytes, or one that does not end inside the packet), the class of every block (none / unchanged / DC
only / busy) and the busy count; per round the partition of the groups into pools of at most 64 busy blocks, which
pools bail (a busy block with a dequantised coefficient outside rows 0-3 x columns 0-3), which of the three forms of
the short transform a pool runs, how many groups the round stores (the arm of the counted wait) and which chroma parts
go to the list.  kPoolGroups, kMbPerGroup, kXcds and the wave and round of a super group come from
launch_shapes.Shapes; the budget of the three-input packed form from csrc/rtj_idct_pk.h (edge_packets.Budget).

pool_packets() builds 4:2:0 packets whose luma blocks are all DC only, so that no luma part is ever listed and
`parts_listed` of a split launch is the model's count exactly; tests/test_pool_model_cpu.py holds the packets to the
scenarios they are built for, tests/test_gpu_split_edges.py decodes them."""
import numpy as np

import edge_packets as E
import launch_shapes as LS
import rtjlib as R

NONE, UNCHANGED, DC_ONLY, BUSY = 0, 1, 2, 3
SHORT_MAX = 8    # bytes of a block the short forms take (`len > 8u`)
POOL_LANES = 64  # busy blocks a pool holds (`tot + cnt[q] <= 64u`)
_LOW4 = np.array([(n >> 3) < 4 and (n & 7) < 4 for n in range(64)])   # natural order
_LOW3 = np.array([(n >> 3) < 3 and (n & 7) < 3 for n in range(64)])


def int16(v):
    return ((int(v) + 32768) % 65536) - 32768


def dc_pixel(b0, q0):
    """the 64 pixels of a DC-only block: clamp16_235(int16((int16(DC * q0) + 4) >> 3))"""
    s = int16((int16(b0 * q0) + 4) >> 3)
    return 235 if s > 235 else 16 if s < 16 else s


def short_coefficients(blk, ciqt):
    """dequantised coefficients (natural order, int16) of a chroma block of at most eight bytes, cb8 == 0: DC, then tokens"""
    c = np.zeros(64, np.int64)
    c[0] = int16(int(blk[0]) * int(ciqt[0]))
    co = 1
    for v in blk[1:]:
        s = int(v) - 256 if v > 127 else int(v)
        if s > 63:
            co = min(64, co + s - 63)
        else:
            c[E.ZZ[co]] = int16(s * int(ciqt[E.ZZ[co]]))
            co += 1
        if co >= 64:
            break
    return c


class Group:
    pass


class Pool:
    pass


class Round:
    pass


class Picture:
    pass


class Model:
    def __init__(self, shapes=None):
        self.S = shapes or LS.Shapes()
        self.budget3 = E.Budget(self.S.csrc).budget3

    def store_branch(self, w, h, g):
        """the branch of the store address group g's lanes take: 'narrow' (mbw < kMbPerGroup: a division per lane),
        'wrap' (some lane of the group lies on the next macroblock row) or 'no-wrap'"""
        M, mbw, nmb = self.S.kMbPerGroup, w // 16, (w // 16) * (h // 16)
        if mbw < M:
            return "narrow"
        gx = (g * M) % mbw
        return "wrap" if gx + min(M, nmb - g * M) - 1 >= mbw else "no-wrap"

    def picture(self, pkt, max_groups=None):
        """the rounds of a picture's chroma, by super group; max_groups: of the launch (it sizes the wave counts)"""
        S = self.S
        M, PG = S.kMbPerGroup, S.kPoolGroups
        pkt = np.ascontiguousarray(pkt, np.uint8)
        w, h = E.packet_size(pkt)
        Q = max(int(pkt[10]), 1)
        _, ciqt, _, cb8, _, _ = R.oracle_tables(Q)
        off = R.OracleDecoder().block_offsets(pkt).astype(np.int64) - 12
        data = pkt[12:]
        P = Picture()
        P.w, P.h, P.Q, P.nmb = w, h, Q, (w // 16) * (h // 16)
        P.groups = S.groups(w, h)
        P.nsg = S.super_groups(P.groups)
        P.cw = S.split_chroma_waves(max_groups or P.groups)
        P.data_len = data.size
        step = S.kXcds * P.cw
        P.rounds, P.listed = [], []
        for sg in range(P.nsg):
            r = Round()
            r.sg, r.owner, r.last = sg, S.split_owner(sg, P.cw, S.kSplitXcdRot, 0), sg + step >= P.nsg
            r.have_nn = sg + 2 * step < P.nsg
            r.groups, r.pools, r.listed, r.stored = [], [], [], 0
            for q in range(PG):
                g = Group()
                g.g = sg * PG + q
                g.exists = g.g < P.groups
                lane = np.arange(2 * M)
                mb = g.g * M + (lane % M)
                g.valid = mb < P.nmb
                blk = 6 * np.where(g.valid, mb, 0) + 4 + lane // M
                g.pos, g.len = off[blk], off[blk + 1] - off[blk]
                g.cls = np.full(2 * M, NONE)
                g.bytes = [None] * (2 * M)
                if cb8 != 0:  # tables with raw chroma bytes: every group the general way
                    g.gslow = g.exists
                else:
                    slow = g.valid & ((g.len > SHORT_MAX) | (g.len == 0) | (g.pos + g.len > P.data_len))
                    g.gslow = bool(slow.any())
                if g.exists and not g.gslow:
                    for l in np.nonzero(g.valid)[0]:
                        b = data[g.pos[l]:g.pos[l] + g.len[l]]
                        g.bytes[l] = b
                        g.cls[l] = UNCHANGED if b[0] == 0xFF else DC_ONLY if g.len[l] == 2 else BUSY
                g.cnt = int((g.cls == BUSY).sum())
                g.gstore = bool(((g.cls == DC_ONLY) | (g.cls == BUSY)).any())
                if g.gslow:
                    r.listed.append(g.g)
                r.groups.append(g)
            qa = 0
            while qa < PG:  # as many consecutive groups as have 64 busy blocks or fewer between them
                p = Pool()
                p.members, p.tot = [qa], r.groups[qa].cnt
                while qa + len(p.members) < PG and p.tot + r.groups[qa + len(p.members)].cnt <= POOL_LANES:
                    p.tot += r.groups[qa + len(p.members)].cnt
                    p.members.append(qa + len(p.members))
                qa += len(p.members)
                p.storing = [q for q in p.members if r.groups[q].gstore]
                p.bail, p.form, p.sums = False, None, []
                if not p.storing:
                    p.skipped = True  # mask == 0: nothing parsed, nothing stored
                    r.pools.append(p)
                    continue
                p.skipped = False
                if p.tot:
                    t3 = False
                    for q in p.storing:
                        gq = r.groups[q]
                        for l in np.nonzero(gq.cls == BUSY)[0]:
                            c = short_coefficients(gq.bytes[l], ciqt)
                            p.bail |= bool((c[~_LOW4] != 0).any())
                            t3 |= bool((c[_LOW4 & ~_LOW3] != 0).any())
                            p.sums.append(int(np.abs(c[_LOW3]).sum()))
                    if not p.bail:
                        p.form = "four" if t3 else "packed3" if max(p.sums) <= self.budget3 else "plain3"
                if p.bail:
                    r.listed += [r.groups[q].g for q in p.storing]
                else:
                    r.stored += len(p.storing)
                r.pools.append(p)
            r.listed.sort()
            r.counts = tuple(g.cnt for g in r.groups)
            r.partition = tuple(tuple(p.members) for p in r.pools)
            P.rounds.append(r)
            P.listed += r.listed
        return P

    def parts_listed(self, pkts):
        """chroma parts a split launch of these packets leaves to k_decode_list"""
        mg = max(self.S.groups(*E.packet_size(p)) for p in pkts)
        return sum(len(self.picture(p, mg).listed) for p in pkts)


# =========================================================================== directed packets
def tokens_block(dc, pairs):
    """DC, then (zig-zag slot, token value) pairs in rising slot order, zero runs between them and to the end"""
    out, co = [dc & 0xFF], 1
    for slot, v in pairs:
        assert slot >= co and -128 <= v <= 63 and v != 0
        if slot > co:
            out.append(63 + slot - co)
        out.append(v & 0xFF)
        co = slot + 1
    if co < 64:
        out.append(63 + 64 - co)
    return out


def b_ff():
    return [255]


def b_dc(dc, run=126):
    return [dc, run]  # 126: the run to the block's end; 127: one slot past it


def b_busy(rng, length, vmax=2, dcmax=200):
    """a busy block of `length` bytes (3..9): DC, length - 2 values on zig-zag slots 1 .. length - 2, one run.  Up to
    seven bytes everything lies in the low 3x3; eight and nine reach slot 6 (row 3 of column 0)."""
    vals = [(s, int(rng.integers(1, vmax + 1)) * int(rng.choice([-1, 1]))) for s in range(1, length - 1)]
    return tokens_block(int(rng.integers(0, dcmax + 1)), vals)


def b_busy8_low3(rng, vmax=2, dcmax=200):
    """eight bytes, nothing outside the low 3x3: slots 1-4, a run over 5 and 6, slot 7"""
    v = lambda: int(rng.integers(1, vmax + 1)) * int(rng.choice([-1, 1]))
    blk = tokens_block(int(rng.integers(0, dcmax + 1)), [(1, v()), (2, v()), (3, v()), (4, v()), (7, v())])
    assert len(blk) == 8
    return blk


def b_four(rng, slot=6):
    """DC, run, value, run: the value on row 3 (slot 6) or column 3 (slot 9) of the low 4x4"""
    return tokens_block(int(rng.integers(0, 201)), [(slot, int(rng.choice([-2, -1, 1, 2])))])


def b_bail(rng, slot=10):
    """DC, run, value, run: four bytes whose value lands outside the low 4x4 (slot 10: row 0, column 4)"""
    blk = tokens_block(int(rng.integers(0, 201)), [(slot, int(rng.choice([-3, -2, 2, 3])))])
    assert len(blk) == 4
    return blk


def group(rng, busy=0, lengths=(3, 4, 5, 6, 7), rest="dc", put=None, scatter=True, run127=False):
    """the 64 chroma blocks of a group by lane (Cb of the 32 macroblocks, then Cr): `busy` busy ones with lengths taken
    in turn, on lanes chosen at random (scatter) or on the first lanes; the rest DC only or unchanged; put: lane -> block"""
    lanes = sorted(rng.choice(64, busy, replace=False).tolist()) if scatter else list(range(busy))
    out = [None] * 64
    for i, l in enumerate(lanes):
        L = lengths[i % len(lengths)]
        out[l] = b_busy8_low3(rng) if L == "8low3" else b_busy(rng, L)
    for l in range(64):
        if out[l] is None:
            out[l] = b_ff() if rest == "ff" else b_dc(int(rng.integers(0, 255)), 127 if run127 and l % 2 else 126)
    for l, b in (put or {}).items():
        out[l] = b
    return out


def build_packet(rng, w, h, Q, rounds, S, default=None):
    """rounds: super group -> [group spec or None] * kPoolGroups; groups not named get default(rng) (ordinary content:
    a dozen busy blocks of three to seven bytes among DC-only ones).  Luma blocks are all DC only."""
    _, _, lb8, cb8, _, _ = R.oracle_tables(Q)
    assert cb8 == 0
    M, PG = S.kMbPerGroup, S.kPoolGroups
    nmb = (w // 16) * (h // 16)
    default = default or (lambda rng: group(rng, busy=int(rng.integers(8, 20))))
    specs = {}
    for g in range(S.groups(w, h)):
        given = rounds.get(g // PG)
        spec = given[g % PG] if given is not None and given[g % PG] is not None else default(rng)
        specs[g] = spec
    blocks = []
    for mb in range(nmb):
        for k in range(4):
            blocks.append([int(rng.integers(0, 255))] + [0] * lb8 + [63 + 63 - lb8])
        blocks.append(specs[mb // M][mb % M])
        blocks.append(specs[mb // M][M + mb % M])
    return E.packet_from_blocks(w, h, Q, blocks)


# busy counts per round -> the partition the kernel must make of them
PARTITIONS = {
    (64, 0, 0): ((0, 1, 2),),
    (32, 32, 0): ((0, 1, 2),),   # one pool of exactly 64
    (21, 21, 22): ((0, 1, 2),),  # one pool of exactly 64
    (22, 22, 21): ((0, 1), (2,)),
    (33, 31, 1): ((0, 1), (2,)),
    (1, 64, 0): ((0,), (1, 2)),
    (64, 64, 64): ((0,), (1,), (2,)),
    (0, 0, 0): ((0, 1, 2),),     # DC-only blocks alone
}
# three groups, one round: a group is a whole macroblock row (no wrap), rows narrower than a group (a division per
# lane), one long row (no wrap), and rows of a group and a half (768x32: the only one whose lanes wrap to the next row)
ONE_ROUND_SHAPES = ((512, 48), (256, 96), (1536, 16), (768, 32))
WAIT_ORDERS = ((3, 0, 1), (2, 3, 0), (1, 2, 3))  # groups stored along the rounds of stripe 0 of 1024x416
BUDGET_QUALITIES = (60, 20)


def budget3_tokens(Q, side, budget3, variant=0):
    """token values (per zig-zag slot) of a low-3x3 chroma block whose sum of |coefficients| is the largest not above
    ('in') or the smallest above ('out') the three-input budget that stepping one token reaches; 'far': well above,
    signs chosen so that every term adds at pixel (7, 7)"""
    _, ciqt, _, _, _, _ = R.oracle_tables(Q)
    q = np.array([int(ciqt[E.ZZ[k]]) for k in range(64)])
    slots = [1, 2, 3, 4, 5]
    tok = np.zeros(64, np.int64)
    tok[0] = min(254, 32767 // q[0]) - variant  # no int16 wrap of the DC
    total = lambda: int(sum(abs(int16(tok[k] * q[k])) for k in [0] + slots))
    lim = lambda k: min(128, 32767 // q[k])  # as far as a token goes without an int16 wrap of its product
    if side == "far":
        # under twice the budget, so that a range test with the budget doubled would still let it through
        for k in slots:
            odd = ((E.ZZ[k] >> 3) + (E.ZZ[k] & 7)) & 1
            tok[k] = -lim(k) if odd else min(63, lim(k))
        for _ in range(200):
            if total() <= 2 * budget3 - budget3 // 10:
                break
            for k in slots:
                tok[k] -= np.sign(tok[k]) * (abs(tok[k]) > 1)
        assert budget3 + 3000 < total() < 2 * budget3
        return tok
    used = []
    for k in slots:  # tokens of -128 (or as far as int16 allows) until the sum is above the budget
        tok[k] = -lim(k)
        used.append(k)
        if total() > budget3:
            break
    assert total() > budget3, (Q, total())
    while total() > budget3:  # the last token back until the sum is inside ...
        assert tok[used[-1]] < -1
        tok[used[-1]] += 1
    by_step = sorted(used, key=lambda s: q[s])
    for k in by_step:  # ... then every token, finest step first, as far as the sum stays inside
        while -tok[k] < lim(k):
            tok[k] -= 1
            if total() > budget3:
                tok[k] += 1
                break
    assert total() <= budget3
    if side == "out":
        k = next(s for s in by_step if -tok[s] < lim(s))  # the finest step there is: the smallest sum above
        tok[k] -= 1
        assert total() > budget3
    return tok


def pool_packets(shapes=None, seed=31):
    """[(name, packet)]: see the module's docstring and tests/test_pool_model_cpu.py for what each is held to"""
    S = shapes or LS.Shapes()
    B3 = E.Budget(S.csrc).budget3
    rng = np.random.default_rng(seed)
    out = []

    def counts_round(c, lengths=(3, 4, 5, 6, 7)):
        return [group(rng, busy=n, lengths=lengths) for n in c]

    # ---- 1. one round, every partition, on the shapes that reach each branch of the store address ----
    parts = list(PARTITIONS)
    for i, (w, h) in enumerate(ONE_ROUND_SHAPES):
        for j in range(3):
            c = parts[(3 * i + j) % len(parts)]
            out.append((f"one-round-{w}x{h}-{'-'.join(map(str, c))}", build_packet(rng, w, h, 255, {0: counts_round(c)}, S)))
    out.append(("one-round-512x48-all-unchanged",
                build_packet(rng, 512, 48, 255, {0: [group(rng, rest="ff") for _ in range(3)]}, S)))
    # ---- 2. 176x48: a second group of one macroblock (lanes without a block), busy and DC only ----
    out.append(("two-groups-176x48-busy-tail", build_packet(rng, 176, 48, 255, {0: [group(rng, busy=20), group(rng, busy=64), None]}, S)))
    out.append(("two-groups-176x48-dc-tail", build_packet(rng, 176, 48, 200, {0: [group(rng, busy=64), group(rng, busy=0), None]}, S)))
    # ---- 3. 1024x416: every partition again, one per round, and the all-unchanged round between storing ones ----
    rounds = {sg: counts_round(c) for sg, c in enumerate(parts)}
    rounds[8] = [group(rng, rest="ff") for _ in range(3)]  # stripe 0's middle round
    rounds[9] = counts_round((64, 64, 64), lengths=(3, 4, 5, 6, 7, 8))
    out.append(("partitions-1024x416", build_packet(rng, 1024, 416, 255, rounds, S)))
    # ---- 4. lengths (1024x224): 3..8 bytes, the two spellings of two bytes, nine bytes in one group of a round ----
    nine = lambda: b_busy(rng, 9)
    rounds = {
        0: [group(rng, busy=18, lengths=(3, 4, 5, 6, 7, 8), run127=True) for _ in range(3)],
        1: [group(rng, busy=12), group(rng, busy=12, put={37: nine()}), group(rng, busy=12)],  # not stripe 1's last round
        2: [group(rng, busy=10, lengths=("8low3", 7, 3)), group(rng, busy=0, run127=True), group(rng, busy=30, lengths=(8,))],
        8: [group(rng, busy=12, put={0: nine()}), group(rng, busy=12), group(rng, busy=12)],   # stripe 0's last round
        9: [group(rng, busy=15, lengths=(3, 5, 8), put={63: b_busy(rng, 5)}), None, None],  # the partial last super group: its last block ends the packet
    }
    lengths_pkt = build_packet(rng, 1024, 224, 255, rounds, S)
    out.append(("lengths-1024x224", lengths_pkt))
    # ---- 5. packet end: the same packet whole (above), one byte short, and the header alone ----
    out.append(("cut-one-byte-short-1024x224", lengths_pkt[:-1].copy()))
    out.append(("cut-header-alone-1024x224", lengths_pkt[:12].copy()))
    # ---- 6. bail (1024x416): pools of one, two and three groups, in a round that is not its wave's last and in one
    # that is; next to a bailing pool of one or two groups another pool of the round stores (a pool of three is the
    # whole round).  The pool of three holds exactly 64 busy blocks. ----
    def bail1():
        return [group(rng, busy=40, put={5: b_bail(rng)}), group(rng, busy=40), group(rng, busy=10)]

    def bail2():
        return [group(rng, busy=20), group(rng, busy=20, put={63: b_bail(rng, 14)}), group(rng, busy=60)]

    def bail3():
        g = [group(rng, busy=21, scatter=False), group(rng, busy=21, scatter=False), group(rng, busy=22, scatter=False)]
        g[2][3] = b_bail(rng)  # (a busy lane: the count stays 22)
        return g

    rounds = {0: bail1(), 10: bail1(), 1: bail2(), 11: bail2(), 4: bail3(), 12: bail3()}
    out.append(("bail-1024x416", build_packet(rng, 1024, 416, 255, rounds, S)))
    # ---- 7. the form of the transform inside one pool, on both sides of the three-input budget ----
    for Q in BUDGET_QUALITIES:
        def quiet(n=14):  # low 3x3, far inside the budget
            return group(rng, busy=n, lengths=(3, 4, 5, 6, 7, "8low3"))

        def lane_from(side, variant=0):
            return E.block_bytes(budget3_tokens(Q, side, B3, variant), 0)

        rounds = {
            0: [quiet(), quiet(), quiet()],                                        # packed
            1: [quiet(), quiet(20), quiet()],
            2: [quiet(), group(rng, busy=14, put={40: lane_from("out")}), quiet()],  # plain, for all three groups
            3: [quiet(), quiet(), group(rng, busy=14, put={7: lane_from("in")})],    # still packed
            4: [quiet(), group(rng, busy=14, put={9: b_four(rng, 9)}), quiet()],     # four-input, for all
            5: [group(rng, busy=14, put={22: lane_from("far")}), quiet(), quiet()],  # plain
            6: [quiet(), quiet(), group(rng, busy=14, put={1: b_four(rng, 6)})],     # four-input
        }
        for sg in range(7, 10):  # more blocks next to the budget, inside and outside in the same picture
            rounds[sg] = [group(rng, busy=14, put={l: lane_from("in" if (sg + q) & 1 else "out", 1 + l % 7 + 7 * q) for l in range(0, 64, 9)})
                          for q in range(3)]
        out.append((f"forms-1024x224-q{Q}", build_packet(rng, 1024, 224, Q, rounds, S)))
    # ---- 8. the DC-only pixel: every DC byte at three qualities (Q 1: the int16 product wraps from DC 13 on) ----
    for Q in (255, 128, 1):
        n = [0]

        def dcs(rng_):
            g = [b_dc((n[0] + l) % 255, 126) for l in range(64)]
            n[0] += 64
            return g
        out.append((f"dc-bytes-1024x32-q{Q}", build_packet(rng, 1024, 32, Q, {}, S, default=dcs)))
    # ---- 9. the arms of the counted wait: groups stored along the rounds of stripe 0 of 1024x416 ----
    step = S.kXcds * S.split_chroma_waves(S.groups(1024, 416))
    for order in WAIT_ORDERS:
        rounds = {}
        for i, n in enumerate(order):
            gs = [group(rng, busy=int(rng.integers(10, 20))) for _ in range(n)]
            # the groups that store nothing: unchanged blocks alone, or a nine-byte block (the list's)
            gs += [group(rng, rest="ff") if (i + k) & 1 else group(rng, busy=12, put={17: b_busy(rng, 9)}) for k in range(3 - n)]
            rounds[i * step] = [gs[(k + i) % 3] for k in range(3)]
        out.append((f"wait-arms-{''.join(map(str, order))}-1024x416", build_packet(rng, 1024, 416, 255, rounds, S)))
    return out


def pad_packet(extra):
    """a packet that is its header and `extra` bytes of nothing: a 16x16 picture cut short"""
    return np.concatenate([np.frombuffer(E.header(16, 16, 255, 12 + extra), np.uint8), np.zeros(extra, np.uint8)])


def aligned_plan(pkt):
    """[pad, pkt] four times over, the pads sized so that the four copies of pkt start at stream byte offsets
    0, 1, 2, 3 mod 4 when the packets are laid end to end.  Returns (packets, offsets of the copies)."""
    pkts, cur, at = [], 0, []
    for r in range(4):
        extra = (r - (cur + 12)) % 4
        pkts.append(pad_packet(extra))
        cur += 12 + extra
        at.append(cur)
        pkts.append(pkt)
        cur += pkt.size
    assert [a % 4 for a in at] == [0, 1, 2, 3]
    return pkts, at
