"""Statement of the DV timecode, recording date and time and aspect flag on resident frames (k_dv_meta_extract,
k_dv_meta_write: csrc/dv_meta_kernels.h).  TEST INFRASTRUCTURE ONLY: the product never imports it.  numpy and integers, no
ctypes: tests/test_dv_meta_cpu.py holds this file to csrc/dvframe_host.c's readers (mi_dv_timecode, mi_dv_date, mi_dv_time,
mi_dv_pixel_aspect) and to Python's datetime, and tests/test_gpu_dv_meta.py holds the kernels to this file, value for value
and byte for byte.

extract() restates GetSSYBPack and its users (lib/dvframe.c:678-783, :460-471) and its fields 0-4 and 6-12 are PINNED to
that file (tests/test_dvframe_reference_cpu.py, tests/test_dvframe_fixtures_cpu.py).  UNPINNED: the packs write() makes are
this repository's reading of IEC 61834-2/-4 from memory; what is checked is that the library's own
readers, on host and on device, read them back.  The readers' two-digit year has a pivot (below 25: 20xx, else 19xx), so a
year from 2025 on that write() records reads back as 19xx: the reference's rule, kept."""
import numpy as np

INTS = 16
FOUND, TC_H, TC_M, TC_S, TC_F, TC_DROP, YEAR, MONTH, DAY, HOUR, MINUTE, SECOND, WIDE, TC_RAW, DATE_RAW, TIME_RAW = range(INTS)
HAS_TIMECODE, HAS_DATE, HAS_TIME, HAS_CONTROL = 1, 2, 4, 8
PACK_TIMECODE, PACK_SOURCE, PACK_CONTROL, PACK_DATE, PACK_TIME = 0x13, 0x60, 0x61, 0x62, 0x63
CONTROL_AT = 80 * 5 + 48 + 5      # the VAUX source control pack mi_dv_pixel_aspect reads
DROP_PERIOD = 2589408             # frames of 24 hours of drop-frame timecode
LAST_SECOND = 3155760000          # 2070-01-01 00:00:00: recording times lie below it


class Meta:
    """what the packs need of a system: DIF sequences per channel, channels, and what k_dv_encode writes into the header
    (APT) and the VAUX source pack (stype)"""

    def __init__(self, system, seqs, chans, apt, stype):
        self.system, self.seqs, self.chans, self.apt, self.stype = system, seqs, chans, apt, stype
        self.dsf = int(seqs == 12)
        self.frame_bytes = chans * seqs * 150 * 80
        self.base = 25 if self.dsf else 30
        self.fps = (25, 1) if self.dsf else (30000, 1001)
        self.places = 12 * seqs  # subcode packets the readers scan: channel 0 alone


META = {m.system: m for m in (Meta(0, 10, 1, 0, 0), Meta(1, 12, 1, 0, 0), Meta(3, 12, 1, 1, 0), Meta(4, 10, 2, 1, 4),
                              Meta(5, 12, 2, 1, 4))}
SYSTEMS = tuple(META)


# ---- a frame number as a timecode, seconds as a date ----
def timecode_of(system, frame, drop):
    """(h, m, s, f) of frame number `frame`: base 25 (625/50) or 30; drop 1 (525/60 only) is SMPTE drop-frame.  Hours wrap
    at 24"""
    m = META[system]
    assert drop in (0, 1) and not (drop and m.dsf) and frame >= 0
    n = frame
    if drop:
        n %= DROP_PERIOD
        d, r = n // 17982, n % 17982
        n += 18 * d + (2 * ((r - 2) // 1798) if r >= 2 else 0)
    f, s = n % m.base, n // m.base
    return s // 3600 % 24, s // 60 % 60, s % 60, f


def civil_of(seconds):
    """(Y, M, D, h, m, s) of seconds from 1970-01-01 00:00:00 in the proleptic Gregorian calendar, no time zone; integers
    only (days to civil: years of 400 x 146097 days that begin on 1 March)"""
    assert seconds >= 0
    days, sod = divmod(seconds, 86400)
    z = days + 719468
    era, doe = divmod(z, 146097)
    yoe = (doe - doe // 1460 + doe // 36524 - doe // 146096) // 365
    doy = doe - (365 * yoe + yoe // 4 - yoe // 100)
    mp = (5 * doy + 2) // 153
    day, month = doy - (153 * mp + 2) // 5 + 1, mp + 3 if mp < 10 else mp - 9
    return yoe + era * 400 + (month <= 2), month, day, sod // 3600, sod // 60 % 60, sod % 60


def bcd(v):
    assert 0 <= v < 100
    return v // 10 << 4 | v % 10


def unbcd(b, tens_mask):
    return (b & 0xF) + 10 * ((b >> 4) & tens_mask)


# ---- the packs ----
def pack_timecode(hmsf, drop):
    h, m, s, f = hmsf
    return [PACK_TIMECODE, drop << 6 | bcd(f), 0x80 | bcd(s), 0x80 | bcd(m), 0xC0 | bcd(h)]


def pack_date(civil):
    return [0xFF] * 5 if civil is None else [PACK_DATE, 0xFF, 0xC0 | bcd(civil[2]), 0xE0 | bcd(civil[1]), bcd(civil[0] % 100)]


def pack_time(civil):
    return [0xFF] * 5 if civil is None else [PACK_TIME, 0xFF, 0x80 | bcd(civil[5]), 0x80 | bcd(civil[4]), 0xC0 | bcd(civil[3])]


def pack_source(system):
    m = META[system]
    return [PACK_SOURCE, 0xFF, 0xFF, 0xC0 | m.dsf << 5 | m.stype, 0xFF]


def pack_control(wide):
    return [PACK_CONTROL, 0x3F, 0xC8 | (2 if wide else 0), 0xFC, 0xFF]


def place_at(seq, block, packet):
    """byte offset of the pack (its id byte) of subcode packet `packet` of subcode block `block` of sequence `seq` (of the
    frame, in byte order: channel 1 follows channel 0)"""
    return seq * 12000 + 80 + 80 * block + 3 + 8 * packet + 3


def place_of(c):
    """candidate c of the readers' scan, and of the kernel's lane mapping (lane c % 64 of round c // 64)"""
    return c // 12, c % 12 // 6, c % 6


def block_at(fs, b):
    """byte offset of block b (0, 1: subcode; 2..4: VAUX) of sequence fs of the frame"""
    return (fs * 150 + 1 + b) * 80


def write_one(system, frame, number, drop, rec, wide):
    """one frame with the timecode of frame number `number`, the recording time `rec` (seconds; None: no date) and the
    aspect flag: the two subcode and three VAUX blocks of every sequence of every channel rewritten whole, no other byte"""
    m = META[system]
    out = np.array(frame, np.uint8)
    assert out.size == m.frame_bytes and wide in (0, 1)
    civil = None if rec is None else civil_of(rec)
    turn = (pack_timecode(timecode_of(system, number, drop), drop), pack_date(civil), pack_time(civil))
    vaux = (pack_source(system), pack_control(wide), pack_date(civil), pack_time(civil))
    for c in range(m.chans):
        for q in range(m.seqs):
            fs = c * m.seqs + q
            for j in range(2):
                blk = np.full(80, 0xFF, np.uint8)
                blk[:3] = (0x3F, q << 4 | c << 3 | 7, j)
                for k in range(6):
                    s = 6 * j + k
                    mid = m.apt if s in (0, 6, 11) else 7
                    blk[3 + 8 * k:3 + 8 * k + 3] = (int(q < m.seqs // 2) << 7 | mid << 4 | 0xF, 0xF0 | s, 0xFF)
                    blk[3 + 8 * k + 3:3 + 8 * k + 8] = turn[s % 3]
                out[block_at(fs, j):block_at(fs, j) + 80] = blk
            for v in range(3):
                blk = np.full(80, 0xFF, np.uint8)
                blk[:3] = (0x5F, q << 4 | c << 3 | 7, v)
                first = {0: 0, 2: 9}.get(v)
                if first is not None:
                    for i, p in enumerate(vaux):
                        blk[3 + 5 * (first + i):3 + 5 * (first + i) + 5] = p
                out[block_at(fs, 2 + v):block_at(fs, 2 + v) + 80] = blk
    return out


def rec_of(system, rec_seconds, k):
    """the recording time of frame k of a batch that starts at rec_seconds (below 0: none)"""
    num, den = META[system].fps
    return None if rec_seconds < 0 else rec_seconds + k * den // num


def write(system, frames, first_frame, drop, rec_seconds, wide):
    """the batch: frame k carries the timecode of frame number first_frame + k and the recording time rec_seconds +
    k frames, rounded down to a second"""
    m = META[system]
    assert rec_seconds < LAST_SECOND and first_frame >= 0
    frames = np.asarray(frames, np.uint8).reshape(-1, m.frame_bytes)
    return np.stack([write_one(system, f, first_frame + k, drop, rec_of(system, rec_seconds, k), wide) for k, f in enumerate(frames)])


def meta_mask(system):
    """True at the bytes of a frame's subcode and VAUX blocks"""
    m = META[system]
    mask = np.zeros(m.frame_bytes, bool)
    for fs in range(m.chans * m.seqs):
        mask[block_at(fs, 0):block_at(fs, 0) + 5 * 80] = True
    return mask


def find_pack(system, frame, pack_id):
    """GetSSYBPack: the first subcode packet of channel 0, by sequence, block, packet, whose pack has the id -> its five
    bytes, or None"""
    for c in range(META[system].places):
        at = place_at(*place_of(c))
        if frame[at] == pack_id:
            return [int(b) for b in frame[at:at + 5]]
    return None


def extract(system, frame):
    """one frame -> its row of INTS int32 (module constants name the indices).  Every field of a pack that was not found
    is 0"""
    frame = np.asarray(frame, np.uint8)
    row = np.zeros(INTS, np.int64)
    raw = lambda p: p[1] | p[2] << 8 | p[3] << 16 | p[4] << 24
    tc, date, time = (find_pack(system, frame, i) for i in (PACK_TIMECODE, PACK_DATE, PACK_TIME))
    if tc:
        row[FOUND] |= HAS_TIMECODE
        row[TC_H:TC_DROP + 1] = (unbcd(tc[4], 0x3), unbcd(tc[3], 0x7), unbcd(tc[2], 0x7), unbcd(tc[1], 0x3), tc[1] >> 6 & 1)
        row[TC_RAW] = raw(tc)
    if date:
        year = unbcd(date[4], 0xF)
        row[FOUND] |= HAS_DATE
        row[YEAR:DAY + 1] = (year + (2000 if year < 25 else 1900), unbcd(date[3], 0x1), unbcd(date[2], 0x3))
        row[DATE_RAW] = raw(date)
    if time:
        row[FOUND] |= HAS_TIME
        row[HOUR:SECOND + 1] = (unbcd(time[4], 0x3), unbcd(time[3], 0x7), unbcd(time[2], 0x7))
        row[TIME_RAW] = raw(time)
    if frame[CONTROL_AT] == PACK_CONTROL:  # mi_dv_pixel_aspect: its APT is byte 4 of the frame
        row[FOUND] |= HAS_CONTROL
        b, apt = int(frame[CONTROL_AT + 2]) & 7, int(frame[4]) & 7
        row[WIDE] = int(b == 2 or (apt == 0 and b == 7))
    return row.astype(np.uint32).view(np.int32)


# ---- frames the tests share ----
def blank_frame(system):
    """zeros that announce the system in the header block (DSF, APT; write() adds the stype)"""
    m = META[system]
    f = np.zeros(m.frame_bytes, np.uint8)
    f[3], f[5] = m.dsf << 7, m.apt
    return f


def noise_frame(system, seed, wiped=True):
    """random bytes that announce the system (DSF, APT, VAUX stype).  wiped: no subcode packet of either channel carries
    one of the three pack ids (0xFF stands where the noise had one)"""
    m = META[system]
    f = np.random.default_rng(seed).integers(0, 256, m.frame_bytes, dtype=np.uint8)
    f[3] = (f[3] & 0x7F) | m.dsf << 7
    f[5] = (f[5] & 0xF8) | m.apt
    f[80 * 5 + 48 + 3] = (f[80 * 5 + 48 + 3] & 0xE0) | m.stype
    if wiped:
        for fs in range(m.chans * m.seqs):
            for c in range(12):
                at = place_at(fs, c // 6, c % 6)
                if f[at] in (PACK_TIMECODE, PACK_DATE, PACK_TIME):
                    f[at] = 0xFF
    return f


def plant(frame, seq, block, packet, pack):
    """the five pack bytes into a subcode packet, in place"""
    at = place_at(seq, block, packet)
    frame[at:at + 5] = pack
    return frame


def some_pack(pack_id, rng):
    """a pack of the id with four random bytes"""
    return [pack_id] + [int(b) for b in rng.integers(0, 256, 4)]


PLANTED_IDS = (PACK_TIMECODE, PACK_DATE, PACK_TIME)


def planted_names(system):
    """the cases of planted_frame, every one tests/test_dv_meta_cpu.py runs:
      alone c      one pack (the ids in turns) at candidate place c alone: every one of the 120 / 144 places; every fourth
                   frame also has a source control pack with some display mode, and some APT in byte 4
      two a b      the same id at places a < b with different bytes: the first in scan order wins; pairs within one round
                   of the kernel's lane mapping (64 places a round) and across rounds; another id lies at a third place
      channel 1    packs only in channel 1 of a 4:2:2 system: not found
      off-place    the ids only at bytes of the subcode blocks that begin no pack: not found"""
    m = META[system]
    last = m.places - 1
    pairs = [(0, 1), (3, 63), (64, min(127, last - 1)), (65, 66), (63, 64), (0, last), (70, last), (62, 65)] + \
        ([(128, last), (62, 130), (127, 128)] if last > 128 else [(100, last)])  # (625/50: a third round)
    return [f"alone {c}" for c in range(m.places)] + [f"two {a} {b}" for a, b in pairs] + \
        (["channel 1"] if m.chans == 2 else []) + ["off-place"]


def rounds_of(what):
    """the rounds of the kernel's lane mapping a case's places lie in"""
    return tuple(int(c) // 64 for c in what.split()[1:])


def planted_frame(system, what):
    """a noise frame with the packs of case `what` planted (the same frame every time)"""
    m = META[system]
    kind, places = what.split()[0], [int(c) for c in what.split()[1:]]
    seed = 100000 * system + {"alone": 0, "two": 20000, "channel": 40000, "off-place": 50000}[kind] + sum((i + 1) * 150 * c for i, c in enumerate(places))
    rng = np.random.default_rng(seed)
    f = noise_frame(system, seed + 1)
    if kind == "alone":
        c = places[0]
        plant(f, *place_of(c), some_pack(PLANTED_IDS[c % 3], rng))
        if c % 4 == 0:
            f[CONTROL_AT], f[CONTROL_AT + 2] = PACK_CONTROL, (0x02, 0x07, 0xCA, 0xFF, 0x00, 0xC8)[c // 4 % 6]
            f[4] = (f[4] & 0xF8) | (0 if c % 8 == 0 else c % 7 + 1)
    elif kind == "two":
        a, b = places
        pid = PLANTED_IDS[(a + b) % 3]
        first, second = some_pack(pid, rng), some_pack(pid, rng)
        second[1] = first[1] ^ 0x15  # (never the same bytes)
        plant(f, *place_of(a), first)
        plant(f, *place_of(b), second)
        third = next(c for c in ((a + 7) % m.places, (a + 9) % m.places) if c not in (a, b))
        plant(f, *place_of(third), some_pack(PLANTED_IDS[(a + b + 1) % 3], rng))
    elif kind == "channel":
        for n, pid in enumerate(PLANTED_IDS):
            plant(f, m.seqs + 3 * n, n % 2, 2 * n, some_pack(pid, rng))
    else:
        for q in range(m.seqs):
            for j in range(2):
                for p in range(80):
                    if p < 3 or p >= 51 or (p - 3) % 8 != 3:
                        f[block_at(q, j) + p] = PLANTED_IDS[(q + j + p) % 3]
    return f
