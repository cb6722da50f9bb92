"""The statement of DVD subpictures (fourcc 'DVDS') as lib/subovl_dvd.c (S) decodes them: what libmi_spu.so is checked
against, byte for byte (include/mi_spu.h states the rules and cites the lines).

`parse` restates the control walk (S:186-256) and what upstream returns beside the picture (S:311-323); `decode` adds the
local palette (S:260-266), the two fields (S:132-147, S:294-304) and the scanline (S:77-130), loop for loop: get_nibble, the
read pointer that is not reset between sequences, pos < len at a line's start only.  Where upstream would read outside the
packet, or write nothing or across rows, the library's statuses are returned in its order: SHORT, CTRL_RANGE, RECT,
DATA_RANGE.

`encode` is a deterministic packer (the shortest code a run, runs over 255 split, lines ended with fill codes or without),
`build` assembles a packet from field bytes and control sequences, and the builders below make every quirk the tests name.
Pictures are (H, W, 4) uint8 arrays, GAVL_YUVA_32; a palette is the disc's 16 uint32."""
import collections

import numpy as np

OK, SHORT, CTRL_RANGE, RECT, DATA_RANGE = range(5)
STATUSES = {"SHORT": SHORT, "CTRL_RANGE": CTRL_RANGE, "RECT": RECT, "DATA_RANGE": DATA_RANGE}
MAX_SIDE = 4096

# the fields of mi_spu_info, in its order
Info = collections.namedtuple("Info", "status src_w src_h dst_x dst_y lines1 lines2 ctrl_start offset1 offset2 x1 x2 y1 y2 sequences "
                                      "palette alpha ctrl_end")


class _Range(Exception):
    pass


def be16(buf, at):
    return int(buf[at]) << 8 | int(buf[at + 1])


def parse(packet, W, H):
    """the Info of a packet's control section for a video of W x H: status OK, SHORT, CTRL_RANGE or RECT; lines1 and lines2
    are 0.  A command that cannot be read whole changes nothing."""
    buf = np.frombuffer(bytes(packet), np.uint8)
    n = buf.size
    palette, alpha = [0, 0, 0, 0], [0, 0, 0, 0]
    x1 = y1 = x2 = y2 = offset1 = offset2 = sequences = 0

    def info(status, ctrl_start, ptr, rect=True):
        src_w, src_h = (x2 - x1 + 1, y2 - y1 + 1) if rect else (0, 0)
        dst_x, dst_y = (x1, y1) if rect else (0, 0)
        if rect and dst_x + src_w > W:                                    # S:319-323
            dst_x = W - src_w
        if rect and dst_y + src_h > H:
            dst_y = H - src_h
        return Info(status, src_w, src_h, dst_x, dst_y, 0, 0, ctrl_start, offset1, offset2, x1, x2, y1, y2, sequences,
                    tuple(palette), tuple(alpha), ptr)

    if n < 4:
        return Info(SHORT, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, (0, 0, 0, 0), (0, 0, 0, 0), 0)
    ctrl_offset = ctrl_start = be16(buf, 2)                               # S:186-187
    ptr = ctrl_offset                                                     # S:190

    def need(k):
        if ptr + k > n:
            raise _Range

    try:
        while True:                                                       # S:192
            need(4)
            next_ctrl_offset = be16(buf, ptr + 2)                         # S:195-197: the date is skipped
            ptr += 4
            sequences += 1
            ctrl_seq_end = False
            while not ctrl_seq_end:                                       # S:201
                need(1)
                cmd = int(buf[ptr])
                if cmd == 0x03:                                           # S:216-222
                    need(3)
                    palette = [int(buf[ptr + 2]) & 15, int(buf[ptr + 2]) >> 4, int(buf[ptr + 1]) & 15, int(buf[ptr + 1]) >> 4]
                    ptr += 3
                elif cmd == 0x04:                                         # S:223-229
                    need(3)
                    alpha = [int(buf[ptr + 2]) & 15, int(buf[ptr + 2]) >> 4, int(buf[ptr + 1]) & 15, int(buf[ptr + 1]) >> 4]
                    ptr += 3
                elif cmd in (0x05, 0x85):                                 # S:230-237
                    need(7)
                    p = [int(b) for b in buf[ptr + 1:ptr + 7]]
                    x1, x2 = p[0] << 4 | p[1] >> 4, (p[1] & 15) << 8 | p[2]
                    y1, y2 = p[3] << 4 | p[4] >> 4, (p[4] & 15) << 8 | p[5]
                    ptr += 7
                elif cmd == 0x06:                                         # S:238-241
                    need(5)
                    offset1, offset2 = be16(buf, ptr + 1), be16(buf, ptr + 3)
                    ptr += 5
                elif cmd == 0xff:                                         # S:242-244
                    ctrl_seq_end = True
                    ptr += 1
                else:                                                     # S:208-215, S:245-249: one byte
                    ptr += 1
            if ctrl_offset == next_ctrl_offset:                           # S:253-255: ptr stays where it is
                break
            ctrl_offset = next_ctrl_offset
    except _Range:
        return info(CTRL_RANGE, ctrl_start, ptr, rect=False)
    width = x2 - x1 + 1
    return info(RECT if width < 1 or width > W else OK, ctrl_start, ptr)


def local_palette(info, palette16):
    """S:260-266, the little-endian arm: four colours of four bytes"""
    out = np.zeros((4, 4), np.uint8)
    for i in range(4):
        e = int(palette16[info.palette[i]])
        out[i] = ((e >> 16) & 255, (e >> 8) & 255, e & 255, info.alpha[i] * 17)
    return out


def get_nibble(buf, ptr, nibble_offset):                                  # S:77-80
    at = ptr + (nibble_offset >> 1)
    if at >= buf.size:
        raise _Range
    return (int(buf[at]) >> ((1 - (nibble_offset & 1)) << 2)) & 0xf


def decode_scanline(buf, ptr, dst, palette, width):                       # S:82-130
    x = nibble_offset = 0
    while True:
        v = get_nibble(buf, ptr, nibble_offset)
        nibble_offset += 1
        if v < 0x4:
            v = (v << 4) | get_nibble(buf, ptr, nibble_offset)
            nibble_offset += 1
            if v < 0x10:
                v = (v << 4) | get_nibble(buf, ptr, nibble_offset)
                nibble_offset += 1
                if v < 0x040:
                    v = (v << 4) | get_nibble(buf, ptr, nibble_offset)
                    nibble_offset += 1
                    if v < 4:
                        v |= (width - x) << 2
        length, color = v >> 2, v & 0x03
        if x + length > width:                                            # S:114-118
            length = width - x
        dst[x:x + length] = palette[color]
        x += length
        if x >= width:
            return (nibble_offset + (nibble_offset & 1)) >> 1


def decode_field(buf, ptr, length, pic, first_row, width, palette, max_height):  # S:132-147
    ypos = pos = 0
    while pos < length and ypos < max_height:
        pos += decode_scanline(buf, ptr + pos, pic[first_row + 2 * ypos], palette, width)
        ypos += 1
    return ypos


def decode(packet, W, H, palette16):
    """(status, the picture as (H, W, 4) uint8 or None, the Info with the lines each field decoded)"""
    buf = np.frombuffer(bytes(packet), np.uint8)
    info = parse(buf, W, H)
    if info.status != OK:
        return info.status, None, info
    pic = np.zeros((H, W, 4), np.uint8)                                   # S:182
    pal = local_palette(info, palette16)
    width = info.x2 - info.x1 + 1
    try:                                                                  # S:294-304
        lines1 = decode_field(buf, info.offset1, info.offset2 - info.offset1, pic, 0, width, pal, H // 2)
        lines2 = decode_field(buf, info.offset2, info.ctrl_start - info.offset2, pic, 1, width, pal, H // 2)
    except _Range:
        return DATA_RANGE, None, info._replace(status=DATA_RANGE)
    return OK, pic, info._replace(lines1=lines1, lines2=lines2)


# ------------------------------------------------------------------ the packer
def code(length, colour, nibbles=0):
    """the nibbles of one run: the shortest code, or one of `nibbles` nibbles where the length allows it; length 0: the
    fill code"""
    if length == 0:
        return [0, 0, 0, colour]
    assert 1 <= length <= 255 and 0 <= colour <= 3
    least = 1 if length < 4 else 2 if length < 16 else 3 if length < 64 else 4
    k = nibbles or least
    assert k == least or k == 4, f"a run of {length} has a code of {least} nibbles, or of 4"
    v = length << 2 | colour
    return [(v >> (4 * (k - 1 - i))) & 15 for i in range(k)]


def runs_of(row):
    """[(length, colour)] of a row of colour indices"""
    row = np.asarray(row)
    cuts = np.flatnonzero(np.diff(row)) + 1
    starts = np.concatenate([[0], cuts])
    ends = np.concatenate([cuts, [row.size]])
    return [(int(e - s), int(row[s])) for s, e in zip(starts, ends)]


def line_nibbles(row, fill_ends=True, wide=False):
    """a row of colour indices as nibbles, padded to a whole byte: the shortest code a run (wide: codes of 4 nibbles),
    runs over 255 split, the last run as a fill code if fill_ends"""
    out = []
    runs = runs_of(row)
    for k, (length, colour) in enumerate(runs):
        if fill_ends and k == len(runs) - 1:
            out += code(0, colour)
            break
        while length:
            part = min(length, 255)
            out += code(part, colour, 4 if wide else 0)
            length -= part
    return out + [0] * (len(out) & 1)


def to_bytes(nibbles):
    assert len(nibbles) % 2 == 0
    a = np.array(nibbles, np.uint8).reshape(-1, 2)
    return (a[:, 0] << 4 | a[:, 1]).astype(np.uint8).tobytes()


def field_bytes(rows, fill_ends=True, wide=False):
    return b"".join(to_bytes(line_nibbles(r, fill_ends, wide)) for r in rows)


def cmd_palette(p4):
    return bytes([0x03, p4[3] << 4 | p4[2], p4[1] << 4 | p4[0]])


def cmd_alpha(a4):
    return bytes([0x04, a4[3] << 4 | a4[2], a4[1] << 4 | a4[0]])


def cmd_rect(x1, x2, y1, y2, cmd=0x05):
    return bytes([cmd, x1 >> 4, (x1 & 15) << 4 | x2 >> 8, x2 & 255, y1 >> 4, (y1 & 15) << 4 | y2 >> 8, y2 & 255])


def cmd_offsets(o1, o2):
    return bytes([0x06, o1 >> 8, o1 & 255, o2 >> 8, o2 & 255])


def build(field1, field2, sequences, offsets=None):
    """a packet: 2 bytes of size, 2 of the control section's offset, the two fields, the control section.  sequences: a list
    of functions (offset1, offset2) -> the commands of one sequence (without ff); sequence k names sequence k + 1 as its
    next, the last one itself, as discs do.  offsets: what the 06 commands say, if not where the fields lie."""
    o1, o2 = 4, 4 + len(field1)
    ctrl_start = o2 + len(field2)
    said = offsets or (o1, o2)
    bodies = [s(*said) + b"\xff" for s in sequences]
    at, ctrl = ctrl_start, b""
    for k, body in enumerate(bodies):
        nxt = at + 4 + len(body) if k + 1 < len(bodies) else at
        ctrl += bytes([0x44, 0x44 + k, nxt >> 8, nxt & 255]) + body
        at += 4 + len(body)
    size = ctrl_start + len(ctrl)
    assert size < 65536
    return np.frombuffer(bytes([size >> 8, size & 255, ctrl_start >> 8, ctrl_start & 255]) + field1 + field2 + ctrl, np.uint8)


def usual(x1, x2, y1, y2, palette4=(0, 1, 2, 3), alpha4=(0, 15, 15, 15), with_offsets=True):
    """one sequence as discs write it: palette, alpha, rectangle, offsets, start display"""
    return lambda o1, o2: (cmd_palette(palette4) + cmd_alpha(alpha4) + cmd_rect(x1, x2, y1, y2)
                           + (cmd_offsets(o1, o2) if with_offsets else b"") + b"\x01")


def encode(indices, x1=0, y1=0, palette4=(0, 1, 2, 3), alpha4=(0, 15, 15, 15), fill_ends=True, wide=False, y2=None, more=()):
    """the packet of a picture of colour indices, (rows, width): even rows to field 1, odd rows to field 2, the rectangle
    x1, y1 .. x1 + width - 1, y2 (default: y1 + rows - 1).  more: further sequences (functions as build takes them)."""
    indices = np.asarray(indices)
    rows, width = indices.shape
    y2 = y1 + rows - 1 if y2 is None else y2
    return build(field_bytes(indices[0::2], fill_ends, wide), field_bytes(indices[1::2], fill_ends, wide),
                 [usual(x1, x1 + width - 1, y1, y2, palette4, alpha4)] + list(more))


def expected(indices, W, H, info, palette16):
    """the picture an encoded array of indices must decode to: the indices through the local palette at the frame's origin"""
    pic = np.zeros((H, W, 4), np.uint8)
    pal = local_palette(info, palette16)
    rows, width = indices.shape
    pic[:rows, :width] = pal[indices]
    return pic


def random_palette(rng):
    return rng.integers(0, 1 << 32, 16, dtype=np.uint64).astype(np.uint32)


def random_indices(rng, rows, width, mean_run=6):
    """rows of runs with geometric lengths around mean_run, a few of them long"""
    out = np.zeros((rows, width), np.uint8)
    for r in range(rows):
        x = 0
        while x < width:
            length = int(rng.geometric(1.0 / mean_run)) * (40 if rng.integers(0, 12) == 0 else 1)
            out[r, x:x + length] = rng.integers(0, 4)
            x += length
    return out


# ------------------------------------------------------------------ the quirks
def two_sequences(indices, x1=0, y1=0):
    """the second sequence changes palette and alpha: the last one wins"""
    return encode(indices, x1, y1, (0, 1, 2, 3), (0, 15, 15, 15),
                  more=[lambda o1, o2: b"\x02" + cmd_palette((7, 9, 4, 12)) + cmd_alpha((15, 3, 0, 9))])


def unknown_command(indices, x1=0, y1=0):
    """a 07 in front of the usual commands, with four operand bytes that upstream reads as commands: 04 with its two bytes
    (alpha 1, 2, 3, 4), then 00 (S:245-249)"""
    rows, width = indices.shape
    seq = lambda o1, o2: b"\x07\x04\x43\x21\x00" + cmd_palette((3, 2, 1, 0)) + cmd_rect(x1, x1 + width - 1, y1, y1 + rows - 1) + cmd_offsets(o1, o2)  # noqa: E731
    return build(field_bytes(indices[0::2]), field_bytes(indices[1::2]), [seq])


def clamped(width, rows=2):
    """every line is a run of 3 of colour 2 and a run of 255 of colour 1: x + len > width (S:114-118)"""
    line = to_bytes(code(3, 2) + code(255, 1) + [0])
    return build(line * (rows - rows // 2), line * (rows // 2), [usual(0, width - 1, 0, rows - 1)])


def field_ends_mid_line(indices):
    """offset2 is said one byte into field 1's last line (which is 4 bytes or more): pos < len holds at that line's start,
    and the line is decoded whole, past its field (S:139-141); field 2 then starts at the line's second byte"""
    f1, f2 = field_bytes(indices[0::2], fill_ends=False, wide=True), field_bytes(indices[1::2], fill_ends=False, wide=True)
    last = len(field_bytes(indices[0::2][-1:], fill_ends=False, wide=True))
    assert last >= 4
    rows, width = indices.shape
    return build(f1, f2, [usual(0, width - 1, 0, rows - 1)], offsets=(4, 4 + len(f1) - last + 1))


def lines_beyond_y2(indices, y2):
    """the rectangle says fewer rows than the fields hold: the count of lines comes from the data (S:139-146)"""
    return encode(indices, y2=y2)


def fewer_lines(indices, said_rows):
    """the rectangle says more rows than the fields hold: the rows below stay 0"""
    return encode(indices, y2=said_rows - 1)


def no_offsets(indices):
    """no 06 command: both offsets are 0, field 1 has length 0, field 2 decodes the packet's own head (S:161, S:294-304)"""
    rows, width = indices.shape
    return build(field_bytes(indices[0::2]), field_bytes(indices[1::2]), [usual(0, width - 1, 0, rows - 1, with_offsets=False)])


def reversed_offsets(indices):
    """offset2 < offset1: field 1 has a negative length and decodes nothing; field 2 runs from offset2 to ctrl_start, over
    both fields' bytes"""
    f1, f2 = field_bytes(indices[0::2]), field_bytes(indices[1::2])
    rows, width = indices.shape
    return build(f1, f2, [usual(0, width - 1, 0, rows - 1)], offsets=(4 + len(f1), 4))


def bad_packets(W, H):
    """name -> (packet, status): every refusal, and packets bad in two ways whose code the order decides.  "field 2 runs off
    the packet" has a line of W pixels that walks through the control section, whose dates are 44 4x so that it holds no
    fill code: tests/test_spuraw_cpu.py holds it to its status for the frames the tests use."""
    idx = np.array([[1, 1, 2, 0], [3, 3, 3, 1]], np.uint8)
    good = encode(idx)
    ctrl = be16(good, 2)
    fill = b"\x00\x01"
    end = build(fill, fill, [usual(0, 7, 0, 1)]).size  # field 1 is said to be the packet's last byte, ff: 6 pixels of 8
    return {
        "three bytes": (good[:3], SHORT),
        "no bytes": (good[:0], SHORT),
        "control offset past the end": (np.frombuffer(bytes([0, 9, 0, 200, 1, 2, 3, 4, 5]), np.uint8), CTRL_RANGE),
        "control section cut in the rectangle": (good[:ctrl + 4 + 3 + 3 + 4], CTRL_RANGE),
        "no ff before the end": (good[:-1], CTRL_RANGE),
        "a second sequence that is not there": (np.concatenate([good[:ctrl + 2], np.array([0, 0], np.uint8), good[ctrl + 4:]]), CTRL_RANGE),
        "cut in the control section, and no rectangle": (good[:ctrl + 6], CTRL_RANGE),
        "width 0": (build(fill, fill, [usual(5, 4, 0, 1)]), RECT),
        "x2 below x1": (build(fill, fill, [usual(9, 2, 0, 1)]), RECT),
        "wider than the frame": (encode(np.ones((2, W + 1), np.uint8)), RECT),
        "wider than the frame, and data past the end": (build(b"", b"", [usual(0, W, 0, 1)], offsets=(200, 300)), RECT),
        "field 1 past the end": (build(b"", b"", [usual(0, 3, 0, 1)], offsets=(200, 300)), DATA_RANGE),
        "field 1 runs off the packet": (build(fill, fill, [usual(0, 7, 0, 1)], offsets=(end - 1, end)), DATA_RANGE),
        "field 2 runs off the packet": (build(fill, b"\x44", [lambda o1, o2: cmd_rect(0x111, 0x110 + W, 0x111, 0x112) + cmd_offsets(o1, o2)]), DATA_RANGE),
    }
