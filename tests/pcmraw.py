"""The statement of the PCM family: what lib/audio_pcm.c (P) makes of a packet, restated twice.

`upstream` is P loop for loop: get_packet's byte count, decode_frame_pcm's chunk loop of at most 1024 sample frames, and
each of the seventeen functions with its own num_samples, num_bytes and loop bound.  The frame buffer is filled with
PATTERN before every call, so the result says which samples a function wrote.  The float readers are P:399-520 with Python
integers and exact power-of-two scaling; where 1 << exponent is undefined they raise OutsideDomain.

`decode` is the same in numpy, whole packet at once, with the library's three stated departures (include/mi_pcm.h): the
tail under a sample frame is dropped, the samples of an LPCM group tail are zeros, and a float outside the domain is its
IEEE value and is counted.  tests/test_pcmraw_cpu.py holds the two to each other and to upstream's recorded results."""
import math
import struct

import numpy as np

FRAME_SAMPLES = 1024  # P:32
PATTERN = 0xA5

CODECS = ("COPY8", "COPY16", "SWAP16", "S24LE", "S24BE", "LPCM24", "LPCM24_MONO", "LPCM20", "LPCM20_MONO", "COPY32", "SWAP32",
          "F32LE", "F32BE", "F64LE", "F64BE", "ULAW", "ALAW")
# upstream's function on a little-endian host (P:385-395)
FUNCTIONS = ("decode_8", "decode_s_16", "decode_s_16_swap", "decode_s_24_le", "decode_s_24_be", "decode_s_24_lpcm",
             "decode_s_24_lpcm_mono", "decode_s_20_lpcm", "decode_s_20_lpcm_mono", "decode_s_32", "decode_s_32_swap",
             "decode_float_32_le", "decode_float_32_be", "decode_float_64_le", "decode_float_64_be", "decode_ulaw", "decode_alaw")
# (input bytes, output bytes, samples) of a group
GROUPS = ((1, 1, 1), (2, 2, 1), (2, 2, 1), (3, 4, 1), (3, 4, 1), (12, 16, 4), (6, 8, 2), (10, 16, 4), (5, 8, 2), (4, 4, 1), (4, 4, 1),
          (4, 4, 1), (4, 4, 1), (8, 8, 1), (8, 8, 1), (1, 2, 1), (1, 2, 1))
LPCM = (5, 6, 7, 8)
MONO = (6, 8)
FLOATS = (11, 12, 13, 14)
LABELS = ("U8", "S8", "U16", "S16", "S32", "FLOAT", "DOUBLE")


def codec(name):
    return CODECS.index(name)


def sample_bytes(c):
    return GROUPS[c][1] // GROUPS[c][2]


class OutsideDomain(Exception):
    """1 << exponent of P:419-422 or P:481-484 is undefined for this sample"""


# ------------------------------------------------------------------ G.711 (P:650-684, 721-754): the closed forms
def ulaw(b):
    u = ~b & 0xFF
    t = (((u & 15) << 3) + 0x84) << ((u >> 4) & 7)
    return 0x84 - t if u & 0x80 else t - 0x84


def alaw(b):
    a = b ^ 0x55
    t, seg = (a & 15) << 4, (a >> 4) & 7
    t = t + 8 if seg == 0 else (t + 0x108) << (0 if seg == 1 else seg - 1)
    return t if a & 0x80 else -t


ULAW = np.array([ulaw(b) for b in range(256)], np.int16)
ALAW = np.array([alaw(b) for b in range(256)], np.int16)


# ------------------------------------------------------------------ the float readers, P:399-520
def _shift(exponent):
    if abs(exponent) > 30:  # 1 << 31 overflows an int, 1 << 32 and more shifts past its width
        raise OutsideDomain(exponent)
    return 1 << abs(exponent)


def float32_read(c, big):
    """P:399-454 on four bytes; the bits of the float it returns"""
    if not big:
        c = c[::-1]
    negative = c[0] & 0x80
    exponent = ((c[0] & 0x7F) << 1) | (1 if c[1] & 0x80 else 0)
    mantissa = ((c[1] & 0x7F) << 16) | (c[2] << 8) | c[3]
    if not (exponent or mantissa):
        return 0
    mantissa |= 0x800000
    exponent = exponent - 127 if exponent else 0
    fvalue = mantissa / 0x800000  # 24 bits over a power of two: exact
    if negative:
        fvalue *= -1
    if exponent > 0:
        fvalue *= _shift(exponent)
    elif exponent < 0:
        fvalue /= _shift(exponent)
    bits = struct.unpack("<I", struct.pack("<f", fvalue))[0]
    assert struct.unpack("<f", struct.pack("<I", bits))[0] == fvalue  # (nothing was rounded)
    return bits


def double64_read(c, big):
    """P:456-520 on eight bytes; the bits of the double it returns"""
    if not big:
        c = c[::-1]
    negative = 1 if c[0] & 0x80 else 0
    exponent = ((c[0] & 0x7F) << 4) | ((c[1] >> 4) & 0xF)
    dvalue = float(((c[1] & 0xF) << 24) | (c[2] << 16) | (c[3] << 8) | c[4])
    dvalue += ((c[5] << 16) | (c[6] << 8) | c[7]) / float(0x1000000)  # 52 bits in all: exact
    if exponent == 0 and dvalue == 0.0:
        return 0
    dvalue += 0x10000000
    exponent = exponent - 0x3FF
    dvalue = dvalue / float(0x10000000)
    if negative:
        dvalue *= -1
    if exponent > 0:
        dvalue *= _shift(exponent)
    elif exponent < 0:
        dvalue /= _shift(exponent)
    return struct.unpack("<Q", struct.pack("<d", dvalue))[0]


# ------------------------------------------------------------------ upstream, loop for loop
def _u32(x):
    return struct.pack("<I", x & 0xFFFFFFFF)


def _one_call(c, ch, src, frame, outside):
    """one call of codec c's function on the bytes left: writes the frame, returns (num_samples, num_bytes, samples
    outside the domain); outside "raise" or "ieee" """
    left, count = len(src), 0
    a, _, _ = GROUPS[c]
    name = CODECS[c]
    if name in ("LPCM20", "LPCM20_MONO"):
        num_samples = (2 * left) // (5 * ch)  # P:270, 304
    elif name in ("LPCM24", "LPCM24_MONO"):
        num_samples = left // (3 * ch)  # P:203, 237 (mono: ch is 1)
    else:
        num_samples = left // (a * ch)
    num_samples = min(num_samples, FRAME_SAMPLES)
    if name in ("LPCM20", "LPCM20_MONO"):
        num_bytes = (num_samples * 5 * ch) // 2  # P:275, 309
    elif name in ("LPCM24", "LPCM24_MONO"):
        num_bytes = num_samples * 3 * ch
    else:
        num_bytes = num_samples * a * ch
    if name in ("COPY8", "COPY16", "COPY32"):
        frame[:num_bytes] = src[:num_bytes]  # memcpy
    elif name in ("SWAP16", "SWAP32"):
        for i in range(num_samples * ch):
            frame[a * i:a * i + a] = src[a * i:a * i + a][::-1]
    elif name == "S24LE":
        for i in range(num_samples * ch):
            s = src[3 * i:3 * i + 3]
            frame[4 * i:4 * i + 4] = _u32(s[0] << 8 | s[1] << 16 | s[2] << 24)
    elif name == "S24BE":
        for i in range(num_samples * ch):
            s = src[3 * i:3 * i + 3]
            frame[4 * i:4 * i + 4] = _u32(s[2] << 8 | s[1] << 16 | s[0] << 24)
    elif name == "LPCM24":
        for i in range((num_samples * ch) // 4):  # P:213
            s = src[12 * i:12 * i + 12]
            for k in range(4):
                frame[16 * i + 4 * k:16 * i + 4 * k + 4] = _u32(s[2 * k] << 24 | s[2 * k + 1] << 16 | s[8 + k] << 8)
    elif name == "LPCM24_MONO":
        for i in range(num_samples // 2):  # P:247
            s = src[6 * i:6 * i + 6]
            for k in range(2):
                frame[8 * i + 4 * k:8 * i + 4 * k + 4] = _u32(s[2 * k] << 24 | s[2 * k + 1] << 16 | s[4 + k] << 8)
    elif name == "LPCM20":
        for i in range((num_samples * ch) // 4):  # P:280
            s = src[10 * i:10 * i + 10]
            d = (s[0] << 24 | s[1] << 16 | (s[8] & 0xF0) << 8, s[2] << 24 | s[3] << 16 | (s[8] & 0x0F) << 12,
                 s[4] << 24 | s[5] << 16 | (s[9] & 0xF0) << 8, s[6] << 24 | s[7] << 16 | (s[9] & 0x0F) << 12)
            for k in range(4):
                frame[16 * i + 4 * k:16 * i + 4 * k + 4] = _u32(d[k])
    elif name == "LPCM20_MONO":
        for i in range(num_samples // 2):  # P:314
            s = src[5 * i:5 * i + 5]
            frame[8 * i:8 * i + 4] = _u32(s[0] << 24 | s[1] << 16 | (s[4] & 0xF0) << 8)
            frame[8 * i + 4:8 * i + 8] = _u32(s[2] << 24 | s[3] << 16 | (s[4] & 0x0F) << 12)
    elif name in ("F32LE", "F32BE", "F64LE", "F64BE"):
        big, read = name.endswith("BE"), float32_read if a == 4 else double64_read
        for i in range(num_samples * ch):
            s = bytes(src[a * i:a * i + a])
            try:
                bits = read(s, big)
            except OutsideDomain:
                if outside == "raise":
                    raise
                bits, count = int.from_bytes(s, "big" if big else "little"), count + 1
            frame[a * i:a * i + a] = bits.to_bytes(a, "little")
    else:
        table = ULAW if name == "ULAW" else ALAW
        for i in range(num_samples * ch):
            frame[2 * i:2 * i + 2] = struct.pack("<h", int(table[src[i]]))
    return num_samples, num_bytes, count


def upstream(c, ch, data, outside="raise"):
    """decode_frame_pcm until the packet is done or a call gives 0 samples: [(valid_samples, the frame's bytes for them)]
    a chunk, the bytes left, and the samples outside the domain (outside="ieee"; "raise" raises at the first)"""
    data = bytes(data)
    at, chunks, total = 0, [], 0
    size = sample_bytes(c)
    while True:
        frame = bytearray([PATTERN]) * (FRAME_SAMPLES * ch * size)
        n, used, count = _one_call(c, ch, data[at:], frame, outside)
        at, total = at + used, total + count
        chunks.append((n, bytes(frame[:n * ch * size])))
        if at == len(data) or n == 0:  # P:1255: bytes_in_packet is 0; or the tail upstream never finishes
            break
    return chunks, len(data) - at, total


def chunk_loop(c, ch, lengths):
    """the arithmetic of the chunk loop alone, for an array of lengths at once: (frames, samples written, bytes consumed)"""
    left = np.asarray(lengths, np.int64).copy()
    frames, written, consumed = np.zeros_like(left), np.zeros_like(left), np.zeros_like(left)
    a, _, g = GROUPS[c]
    lp20, lp24 = CODECS[c].startswith("LPCM20"), CODECS[c].startswith("LPCM24")
    while True:
        n = (2 * left) // (5 * ch) if lp20 else left // (3 * ch) if lp24 else left // (a * ch)
        n = np.minimum(n, FRAME_SAMPLES)
        if not n.any():
            return frames, written, consumed
        used = (n * 5 * ch) // 2 if lp20 else n * 3 * ch if lp24 else n * a * ch
        frames += n
        written += (n * ch) // g * g  # (g is 1 but for the LPCM codecs; the mono forms have ch 1: P:247, 314)
        consumed += used
        left -= used


def expected(c, ch, data):
    """what the library must write, from `upstream`: the reported samples of every chunk, zeros where the pattern stayed
    (departure 2), IEEE values outside the domain (departure 3); and the count"""
    chunks, _, count = upstream(c, ch, data, outside="ieee")
    out = np.frombuffer(b"".join(f for _, f in chunks), np.uint8).copy()
    if c in LPCM:  # a written sample's low byte is 0: the pattern marks exactly the samples that were not written
        w = out.view("<u4")
        w[w == int.from_bytes(bytes([PATTERN] * 4), "little")] = 0
    return out, count


# ------------------------------------------------------------------ the same in numpy, with the three departures
def layout(c, ch, length):
    """(frames, samples upstream writes, bytes consumed, output bytes) in closed form"""
    a, _, g = GROUPS[c]
    if CODECS[c].startswith("LPCM20"):
        frames = 2 * length // (5 * ch)
        consumed = 5 * frames * ch // 2
    elif CODECS[c].startswith("LPCM24"):
        frames = length // (3 * ch)
        consumed = 3 * frames * ch
    else:
        frames = length // (a * ch)
        consumed = frames * ch * a
    return frames, frames * ch // g * g, consumed, frames * ch * sample_bytes(c)


def decode(c, ch, data):
    """(the output bytes, the samples outside the float domain)"""
    data = np.frombuffer(bytes(data), np.uint8)
    frames, written, _, out_bytes = layout(c, ch, data.size)
    a, b, g = GROUPS[c]
    name = CODECS[c]
    s = data[:written // g * a].reshape(-1, a).astype(np.uint32)
    count = 0
    if name in ("COPY8", "COPY16", "COPY32"):
        out = s.astype(np.uint8)
    elif name in ("SWAP16", "SWAP32"):
        out = s[:, ::-1].astype(np.uint8)
    elif name == "S24LE":
        out = (s[:, 0] << 8 | s[:, 1] << 16 | s[:, 2] << 24).astype("<u4")
    elif name == "S24BE":
        out = (s[:, 2] << 8 | s[:, 1] << 16 | s[:, 0] << 24).astype("<u4")
    elif name in ("LPCM24", "LPCM24_MONO"):
        k = g
        out = np.stack([s[:, 2 * i] << 24 | s[:, 2 * i + 1] << 16 | s[:, 2 * k + i] << 8 for i in range(k)], 1).astype("<u4")
    elif name in ("LPCM20", "LPCM20_MONO"):
        k = g
        low = [(s[:, 2 * k + i // 2] & 0xF0) << 8 if i % 2 == 0 else (s[:, 2 * k + i // 2] & 0x0F) << 12 for i in range(k)]
        out = np.stack([s[:, 2 * i] << 24 | s[:, 2 * i + 1] << 16 | low[i] for i in range(k)], 1).astype("<u4")
    elif name in ("F32LE", "F32BE"):
        v = np.ascontiguousarray(s.astype(np.uint8)).view(">u4" if name == "F32BE" else "<u4").astype(np.uint32).ravel()
        e, m = (v >> 23) & 0xFF, v & 0x7FFFFF
        out = np.where(e != 0, v, np.where(m != 0, (v & 0x80000000) | 0x3F800000 | m, 0)).astype("<u4")
        count = int(((e != 0) & ((e < 97) | (e > 157))).sum())
    elif name in ("F64LE", "F64BE"):
        v = np.ascontiguousarray(s.astype(np.uint8)).view(">u8" if name == "F64BE" else "<u8").astype(np.uint64).ravel()
        e, zero = (v >> np.uint64(52)) & np.uint64(0x7FF), (v << np.uint64(1)) == 0
        out = np.where(zero, np.uint64(0), v).astype("<u8")
        count = int((~zero & ((e < 993) | (e > 1053))).sum())
    else:
        out = (ULAW if name == "ULAW" else ALAW)[s[:, 0]].astype("<i2")
    out = np.ascontiguousarray(out).view(np.uint8).ravel()
    return np.concatenate([out, np.zeros(out_bytes - out.size, np.uint8)]), count


# ------------------------------------------------------------------ content
def content(c, nbytes, seed):
    """nbytes of a packet of codec c from a seed: any bytes, but for the float codecs samples of the defined domain (every
    exponent field of it, zeros and float denormals among them), so that upstream's functions run without undefined
    behaviour; a tail under a sample is noise"""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, nbytes, dtype=np.uint8)
    if c not in FLOATS:
        return raw.tobytes()
    a = GROUPS[c][0]
    n = nbytes // a
    big = CODECS[c].endswith("BE")
    kind = rng.integers(0, 16, n)
    if a == 4:
        v = (rng.integers(97, 158, n).astype(np.uint32) << 23) | rng.integers(0, 1 << 23, n).astype(np.uint32)
        v = np.where(kind == 0, 0, np.where(kind == 1, rng.integers(1, 1 << 23, n).astype(np.uint32), v))
        v = (v | (rng.integers(0, 2, n).astype(np.uint32) << 31)).astype(">u4" if big else "<u4")
    else:
        v = (rng.integers(993, 1054, n).astype(np.uint64) << np.uint64(52)) | rng.integers(0, 1 << 52, n).astype(np.uint64)
        v = np.where(kind == 0, np.uint64(0), v)
        v = (v | (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63))).astype(">u8" if big else "<u8")
    return v.tobytes() + raw[n * a:].tobytes()


def float_edges(c, fields, mantissas=None):
    """one sample for every (exponent field, mantissa, sign) of codec c, a float codec, as packet bytes"""
    a = GROUPS[c][0]
    big = CODECS[c].endswith("BE")
    bits = 23 if a == 4 else 52
    mantissas = (0, 1, (1 << bits) - 1) if mantissas is None else mantissas
    out = []
    for e in fields:
        for m in mantissas:
            for sign in (0, 1):
                out.append((sign << (8 * a - 1) | e << bits | m).to_bytes(a, "big" if big else "little"))
    return b"".join(out)


# ------------------------------------------------------------------ init_pcm (P:810-1236) and get_packet (P:787-808)
def fourcc(name):
    if isinstance(name, int):
        return name
    x = name.encode("latin-1")
    return x[0] << 24 | x[1] << 16 | x[2] << 8 | x[3]


def payload(length, duration, block_align):
    """P:800-804"""
    bytes_in_packet = length
    if duration > 0 and duration * block_align < bytes_in_packet:
        bytes_in_packet = duration * block_align
    return bytes_in_packet


def init_pcm(fcc, bits, ch, endianess, header):
    """(function name, sample_format label, block_align), "RETURN0" where init_pcm returns 0, or ("NULL", ...) where it
    goes on without a decode_func.  header: the codec header's bytes"""
    f, label, align = "NULL", None, 0
    little = endianess == 2
    if fcc in ("twos", "aiff"):
        if bits <= 8:
            f, label = "decode_8", "S8"
        elif bits <= 16:
            f, label = "decode_s_16_swap", "S16"
        elif bits <= 24:
            f, label = "decode_s_24_be", "S32"
        elif bits <= 32:
            f, label = "decode_s_32_swap", "S32"
        else:
            return "RETURN0"
    elif fcc in (0x01, "PCM "):
        if bits <= 8:
            f, label = "decode_8", "U8"
        elif bits <= 16:
            f, label = "decode_s_16", "U16" if fcc == "PCM " else "S16"
        elif bits <= 24:
            f, label = "decode_s_24_le", "S32"
        elif bits <= 32:
            f, label = "decode_s_32", "S32"
    elif fcc in ("raw ", "sowt", "RAWA"):
        if bits == 8:
            f, label = "decode_8", "S8" if fcc == "sowt" else "U8"
        elif bits == 16:
            f, label = "decode_s_16", "S16"
        elif bits == 24:
            f, label = "decode_s_24_le", "S32"
        elif bits == 32:
            f, label = "decode_s_32", "S32"
        else:
            return "RETURN0"
    elif fcc == "LPCM":
        if bits == 16:
            f, label = "decode_s_16_swap", "S16"
        elif bits == 20:
            f, label = "decode_s_20_lpcm_mono" if ch == 1 else "decode_s_20_lpcm", "S32"
        elif bits == 24:
            f, label = "decode_s_24_lpcm_mono" if ch == 1 else "decode_s_24_lpcm", "S32"
        else:
            return "RETURN0"
    elif fcc == "in24":
        f, label, align = "decode_s_24_le" if little else "decode_s_24_be", "S32", ch * 3
    elif fcc == "in32":
        f, label, align = "decode_s_32" if little else "decode_s_32_swap", "S32", ch * 4
    elif fcc == 0x03:
        if bits == 32:
            f, label = "decode_float_32_le", "FLOAT"
        elif bits == 64:
            f, label = "decode_float_64_le", "DOUBLE"
        else:
            return "RETURN0"
    elif fcc == "fl32":
        f, label, align = "decode_float_32_le" if little else "decode_float_32_be", "FLOAT", ch * 4
    elif fcc == "fl64":
        f, label, align = "decode_float_64_le" if little else "decode_float_64_be", "DOUBLE", ch * 8
    elif fcc in ("ulaw", "ULAW", 0x07):
        f, label, align = "decode_ulaw", "S16", ch
    elif fcc in ("alaw", "ALAW", 0x06):
        f, label, align = "decode_alaw", "S16", ch
    elif fcc == "lpcm":
        if len(header) < 4:
            return "RETURN0"
        flags = int.from_bytes(header[:4], "little")
        big = bool(flags & 2)
        if flags & 1:
            if bits == 32:
                f, label, align = "decode_float_32_be" if big else "decode_float_32_le", "FLOAT", ch * 4
            elif bits == 64:
                f, label, align = "decode_float_64_be" if big else "decode_float_64_le", "DOUBLE", ch * 8
        else:
            if bits == 16:
                f, label, align = "decode_s_16_swap" if big else "decode_s_16", "S16", ch * 2
            elif bits == 24:
                f, label, align = "decode_s_24_be" if big else "decode_s_24_le", "S32", ch * 3
            elif bits == 32:
                f, label, align = "decode_s_32_swap" if big else "decode_s_32", "S32", ch * 4
    else:
        return "RETURN0"
    if not align:
        align = ch * ((bits + 7) // 8)
    return f, label, align
