"""Targa packets of fourcc 'tga ' as upstream decodes them: a restatement of lib/video_tga.c (V below) over lib/targa.c (T),
the checker of libmi_tga.so (include/mi_tga.h).  Pinned by statement plus the seven vectors recorded from upstream's own
lib/targa.c (tests/golden/tga_vectors.json): nothing holds this file to a build of the two upstream files.

It is written from the upstream lines cited at every function and from nothing in csrc/, and states the decoder twice:

  decode(packet, palette, expect)       upstream's loops one for one: memread with its pointer and its remaining length,
                                        the run-length loop with p_loaded and pos, the unmap loop from the last pixel
                                        down, the swap loop with its bound, the row and column copies
  decode_fast(packet, palette, expect)  vectorised numpy: the packets as np.repeat over a gather index, the map as a fancy
                                        index, the swap and the flips as slices

Both return (status, picture, info): the status of include/mi_tga.h, the tight picture's bytes (uint8, rows of
w * bytes_per_pixel, top row first; None unless the status is 0), and parse()'s Info.  `expect` is (w, h, format) of the
call, or None: a packet that parses and differs is MISMATCH.  Where upstream's result is uninitialised memory the
statement refuses as the library does: SHORT (T:398 leaves the loop with the stream empty and the picture not full) and
BELOW_ORIGIN (T:322-328 leaves the map's bytes below its origin unwritten); INDEX_RANGE goes before BELOW_ORIGIN, since
upstream's unmap loop returns it whatever else the picture holds.

  parse(packet, palette_entries)  T:239-329 up to the image data: Info, with status 0 or the first refusal in upstream's order
  layout(fmt, w, h)               Layout of a picture
  header(...), packet(...)        builders: the 18 bytes; header + id + map + data
  rle(pixels, packets)            run-length data from stored pixels and an explicit list of (kind, count)
  greedy(pixels)                  the (kind, count) list of a greedy encoder: runs of two or more, raw otherwise
  random_packet(rng, ...)         a whole random packet of a type, size, depth and orientation
  random_palette(rng, entries)    (entries, 4) uint16 whose high and low bytes differ"""
import collections

import numpy as np

FORMATS = ("GRAY8", "RGB15", "BGR24", "RGBA32")
OK, EOF, CMAP_TYPE, IMG_TYPE, NO_IMG, CMAP_MISSING, CMAP_LENGTH, CMAP_DEPTH, ZERO_SIZE, PIXEL_DEPTH, RLE, INDEX_RANGE = \
    0, 2, 4, 5, 6, 7, 9, 10, 11, 12, 15, 16
SHORT, BELOW_ORIGIN, MISMATCH = 32, 33, 34
T_TO_B, R_TO_L = 0x20, 0x10  # targa.h:117-118
Info = collections.namedtuple("Info", "status data_offset map_offset map_origin map_length x_origin y_origin width height id_length "
                              "map_type image_type map_depth pixel_depth descriptor format bytes_per_pixel rle mapped flip_x flip_y "
                              "from_palette")
Layout = collections.namedtuple("Layout", "picture_bytes bytes_per_pixel row_bytes")
LIMIT = 1 << 31


def layout(fmt, w, h):
    bpp = (FORMATS.index(fmt) if isinstance(fmt, str) else fmt) + 1  # V:53-77
    if not (1 <= w <= 65535 and 1 <= h <= 65535) or w * h * bpp >= LIMIT:
        raise ValueError(f"{fmt} at {w} x {h}: width and height are 1 to 65535, pictures stay below 2^31 bytes")
    return Layout(w * h * bpp, bpp, w * bpp)


class _Reader:
    """struct read_struct and memread, T:197-216"""

    def __init__(self, buf):
        self.buf, self.ptr, self.len = bytes(buf), 0, len(buf)

    def read(self, n):
        """(the bytes memread copies, what it returns)"""
        if not self.len:
            return b"", 0
        if n > self.len:
            out = self.buf[self.ptr:self.ptr + self.len]
            ret, self.len = self.len, 0
            return out, ret
        out = self.buf[self.ptr:self.ptr + n]
        self.ptr += n
        self.len -= n
        return out, n


class _Barf(Exception):
    pass


def _read(s, n):  # READ, T:224-225
    out, got = s.read(n)
    if got < n:
        raise _Barf(EOF)
    return out


def _read16(s):  # READ16, T:227-229
    b = _read(s, 2)
    return b[0] | b[1] << 8


def _is_mapped(t):
    return t in (1, 9)


def _is_rle(t):
    return t in (9, 10, 11)


def parse(packet, palette_entries=0):
    f = dict.fromkeys(Info._fields, 0)
    s = _Reader(packet)
    try:
        f["id_length"] = _read(s, 1)[0]                         # T:239
        f["map_type"] = _read(s, 1)[0]                          # T:240
        if f["map_type"] not in (0, 1):                         # T:241-243
            raise _Barf(CMAP_TYPE)
        f["image_type"] = _read(s, 1)[0]                        # T:245
        if f["image_type"] == 0:                                # T:246-247
            raise _Barf(NO_IMG)
        if f["image_type"] not in (1, 2, 3, 9, 10, 11):         # T:249-255
            raise _Barf(IMG_TYPE)
        f["map_origin"] = _read16(s)                            # T:262
        f["map_length"] = _read16(s)                            # T:263
        f["map_depth"] = _read(s, 1)[0]                         # T:264
        mapped = _is_mapped(f["image_type"])
        if mapped and f["map_type"] == 0:                       # T:267-287
            if f["map_length"]:
                f["map_type"] = 1
            elif not palette_entries:
                raise _Barf(CMAP_MISSING)
            else:
                f["map_origin"], f["map_length"], f["map_depth"] = 0, palette_entries & 0xffff, 32
                f["map_type"], f["from_palette"] = 1, 1
        if f["map_type"] == 1:                                  # T:289-296
            if f["map_length"] == 0 and mapped:
                raise _Barf(CMAP_LENGTH)
            if f["map_depth"] not in (16, 24, 32) and mapped:
                raise _Barf(CMAP_DEPTH)
        f["x_origin"] = _read16(s)                              # T:298-301
        f["y_origin"] = _read16(s)
        f["width"] = _read16(s)
        f["height"] = _read16(s)
        if f["width"] == 0 or f["height"] == 0:                 # T:303-304
            raise _Barf(ZERO_SIZE)
        f["pixel_depth"] = _read(s, 1)[0]                       # T:306-309
        if f["pixel_depth"] not in (8, 16, 24, 32) or (f["pixel_depth"] != 8 and mapped):
            raise _Barf(PIXEL_DEPTH)
        f["descriptor"] = _read(s, 1)[0]                        # T:311
        if f["id_length"] > 0:                                  # T:313-318
            _read(s, f["id_length"])
        if f["map_type"] == 1 and not f["from_palette"]:        # T:320-329
            f["map_offset"] = s.ptr
            _read(s, f["map_length"] * f["map_depth"] // 8)
    except _Barf as e:
        f["status"] = e.args[0]
        return Info(**f)
    f["data_offset"] = s.ptr
    depth = f["map_depth"] if mapped else f["pixel_depth"]       # V:170-183
    f["format"], f["bytes_per_pixel"] = depth // 8 - 1, depth // 8  # V:53-77
    f["rle"], f["mapped"] = int(_is_rle(f["image_type"])), int(mapped)
    f["flip_x"] = int(bool(f["descriptor"] & R_TO_L))           # V:220-245
    f["flip_y"] = int(not f["descriptor"] & T_TO_B)
    return Info(**f)


def ctab(palette):
    """V:111-117: the caller's palette as the bytes upstream keeps"""
    return (np.asarray(palette, np.uint16) >> 8).astype(np.uint8).reshape(-1)


def _mismatch(info, expect):
    return expect is not None and (info.width, info.height, info.format) != (expect[0], expect[1], FORMATS.index(expect[2]) if isinstance(expect[2], str) else expect[2])


def decode(packet, palette=None, expect=None):
    packet = bytes(np.asarray(packet, np.uint8).tobytes())
    info = parse(packet, 0 if palette is None else len(palette))
    if info.status:
        return info.status, None, info
    if _mismatch(info, expect):
        return MISMATCH, None, info
    w, h, sb = info.width, info.height, info.pixel_depth // 8
    s = _Reader(packet)
    s.read(info.data_offset)
    p_expected = w * h
    image = bytearray(p_expected * sb)
    if info.rle:                                                # tga_read_rle, T:385-433
        p_loaded, pos = 0, 0
        while p_loaded < p_expected and s.len:
            b = _read(s, 1)[0]
            count = (b & 0x7f) + 1
            if b & 0x80:
                tmp, got = s.read(sb)
                if got < sb:
                    return EOF, None, info
                for _ in range(count):
                    p_loaded += 1
                    if p_loaded > p_expected:
                        return RLE, None, info
                    image[pos:pos + sb] = tmp
                    pos += sb
            else:
                if p_loaded + count > p_expected:
                    return RLE, None, info
                p_loaded += count
                raw, got = s.read(sb * count)
                if got < sb * count:
                    return EOF, None, info
                image[pos:pos + sb * count] = raw
                pos += count * sb
        if p_loaded < p_expected:
            return SHORT, None, info                            # (upstream: TGA_NOERR over malloc's bytes)
    else:                                                       # T:345-346
        raw, got = s.read(p_expected * sb)
        if got < p_expected * sb:
            return EOF, None, info
        image[:] = raw
    bpp = info.bytes_per_pixel
    if info.mapped:                                             # tga_color_unmap, T:875-912
        if info.from_palette:
            cmap = list(ctab(palette))                          # T:280-284
        else:
            first, size = info.map_origin * info.map_depth // 8, info.map_length * info.map_depth // 8
            cmap = [None] * first + list(packet[info.map_offset:info.map_offset + size])  # T:322-328
        out = bytearray(p_expected * bpp)
        below = False
        for pos in range(p_expected - 1, -1, -1):
            c = image[pos]
            if c >= info.map_origin + info.map_length:
                return INDEX_RANGE, None, info
            entry = cmap[c * bpp:c * bpp + bpp]
            if None in entry:
                below = True
                continue
            out[pos * bpp:pos * bpp + bpp] = bytes(entry)
        if below:
            return BELOW_ORIGIN, None, info                     # (upstream: bytes nobody wrote)
        image = out
    if bpp == 4:                                                # V:211-212, tga_swap_red_blue, T:1172-1188
        ptr = 0
        while ptr < (w * h - 1) * bpp:
            image[ptr], image[ptr + 2] = image[ptr + 2], image[ptr]
            ptr += bpp
    pic = bytearray(p_expected * bpp)                           # V:220-245
    for y in range(h):
        ys = y if info.descriptor & T_TO_B else h - 1 - y
        for x in range(w):
            xs = w - 1 - x if info.descriptor & R_TO_L else x
            pic[(y * w + x) * bpp:(y * w + x + 1) * bpp] = image[(ys * w + xs) * bpp:(ys * w + xs + 1) * bpp]
    return OK, np.frombuffer(bytes(pic), np.uint8), info


def walk(data, sb, npix):
    """the packets of run-length data as upstream's loop meets them: (status, [(run?, count, offset of the pixel bytes)])"""
    pos, loaded, out, n = 0, 0, [], len(data)
    while loaded < npix and pos < n:
        b = data[pos]
        pos += 1
        count = (b & 0x7f) + 1
        if b & 0x80:
            if n - pos < sb:
                return EOF, out
            if loaded + count > npix:
                return RLE, out
            out.append((True, count, pos))
            pos += sb
        else:
            if loaded + count > npix:
                return RLE, out
            if n - pos < sb * count:
                return EOF, out
            out.append((False, count, pos))
            pos += sb * count
        loaded += count
    return (SHORT if loaded < npix else OK), out


def decode_fast(packet, palette=None, expect=None):
    packet = np.ascontiguousarray(packet, np.uint8).reshape(-1)
    info = parse(packet.tobytes(), 0 if palette is None else len(palette))
    if info.status:
        return info.status, None, info
    if _mismatch(info, expect):
        return MISMATCH, None, info
    w, h, sb, bpp = info.width, info.height, info.pixel_depth // 8, info.bytes_per_pixel
    npix, data = w * h, packet[info.data_offset:]
    if info.rle:
        st, packets = walk(data.tobytes(), sb, npix)
        if st:
            return st, None, info
        runs = np.array([r for r, _, _ in packets], bool)
        counts = np.array([c for _, c, _ in packets], np.int64)
        starts = np.array([o for _, _, o in packets], np.int64)
        within = np.arange(npix) - np.repeat(np.cumsum(counts) - counts, counts)
        at = np.repeat(starts, counts) + np.where(np.repeat(runs, counts), 0, within * sb)
        stored = data[at[:, None] + np.arange(sb)]
    else:
        if data.size < npix * sb:
            return EOF, None, info
        stored = data[:npix * sb].reshape(npix, sb)
    if info.mapped:
        i = stored[:, 0].astype(np.int64)
        if (i >= info.map_origin + info.map_length).any():
            return INDEX_RANGE, None, info
        if info.from_palette:
            stored = ctab(palette).reshape(-1, 4)[i]
        else:
            if (i < info.map_origin).any():
                return BELOW_ORIGIN, None, info
            cmap = packet[info.map_offset:info.map_offset + info.map_length * bpp].reshape(-1, bpp)
            stored = cmap[i - info.map_origin]
    stored = stored.copy()
    if bpp == 4:
        stored[:-1, [0, 2]] = stored[:-1, [2, 0]]
    pic = stored.reshape(h, w, bpp)
    if info.flip_y:
        pic = pic[::-1]
    if info.flip_x:
        pic = pic[:, ::-1]
    return OK, np.ascontiguousarray(pic).reshape(-1), info


# ------------------------------------------------------------------ builders
def header(image_type, w, h, depth, descriptor=0, id_length=0, map_type=0, map_origin=0, map_length=0, map_depth=0, x_origin=0,
           y_origin=0):
    le = lambda v: [v & 0xff, v >> 8 & 0xff]  # noqa: E731
    return bytes([id_length, map_type, image_type] + le(map_origin) + le(map_length) + [map_depth] + le(x_origin) + le(y_origin)
                 + le(w) + le(h) + [depth, descriptor])


def packet(image_type, w, h, depth, data, descriptor=0, ident=b"", map_type=0, map_origin=0, map_length=0, map_depth=0, cmap=b"",
           trailing=b""):
    """header + id + map + data (+ trailing bytes) as a uint8 array; cmap: the map's bytes as they lie in the packet"""
    return np.frombuffer(header(image_type, w, h, depth, descriptor, len(ident), map_type, map_origin, map_length, map_depth)
                         + bytes(ident) + bytes(cmap) + bytes(data) + bytes(trailing), np.uint8)


def rle(pixels, packets):
    """pixels: (npix, sb) uint8 in stored order; packets: (kind, count) with kind "run" or "raw", count 1..128.  A run takes
    its pixel from the first of its pixels; the list may cover fewer or more pixels than there are (more: the last pixel
    repeats): the bad streams are built with it too"""
    pixels = np.asarray(pixels, np.uint8)
    out, p, last = bytearray(), 0, len(pixels) - 1
    for kind, count in packets:
        assert kind in ("run", "raw") and 1 <= count <= 128
        if kind == "run":
            out.append(0x80 | count - 1)
            out += pixels[min(p, last)].tobytes()
        else:
            out.append(count - 1)
            for k in range(count):
                out += pixels[min(p + k, last)].tobytes()
        p += count
    return bytes(out)


def greedy(pixels):
    """(kind, count) of a greedy encoder over stored pixels: two or more equal pixels make a run, the others go raw"""
    pixels = np.asarray(pixels, np.uint8)
    n = len(pixels)
    same = np.zeros(n, bool)
    same[1:] = (pixels[1:] == pixels[:-1]).all(axis=1)
    out, p = [], 0
    while p < n:
        q = p + 1
        while q < n and same[q] and q - p < 128:
            q += 1
        if q - p >= 2:
            out.append(("run", q - p))
        else:
            while q < n and q - p < 128 and not (q + 1 < n and same[q + 1]):
                q += 1
            out.append(("raw", q - p))
        p = q
    return out


def runs_of(pixels, packets):
    """pixels made to fit the packets: every pixel of a run is the run's first"""
    pixels = np.array(pixels, np.uint8)
    p = 0
    for kind, count in packets:
        if kind == "run":
            pixels[p:p + count] = pixels[p]
        p += count
    return pixels


def random_palette(rng, entries):
    hi = rng.integers(0, 256, (entries, 4))
    return (hi << 8 | (hi + 1 + rng.integers(0, 255, (entries, 4))) % 256).astype(np.uint16)


def random_packet(rng, image_type, w, h, depth, descriptor=0, map_depth=24, map_origin=0, map_length=None, ident=b"", packets=None,
                  from_palette=0, trailing=b""):
    """a good packet of the type: random pixels (stored indices inside the map for a mapped type; repeated in places for a
    run-length type, encoded greedily or by `packets`); from_palette: the entries of the caller's palette, and no map in the
    packet"""
    mapped, npix, sb = image_type in (1, 9), w * h, depth // 8
    kw = {}
    if mapped:
        if from_palette:
            lo, hi = 0, min(from_palette, 256)
        else:
            if map_length is None:
                map_length = int(rng.integers(1, 257 - map_origin))
            lo, hi = map_origin, min(map_origin + map_length, 256)
            kw = dict(map_type=1, map_origin=map_origin, map_length=map_length, map_depth=map_depth,
                      cmap=rng.integers(0, 256, map_length * map_depth // 8, dtype=np.uint8).tobytes())
        pixels = rng.integers(lo, hi, (npix, 1)).astype(np.uint8)
    else:
        pixels = rng.integers(0, 256, (npix, sb), dtype=np.uint8)
    if image_type in (9, 10, 11):
        if packets is None:
            hold = rng.integers(0, 3, npix) == 0  # a third of the pixels start a stretch of repeats
            src = np.maximum.accumulate(np.where(hold | (np.arange(npix) == 0), np.arange(npix), 0))
            pixels = pixels[src]
            packets = greedy(pixels)
        else:
            pixels = runs_of(pixels, packets)
        data = rle(pixels, packets)
    else:
        data = pixels.tobytes()
    return packet(image_type, w, h, depth, data, descriptor, ident, trailing=trailing, **kw)
