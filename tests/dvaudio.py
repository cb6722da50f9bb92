"""Statement of the DV sound on resident frames (k_dv_audio_extract, k_dv_audio_write: csrc/dv_audio_kernels.h).  TEST
INFRASTRUCTURE ONLY: the product never imports it.  numpy, no ctypes: the layout data are written out here, not read from
the library; tests/test_dv_audio_cpu.py holds this file to csrc/dvframe_host.c's mi_dv_extract_audio and to
np_extract_audio of tests/test_dvframe_host.py, and tests/test_gpu_dv_audio.py holds the kernels to this file, byte for byte.
extract() restates lib/dvframe.c:545-628 and is PINNED to that file where it is defined (tests/test_dvframe_reference_cpu.py,
tests/test_dvframe_fixtures_cpu.py); the AAUX packs that write() makes are this repository's reading of IEC 61834-4 and
stay UNPINNED."""
import numpy as np

PAIRS, PAIR_BYTES, SLOTS = 4, 8192, 4096
PACK_AT = 80 * 6 + 80 * 16 * 3 + 3  # the AAUX source pack: audio block 3 of sequence 0 of channel 0, behind its id
RATES = (48000, 44100, 32000)       # by the pack's rate field

# first slot of audio block j (column) of DIF sequence q (row); a slot is a 16-bit sample of an interleaved stereo pair
SHUFFLE_525 = np.array([
    [0, 30, 60, 20, 50, 80, 10, 40, 70], [6, 36, 66, 26, 56, 86, 16, 46, 76], [12, 42, 72, 2, 32, 62, 22, 52, 82],
    [18, 48, 78, 8, 38, 68, 28, 58, 88], [24, 54, 84, 14, 44, 74, 4, 34, 64], [1, 31, 61, 21, 51, 81, 11, 41, 71],
    [7, 37, 67, 27, 57, 87, 17, 47, 77], [13, 43, 73, 3, 33, 63, 23, 53, 83], [19, 49, 79, 9, 39, 69, 29, 59, 89],
    [25, 55, 85, 15, 45, 75, 5, 35, 65]], np.int64)
SHUFFLE_625 = np.array([
    [0, 36, 72, 26, 62, 98, 16, 52, 88], [6, 42, 78, 32, 68, 104, 22, 58, 94], [12, 48, 84, 2, 38, 74, 28, 64, 100],
    [18, 54, 90, 8, 44, 80, 34, 70, 106], [24, 60, 96, 14, 50, 86, 4, 40, 76], [30, 66, 102, 20, 56, 92, 10, 46, 82],
    [1, 37, 73, 27, 63, 99, 17, 53, 89], [7, 43, 79, 33, 69, 105, 23, 59, 95], [13, 49, 85, 3, 39, 75, 29, 65, 101],
    [19, 55, 91, 9, 45, 81, 35, 71, 107], [25, 61, 97, 15, 51, 87, 5, 41, 77], [31, 67, 103, 21, 57, 93, 11, 47, 83]], np.int64)


class Sound:
    """what the sound needs of a system: DIF sequences per channel, channels, the line system's table, stride, minimum
    samples per rate, and the frame rate as a fraction"""

    def __init__(self, system, seqs, chans):
        self.system, self.seqs, self.chans, self.dsf = system, seqs, chans, int(seqs == 12)
        self.frame_bytes = chans * seqs * 150 * 80
        self.shuffle = SHUFFLE_625 if self.dsf else SHUFFLE_525
        self.stride = 108 if self.dsf else 90
        self.min_samples = (1896, 1742, 1264) if self.dsf else (1580, 1452, 1053)
        self.fps = (25, 1) if self.dsf else (30000, 1001)
        self.capacity = seqs * 9 * 36 // 2  # samples per channel the blocks of a channel have room for (16-bit)
        self.stype = 2 if chans == 2 else 0  # what the source pack says: two pairs / one

    def block(self, c, q, j):
        """byte offset of audio block j of sequence q of channel c"""
        return ((c * self.seqs + q) * 150 + 6 + 16 * j) * 80


SOUND = {s.system: s for s in (Sound(0, 10, 1), Sound(1, 12, 1), Sound(3, 12, 1), Sound(4, 10, 2), Sound(5, 12, 2))}
SYSTEMS = tuple(SOUND)


def samples_of(system, rate, k):
    """samples per channel of frame k of an unlocked stream"""
    num, den = SOUND[system].fps
    return (k + 1) * rate * den // num - k * rate * den // num


def expand12(code):
    """12-bit non-linear codes -> 16 bits, 0x800 ("no sample") -> 0: magnitudes come in eight segments of 256 codes, the
    first two linear, segment k >= 2 2^(k-1) times as wide; negative codes are the one's complement of the positive law"""
    code = np.asarray(code, np.int64)
    neg = (code & 0x800) != 0
    m = np.where(neg, ~code & 0x7FF, code & 0x7FF)
    k = m >> 8
    v = np.where(k < 2, m, (m - 256 * np.maximum(k - 1, 0)) << np.maximum(k - 1, 0))
    v = np.where(neg, ~v, v) & 0xFFFF
    return np.where(code == 0x800, 0, v).astype(np.uint16)


def _payloads(s, frame, c, seqs):
    """the 72 sample bytes of the nine audio blocks of the given sequences of channel c: (len(seqs), 9, 72)"""
    at = np.array([[s.block(c, q, j) + 8 for j in range(9)] for q in seqs], np.int64)
    return frame[at[:, :, None] + np.arange(72)].astype(np.int64)


def extract(system, frame, pairs):
    """one frame -> (info, pcm): info = int32 (samples per channel | 0: no source pack | -1: unsupported quantisation or
    rate; then, where that is positive: rate, pairs the frame's blocks fill, bits — else zeros); pcm = uint8
    [pairs][PAIR_BYTES], what mi_dv_extract_audio writes into zeroed buffers (little-endian slots)"""
    s = SOUND[system]
    frame = np.asarray(frame, np.uint8)
    pcm = np.zeros((pairs, SLOTS), np.uint16)
    info = np.zeros(4, np.int32)
    as_ = frame[PACK_AT:PACK_AT + 5].astype(np.int64)
    if as_[0] != 0x50:
        return info, pcm.view(np.uint8)
    extra, freq, quant = int(as_[1]) & 0x3F, (int(as_[4]) >> 3) & 7, int(as_[4]) & 7
    if quant > 1 or freq > 2:
        info[0] = -1
        return info, pcm.view(np.uint8)
    samples = s.min_samples[freq] + extra
    limit, half = 2 * samples, s.seqs // 2
    info[:] = (samples, RATES[freq], s.chans * (2 if quant else 1), 12 if quant else 16)
    for k in range(pairs):
        if not quant:
            if k >= s.chans:
                continue
            b = _payloads(s, frame, k, range(s.seqs))
            v = b[:, :, 0::2] << 8 | b[:, :, 1::2]  # big-endian
            v = np.where(v == 0x8000, 0, v)
            slot = s.shuffle[:, :, None] + np.arange(36) * s.stride
            keep = slot < limit
            pcm[k, slot[keep]] = v[keep]
        else:
            c, h = k >> 1, k & 1
            if c >= s.chans:
                continue
            b = _payloads(s, frame, c, range(h * half, (h + 1) * half)).reshape(half, 9, 24, 3)
            left, right = b[..., 0] << 4 | b[..., 2] >> 4, b[..., 1] << 4 | (b[..., 2] & 0xF)
            slot_l = s.shuffle[:half, :, None] + np.arange(24) * s.stride
            slot_r = s.shuffle[half:, :, None] + np.arange(24) * s.stride
            keep = slot_l < limit  # the left slot alone decides for both
            pcm[k, slot_l[keep]] = expand12(left[keep])
            pcm[k, slot_r[keep]] = expand12(right[keep])
    return info, pcm.astype("<u2").view(np.uint8).reshape(pairs, PAIR_BYTES)


def aaux(system, q, j, samplerate, samples):
    """the five AAUX bytes of audio block j of sequence q (of either channel), as write() makes them.  Even sequences carry
    the packs 0x50 (source), 0x51 (source control), 0x52 (rec date), 0x53 (rec time) in blocks 3..6, odd ones in blocks
    0..3; every other block carries no pack (FF x 5).
      0x50: byte 1 = 1 (unlocked) 1 (reserved) | samples beyond the rate's minimum
            byte 2 = 0 in the first half of a channel's sequences, 1 in the second (stereo mode 0, which of the two
                     audio blocks of the channel this is; CHN 0: two channels a block)
            byte 3 = 1 1 (reserved, no multi-language) | DSF << 5 | stype (0: 25 Mbit/s, one pair; 2: 50 Mbit/s, two)
            byte 4 = 1 (no emphasis) 0 (time constant) | rate << 3 | quantisation 0 (16-bit linear)
      0x51: 3F (no copy protection information, input and compression fields all ones), CF (recording start and end
            marks off, mode: original), A0 (direction forward, speed field: normal), FF (no genre)
      0x52, 0x53: FF x 4 (no date, no time)"""
    s = SOUND[system]
    k = j if q & 1 else j - 3
    if k == 0:
        freq = RATES.index(samplerate)
        return [0x50, 0xC0 | (samples - s.min_samples[freq]), int(q >= s.seqs // 2), 0xC0 | s.dsf << 5 | s.stype, 0x80 | freq << 3]
    if k == 1:
        return [0x51, 0x3F, 0xCF, 0xA0, 0xFF]
    if k in (2, 3):
        return [0x50 + k, 0xFF, 0xFF, 0xFF, 0xFF]
    return [0xFF] * 5


def write(system, frame, pcm, samplerate, samples):
    """the frame with 16-bit sound in its audio blocks: pcm = [pairs >= the system's channels][PAIR_BYTES] bytes (or
    [..][SLOTS] int16), pair c to channel c.  Every audio block is rewritten whole — id (section type 3, sequence,
    channel, block number), AAUX pack, 36 big-endian samples: slot < 2 samples ? the sample (0x8000 -> 0x8001) : 0 — and no
    other byte"""
    s = SOUND[system]
    out = np.array(frame, np.uint8)
    pcm = np.ascontiguousarray(pcm).view(np.uint8).reshape(-1, PAIR_BYTES).view("<u2").astype(np.int64)
    assert pcm.shape[0] >= s.chans and s.min_samples[RATES.index(samplerate)] <= samples <= s.min_samples[RATES.index(samplerate)] + 63
    for c in range(s.chans):
        for q in range(s.seqs):
            for j in range(9):
                at = s.block(c, q, j)
                out[at:at + 3] = (0x7F, q << 4 | c << 3 | 7, j)
                out[at + 3:at + 8] = aaux(system, q, j, samplerate, samples)
                slot = s.shuffle[q, j] + np.arange(36) * s.stride
                v = np.where(slot < 2 * samples, pcm[c, slot], 0)
                v = np.where(v == 0x8000, 0x8001, v)
                out[at + 8:at + 80:2], out[at + 9:at + 80:2] = v >> 8, v & 0xFF
    return out


def audio_mask(system):
    """True at the bytes of a frame's audio blocks"""
    s = SOUND[system]
    m = np.zeros(s.frame_bytes, bool)
    for c in range(s.chans):
        for q in range(s.seqs):
            for j in range(9):
                m[s.block(c, q, j):s.block(c, q, j) + 80] = True
    return m


# ---- frames the tests share ----
def set_pack(frame, extra, freq, quant, stype=0):
    frame[PACK_AT:PACK_AT + 5] = (0x50, extra, 0, stype, freq << 3 | quant)
    return frame


def noise_frame(system, seed, extra, freq, quant):
    """random bytes that announce the system (DSF, APT, VAUX stype) and carry a source pack"""
    s = SOUND[system]
    f = np.random.default_rng(seed).integers(0, 256, s.frame_bytes, dtype=np.uint8)
    f[3] = (f[3] & 0x7F) | s.dsf << 7
    f[5] = (f[5] & 0xF8) | (0 if system in (0, 1) else 1)
    f[80 * 5 + 48 + 3] = (f[80 * 5 + 48 + 3] & 0xE0) | (4 if s.chans == 2 else 0)
    return set_pack(f, extra, freq, quant)


def fill_payloads(system, frame, pattern):
    """every audio block's 72 sample bytes = the pattern repeated (the packs stay)"""
    s = SOUND[system]
    pattern = np.asarray(pattern, np.uint8)
    for c in range(s.chans):
        for q in range(s.seqs):
            for j in range(9):
                frame[s.block(c, q, j) + 8:s.block(c, q, j) + 80] = np.resize(pattern, 72)
    return frame


def all_codes_frame(system, seed, extra):
    """a 12-bit frame at 32 kHz whose first 4096 byte triples hold every code 0..0xFFF once as the left sample (high byte,
    high nibble of the third) and once, in another order, as the right one (second byte, low nibble).  Only a 50 Mbit/s
    frame has room (4320 / 5184 triples; a 25 Mbit/s one has 2160 / 2592); with extra = 63 no triple is dropped"""
    s = SOUND[system]
    f = noise_frame(system, seed, extra, 2, 1)
    left = np.arange(4096)
    right = (left * 2731 + 1) & 0xFFF  # a permutation (2731 is odd)
    t = np.stack([left >> 4, right >> 4, (left & 0xF) << 4 | (right & 0xF)], 1).astype(np.uint8).ravel()
    room = s.chans * s.seqs * 9 * 72
    assert t.size <= room
    t, at = np.concatenate([t, np.zeros(room - t.size, np.uint8)]), 0
    for c in range(s.chans):
        for q in range(s.seqs):
            for j in range(9):
                f[s.block(c, q, j) + 8:s.block(c, q, j) + 80] = t[at:at + 72]
                at += 72
    return f
