"""The statement of the GSM 06.10 full-rate decoder as lib/audio_gsm.c (A) drives the vendored lib/GSM610/ (G): what
libmi_gsm.so (include/mi_gsm.h) is held to, byte for byte.  Pure Python integers; every function restates the cited lines
loop for loop, and tests/golden/gsm_vectors.json, recorded from upstream's own code, holds this file to upstream.

A frame's 76 parameters, in the order of the bit stream: LARc[8], then for each of the four subframes Nc, bc, Mc, xmaxc,
xMc[13].  A state is what survives a frame: dp[120] (upstream's dp0[0..119]), v[9], msr, nrp and the last LARpp[8].

COUNTS counts which way every branch of a decode went (census: tests/test_gsmraw_cpu.py).  A name that ends in "+" or "-"
is a saturating operation that reached that rail."""
import collections

import numpy as np

MIN_WORD, MAX_WORD = -32768, 32767
FRAME_BYTES, BLOCK_BYTES, FRAME_SAMPLES, MAGIC = 33, 65, 160, 0xD
WIDTHS = [6, 6, 5, 5, 4, 4, 3, 3] + ([7, 2, 2, 6] + [3] * 13) * 4  # G/gsm_decode.c:278-376, the same fields at :47-268
N_PARAMS = len(WIDTHS)
assert N_PARAMS == 76 and sum(WIDTHS) == 260
STATE_WORDS = 144  # dp[120], v[9], msr, nrp, LARpp[8], five zeros
QLB = (3277, 11469, 21299, 32767)  # G/table.c:67
FAC = (18431, 20479, 22527, 24575, 26623, 28671, 30719, 32767)  # G/table.c:85
# B, MIC, INVA of the STEPs at G/short_term.c:80-88
LAR_STEPS = ((0, -32, 13107), (0, -32, 13107), (2048, -16, 13107), (-2560, -16, 13107),
             (94, -8, 19223), (-1792, -8, 17476), (-341, -4, 31454), (-1144, -4, 29708))

COUNTS = collections.Counter()


# ------------------------------------------------------------------ G/gsm610_priv.h:84-191 and G/add.c
def word(x):
    """what an assignment to `word` keeps of x"""
    return ((x + 32768) & 0xFFFF) - 32768


def GSM_MULT_R(a, b):  # priv.h:123-126: does not saturate
    return (a * b + 16384) >> 15


def GSM_ADD(a, b, site):  # priv.h:155-167
    s = a + b
    if s > MAX_WORD:
        COUNTS[site + "+"] += 1
        return MAX_WORD
    if s < MIN_WORD:
        COUNTS[site + "-"] += 1
        return MIN_WORD
    return s


def GSM_SUB(a, b, site):  # priv.h:169-181
    return GSM_ADD(a, -b, site)


def gsm_sub(a, b):  # add.c:50-54
    return max(MIN_WORD, min(MAX_WORD, a - b))


def gsm_asr(a, n):  # add.c:184-191
    if n >= 16:
        COUNTS["asr>=16"] += 1
        return -(a < 0)
    if n <= -16:
        COUNTS["asr<=-16"] += 1
        return 0
    if n < 0:
        COUNTS["asr<0"] += 1
        return word(a << -n)
    COUNTS["asr"] += 1
    return a >> n


def gsm_asl(a, n):  # add.c:193-199
    if n >= 16:
        COUNTS["asl>=16"] += 1
        return 0
    if n <= -16:
        COUNTS["asl<=-16"] += 1
        return -(a < 0)
    if n < 0:
        COUNTS["asl<0"] += 1
        return gsm_asr(a, -n)
    COUNTS["asl"] += 1
    return word(a << n)


# ------------------------------------------------------------------ the two unpackers and their inverse
def explode(block, fmt):
    """the parameters of a 33-byte frame (fmt 0: 76) or a 65-byte block (fmt 1: 152), or None for a bad magic"""
    b = bytes(block)
    if fmt == 0:  # G/gsm_decode.c:276-376: most significant bit first, behind the nibble of the magic
        assert len(b) == FRAME_BYTES
        if (b[0] >> 4) & 0xF != MAGIC:
            return None
        bits = int.from_bytes(b, "big")
        out, pos = [], 8 * FRAME_BYTES - 4
        for w in WIDTHS:
            pos -= w
            out.append((bits >> pos) & ((1 << w) - 1))
        return out
    # G/gsm_decode.c:40-270: least significant bit first; the first frame ends in the low nibble of byte 32, the high one
    # is frame_chain, which the second call, at +33 (A:130-138), reads first: one stream of 520 bits
    assert len(b) == BLOCK_BYTES
    bits = int.from_bytes(b, "little")
    out, pos = [], 0
    for w in WIDTHS * 2:
        out.append((bits >> pos) & ((1 << w) - 1))
        pos += w
    return out


def implode(params, fmt):
    """the packer of the tests: 76 parameters to a 33-byte frame, 152 to a 65-byte block"""
    params = [int(p) for p in params]
    widths = WIDTHS * (1 + fmt)
    assert len(params) == len(widths) and all(0 <= p < 1 << w for p, w in zip(params, widths))
    if fmt == 0:
        bits = MAGIC
        for p, w in zip(params, widths):
            bits = bits << w | p
        return bits.to_bytes(FRAME_BYTES, "big")
    bits, pos = 0, 0
    for p, w in zip(params, widths):
        bits |= p << pos
        pos += w
    return bits.to_bytes(BLOCK_BYTES, "little")


def random_params(rng, fmt=0):
    return [int(rng.integers(0, 1 << w)) for w in WIDTHS * (1 + fmt)]


# ------------------------------------------------------------------ the state
class State:
    def __init__(self):  # gsm_create: zeros, nrp = 40
        self.dp = [0] * 120
        self.v = [0] * 9
        self.msr = 0
        self.nrp = 40
        self.LARpp = [0] * 8

    def words(self):
        """the 144 int16 of MI_GSM_STATE_BYTES"""
        return np.array(self.dp + self.v + [self.msr, self.nrp] + self.LARpp + [0] * 5, np.int16)

    @classmethod
    def from_words(cls, a):
        a = [int(x) for x in np.asarray(a, np.int16)]
        assert len(a) == STATE_WORDS
        s = cls()
        s.dp, s.v, s.msr, s.nrp, s.LARpp = a[:120], a[120:129], a[129], a[130], a[131:139]
        return s

    def copy(self):
        return State.from_words(self.words())


# ------------------------------------------------------------------ G/rpe.c
def xmaxc_to_exp_mant(xmaxc):  # rpe.c:244-275
    expon = 0
    if xmaxc > 15:
        expon = (xmaxc >> 3) - 1
    mant = xmaxc - (expon << 3)
    if mant == 0:
        COUNTS["mant==0"] += 1
        expon, mant = -4, 7
    else:
        n = 0
        while mant <= 7:
            mant = mant << 1 | 1
            expon -= 1
            n += 1
        COUNTS["mant shifts %d" % n] += 1
        mant -= 8
    assert -4 <= expon <= 6 and 0 <= mant <= 7
    return expon, mant


def apcm_inverse_quantization(xMc, mant, expon):  # rpe.c:369-402
    temp1 = FAC[mant]
    temp2 = gsm_sub(6, expon)
    temp3 = gsm_asl(1, gsm_sub(temp2, 1))
    xMp = []
    for i in range(13):
        temp = (xMc[i] << 1) - 7
        temp = word(temp << 12)
        temp = word(GSM_MULT_R(temp1, temp))
        temp = GSM_ADD(temp, temp3, "apcm add")
        xMp.append(gsm_asr(temp, temp2))
    return xMp


def rpe_grid_positioning(Mc, xMp):  # rpe.c:406-441: what the switch does is what its comment says
    ep = [0] * 40
    for i in range(13):
        ep[Mc + 3 * i] = xMp[i]
    COUNTS["Mc %d" % Mc] += 1
    return ep


def rpe_decoding(xmaxcr, Mcr, xMcr):  # rpe.c:490-506
    expon, mant = xmaxc_to_exp_mant(xmaxcr)
    return rpe_grid_positioning(Mcr, apcm_inverse_quantization(xMcr, mant, expon))


# ------------------------------------------------------------------ G/long_term.c:924-967
def long_term_synthesis(S, Ncr, bcr, erp, drp):
    """drp: list of 160, drp[120 + k] is upstream's drp[k]; the history moves 40 samples"""
    if Ncr < 40:
        COUNTS["Nc<40"] += 1
        Nr = S.nrp
    elif Ncr > 120:
        COUNTS["Nc>120"] += 1
        Nr = S.nrp
    else:
        COUNTS["Nc in range"] += 1
        Nr = Ncr
    S.nrp = Nr
    assert 40 <= Nr <= 120
    brp = QLB[bcr]
    COUNTS["bc %d" % bcr] += 1
    for k in range(40):
        drpp = word(GSM_MULT_R(brp, drp[120 + k - Nr]))
        drp[120 + k] = GSM_ADD(erp[k], drpp, "ltp add")
    out = drp[120:160]
    for k in range(120):
        drp[k] = drp[40 + k]
    return out


# ------------------------------------------------------------------ G/short_term.c
def decode_lar(i, c):  # one STEP of short_term.c:74-88
    B, MIC, INVA = LAR_STEPS[i]
    temp1 = word(GSM_ADD(c, MIC, "lar mic") << 10)
    temp1 = GSM_SUB(temp1, B << 1, "lar sub")
    temp1 = word(GSM_MULT_R(INVA, temp1))
    return GSM_ADD(temp1, temp1, "lar double")


def decode_lars(LARc):  # short_term.c:44-93
    return [decode_lar(i, c) for i, c in enumerate(LARc)]


def coefficients(which, prev, cur):  # short_term.c:111-157
    out = []
    for a, b in zip(prev, cur):
        if which == 0:  # 0..12
            t = GSM_ADD(a >> 2, b >> 2, "interp")
            t = GSM_ADD(t, a >> 1, "interp")
        elif which == 1:  # 13..26
            t = GSM_ADD(a >> 1, b >> 1, "interp")
        elif which == 2:  # 27..39
            t = GSM_ADD(a >> 2, b >> 2, "interp")
            t = GSM_ADD(t, b >> 1, "interp")
        else:  # 40..159
            t = b
        out.append(t)
    return out


def larp_to_rp_one(x, count=True):  # short_term.c:161-195
    if x < 0:
        if x == MIN_WORD:
            if count:
                COUNTS["LARp==MIN_WORD"] += 1
            temp = MAX_WORD
        else:
            temp = -x
        sign = "-"
    else:
        temp = x
        sign = "+"
    if temp < 11059:
        seg, r = 0, temp << 1
    elif temp < 20070:
        seg, r = 1, temp + 11059
    else:
        seg, r = 2, min(MAX_WORD, max(MIN_WORD, (temp >> 2) + 26112))  # GSM_ADD; both operands are positive
    if count:
        COUNTS["rp segment %d%s" % (seg, sign)] += 1
    return word(-r) if x < 0 else word(r)


def larp_to_rp(LARp):
    return [larp_to_rp_one(x) for x in LARp]


def short_term_synthesis_filtering(S, rrp, wt):  # short_term.c:280-318
    v, sr = S.v, []
    for sri in wt:
        for i in range(7, -1, -1):
            tmp1, tmp2 = rrp[i], v[i]
            if tmp1 == MIN_WORD and tmp2 == MIN_WORD:
                COUNTS["lattice MIN*MIN"] += 1
                tmp2 = MAX_WORD
            else:
                tmp2 = word(0xFFFF & ((tmp1 * tmp2 + 16384) >> 15))
            sri = GSM_SUB(sri, tmp2, "lattice sub")
            if tmp1 == MIN_WORD and sri == MIN_WORD:
                COUNTS["lattice MIN*MIN"] += 1
                tmp1 = MAX_WORD
            else:
                tmp1 = word(0xFFFF & ((tmp1 * sri + 16384) >> 15))
            v[i + 1] = GSM_ADD(v[i], tmp1, "lattice add")
        v[0] = sri
        sr.append(sri)
    return sr


def short_term_synthesis(S, LARcr, wt):  # short_term.c:402-443
    prev, cur = S.LARpp, decode_lars(LARcr)
    S.LARpp = cur
    s = []
    for which, (a, b) in enumerate(((0, 13), (13, 27), (27, 40), (40, 160))):
        s += short_term_synthesis_filtering(S, larp_to_rp(coefficients(which, prev, cur)), wt[a:b])
    return s


# ------------------------------------------------------------------ G/decode.c
def postprocessing(S, s):  # decode.c:40-54
    msr, out = S.msr, []
    for x in s:
        tmp = word(GSM_MULT_R(msr, 28180))
        msr = GSM_ADD(x, tmp, "deemphasis")
        out.append(word(GSM_ADD(msr, msr, "upscale") & 0xFFF8))
    S.msr = msr
    return out


def decode_frame(S, params):  # decode.c:56-83
    LARc = params[:8]
    drp, wt = S.dp + [0] * 40, []
    for j in range(4):
        Nc, bc, Mc, xmaxc = params[8 + 17 * j:12 + 17 * j]
        erp = rpe_decoding(xmaxc, Mc, params[12 + 17 * j:25 + 17 * j])
        wt += long_term_synthesis(S, Nc, bc, erp, drp)
    S.dp = drp[:120]
    return postprocessing(S, short_term_synthesis(S, LARc, wt))


# ------------------------------------------------------------------ A:105-145, with this library's two departures
def unit_bytes(fmt):
    return BLOCK_BYTES if fmt else FRAME_BYTES


def decode_stream(data, fmt, state=None):
    """(samples int16, the State after, the count of frames with a bad magic) of floor(len / 33) frames or floor(len / 65)
    blocks; a tail is dropped (A:118-126).  A frame with a bad magic leaves the state alone and gives 160 zeros."""
    data = bytes(data)
    S = State() if state is None else state
    size, pcm, bad = unit_bytes(fmt), [], 0
    for at in range(0, len(data) - size + 1, size):
        p = explode(data[at:at + size], fmt)
        if p is None:
            COUNTS["bad magic"] += 1
            bad += 1
            pcm += [0] * FRAME_SAMPLES
            continue
        for f in range(0, len(p), N_PARAMS):
            pcm += decode_frame(S, p[f:f + N_PARAMS])
    if len(data) % size:
        COUNTS["tail dropped"] += 1
    return np.array(pcm, np.int16), S, bad


# ------------------------------------------------------------------ the two tables of csrc/gsm_format.h
def xmp_table():
    """xMp by (xmaxc, xMc): 64 x 8"""
    return [[apcm_inverse_quantization([c] * 13, *reversed(xmaxc_to_exp_mant(x)))[0] for c in range(8)] for x in range(64)]


def larpp_table():
    """LARpp by (i, LARc): 8 x 64; 0 where LARc is beyond the field's width"""
    return [[decode_lar(i, c) if c < 1 << WIDTHS[i] else 0 for c in range(64)] for i in range(8)]
