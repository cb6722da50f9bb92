"""The statement of the GSM 06.10 decoder (tests/gsmraw.py) against results recorded from upstream's own lib/GSM610/
(tests/golden/gsm_vectors.json), and the host side of libmi_gsm.so (mi_gsm_explode, the tables and the chain of
csrc/gsm_format.h, through tests/harness/gsm_explode_san.cpp built plain) against the statement.  No GPU."""
import ctypes as C
import hashlib
import importlib
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gsmraw as G
from pkg import ROOT
from test_ctypes_signatures_cpu import ctypes_kind, prototypes

gsm = importlib.import_module("gmerlin-avdecoder_amd.gsm")

VECTORS = json.load(open(os.path.join(ROOT, "tests", "golden", "gsm_vectors.json")))["vectors"]
SHORT = [v for v in VECTORS if "pcm" in v]
LONG = [v for v in VECTORS if "pcm" not in v]


def state_words(v):
    s = v["state"]
    return s["dp"] + s["v"] + [s["msr"], s["nrp"]] + s["LARpp"] + [0] * 5


def sha_per_100(pcm):
    pcm = pcm.reshape(-1, 160)
    return [hashlib.sha256(pcm[i:i + 100].astype("<i2").tobytes()).hexdigest() for i in range(0, pcm.shape[0], 100)]


def check_against_vector(v, pcm, words, bad):
    assert [int(x) for x in words] == state_words(v), v["name"] + ": the state"
    pcm = np.asarray(pcm, np.int16).reshape(-1, 160)
    assert pcm.shape[0] == v["frames"]
    if "pcm" in v:
        want = np.frombuffer(bytes.fromhex(v["pcm"]), "<i2").reshape(-1, 160)
        for i in range(want.shape[0]):
            if i in v["not_compared"]:  # upstream hands on a buffer of its caller's: departure 1 writes zeros
                assert not pcm[i].any()
            else:
                assert np.array_equal(pcm[i], want[i]), f"{v['name']}: frame {i}"
        assert bad == len(v["not_compared"])
    else:
        assert sha_per_100(pcm) == v["sha256_per_100_frames"], v["name"]
        assert bad == 0


# ------------------------------------------------------------------ the statement against upstream's recorded results
@pytest.mark.parametrize("v", VECTORS, ids=[v["name"] for v in VECTORS])
def test_the_statement_against_upstream_s_recorded_results(v):
    pcm, S, bad = G.decode_stream(bytes.fromhex(v["input"]), v["fmt"])
    check_against_vector(v, pcm, S.words(), bad)


def test_the_vectors_are_the_issue_s():
    names = {v["name"] for v in VECTORS}
    assert {"speech_plain", "speech_ms", "nc_fallback_fmt0", "nc_fallback_fmt1", "xmaxc_all_fmt0", "xmaxc_all_fmt1", "larc_ends",
            "rails", "bad_magic", "random600", "speech200"} <= names
    by = {v["name"]: v for v in VECTORS}
    assert by["random600"]["frames"] == 600 and by["speech200"]["frames"] == 200 and len(by["random600"]["sha256_per_100_frames"]) == 6
    assert by["bad_magic"]["not_compared"] == [2] and len(bytes.fromhex(by["bad_magic"]["input"])) == 5 * 33 + 7
    p = [G.explode(bytes.fromhex(by["xmaxc_all_fmt0"]["input"])[k:k + 33], 0) for k in range(0, 16 * 33, 33)]
    assert sorted(f[11 + 17 * j] for f in p for j in range(4)) == list(range(64))
    first = G.explode(bytes.fromhex(by["nc_fallback_fmt0"]["input"])[:33], 0)
    assert first[8] < 40 and first[8 + 17] > 120  # the fallback as the first subframe of a fresh state
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "gsm_vectors.json")) < 1 << 20


# ------------------------------------------------------------------ the packer and the unpacker
@pytest.mark.parametrize("fmt", (0, 1))
def test_implode_and_explode_are_inverses(fmt):
    rng = np.random.default_rng(5 + fmt)
    for _ in range(200):
        p = G.random_params(rng, fmt)
        b = G.implode(p, fmt)
        assert len(b) == G.unit_bytes(fmt) and G.explode(b, fmt) == p
    for _ in range(200):
        b = bytes(rng.integers(0, 256, G.unit_bytes(fmt), dtype=np.uint8))
        if fmt == 0:
            b = bytes([0xD0 | b[0] & 15]) + b[1:]
            assert G.implode(G.explode(b, fmt), fmt) == b
        else:
            assert G.implode(G.explode(b, fmt), fmt) == b
    if fmt == 0:
        assert G.explode(bytes([0x70]) + bytes(32), 0) is None


@pytest.mark.parametrize("fmt", (0, 1))
def test_mi_gsm_explode_against_the_statement(fmt):
    units = [bytes.fromhex(v["input"]) for v in VECTORS if v["fmt"] == fmt]
    size = G.unit_bytes(fmt)
    seen = 0
    for data in units:
        for at in range(0, len(data) - size + 1, size):
            assert gsm.explode(np.frombuffer(data[at:at + size], np.uint8), fmt) == G.explode(data[at:at + size], fmt)
            seen += 1
    assert seen > 150
    one = bytearray(units[0][:size])
    for bit in range(8 * size):  # every single-bit flip of one unit, the magic's included
        b = bytearray(one)
        b[bit >> 3] ^= 1 << (bit & 7)
        assert gsm.explode(np.frombuffer(bytes(b), np.uint8), fmt) == G.explode(bytes(b), fmt), bit
    with pytest.raises(gsm.MiGsmError):
        gsm.explode(np.zeros(size + 1, np.uint8), fmt)


# ------------------------------------------------------------------ csrc/gsm_format.h on the CPU
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/harness/gsm_explode_san.cpp")
    exe = str(tmp_path_factory.mktemp("gsm") / "gsm_harness")
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "harness", "gsm_explode_san.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stdout + r.stderr
    return exe


def test_the_two_tables_against_the_statement(harness):
    out = subprocess.run([harness, "tables"], capture_output=True, text=True, check=True).stdout.split()
    got = [int(x) for x in out]
    assert len(got) == 1024
    G.COUNTS.clear()
    assert got[:512] == [x for row in G.xmp_table() for x in row]
    assert got[512:] == [x for row in G.larpp_table() for x in row]
    # over all of both tables no GSM_ADD or GSM_SUB saturates and no shift leaves its plain arm but gsm_asl(1, -1): the
    # kernel's tables hold plain sums
    assert {k for k in G.COUNTS if k[-1] in "+-" or k.startswith(("asr", "asl"))} == {"asr", "asl", "asl<0"}


@pytest.mark.parametrize("v", VECTORS, ids=[v["name"] for v in VECTORS])
def test_the_chain_of_gsm_format_h_against_upstream_s_recorded_results(harness, v):
    out = subprocess.run([harness, "decode", str(v["fmt"])], input=bytes.fromhex(v["input"]), capture_output=True, check=True).stdout.split()
    got = np.array([int(x) for x in out])
    n = v["frames"] * 160
    assert got.size == n + G.STATE_WORDS + 1
    check_against_vector(v, got[:n], got[n:n + G.STATE_WORDS], int(got[-1]))


# ------------------------------------------------------------------ the dead branch, the census, the carry
def test_larp_to_rp_never_returns_min_word():
    """departure 2: the lattice's arm for -32768 times -32768 needs rrp[i] == -32768"""
    rp = [G.larp_to_rp_one(x, count=False) for x in range(-32768, 32768)]
    assert min(rp) == -32767 and max(rp) == 32767
    assert rp[0] == -32767 and rp[32768] == 0  # LARp -32768 and 0


# counters no decode can reach, each with its proof
UNREACHABLE = {
    "lattice MIN*MIN": "rrp[i] is a result of LARp_to_rp, which is never -32768 (test_larp_to_rp_never_returns_min_word)",
    "LARp==MIN_WORD": "LARp is a sum of shifted LARpp, |LARpp| <= 26214 over the whole table (below)",
    "interp+": "the same bound: a/4 + b/4 + a/2 stays within 26214 + 2", "interp-": "the same bound",
    "apcm add+": "over all 64 x 8 entries (test_the_two_tables_against_the_statement)", "apcm add-": "the same",
    "lar mic+": "over all 8 x 64 entries", "lar mic-": "the same", "lar sub+": "the same", "lar sub-": "the same",
    "lar double+": "the same", "lar double-": "the same",
    "asr>=16": "gsm_asr's n is 6 - expon, 0..10", "asr<=-16": "the same", "asr<0": "the same",
    "asl>=16": "gsm_asl's n is 5 - expon, -1..9", "asl<=-16": "the same",
}
REACHABLE = (["Mc %d" % k for k in range(4)] + ["bc %d" % k for k in range(4)] + ["mant shifts %d" % k for k in range(4)] +
             ["Nc in range", "Nc<40", "Nc>120", "mant==0", "asr", "asl", "asl<0", "bad magic", "tail dropped"] +
             ["rp segment %d%s" % (k, s) for k in range(3) for s in "+-"] +
             [site + rail for site in ("ltp add", "lattice sub", "lattice add", "deemphasis", "upscale") for rail in "+-"])


def test_the_vectors_take_every_branch_of_the_statement():
    G.COUNTS.clear()
    for v in SHORT:
        G.decode_stream(bytes.fromhex(v["input"]), v["fmt"])
    short = set(G.COUNTS)
    assert short == set(REACHABLE), (sorted(set(REACHABLE) - short), sorted(short - set(REACHABLE)))
    assert not short & set(UNREACHABLE)
    # every name the statement can count is in one of the two lists
    names = set(re.findall(r'COUNTS\["([^"%]+)"\]', open(os.path.join(ROOT, "tests", "gsmraw.py")).read()))
    assert names <= set(REACHABLE) | set(UNREACHABLE)
    sites = set(re.findall(r'GSM_(?:ADD|SUB)\([^"]*"([^"]+)"\)', open(os.path.join(ROOT, "tests", "gsmraw.py")).read()))
    assert {s + r for s in sites for r in "+-"} <= set(REACHABLE) | set(UNREACHABLE)
    bound = max(abs(x) for row in G.larpp_table() for x in row)
    assert bound == 26214 and (bound >> 2) + (bound >> 2) + (bound >> 1) + 2 < 32767


@pytest.mark.parametrize("fmt", (0, 1))
def test_five_units_equal_two_and_three(fmt):
    v = [x for x in SHORT if x["fmt"] == fmt and x["frames"] >> fmt >= 5 and not x["not_compared"]][0]
    size = G.unit_bytes(fmt)
    data = bytes.fromhex(v["input"])[:5 * size]
    whole, S, _ = G.decode_stream(data, fmt)
    a, Sa, _ = G.decode_stream(data[:2 * size], fmt)
    carried = G.State.from_words(Sa.words())  # through the 144 words
    b, Sb, _ = G.decode_stream(data[2 * size:], fmt, carried)
    assert np.array_equal(np.concatenate([a, b]), whole) and np.array_equal(Sb.words(), S.words())
    fresh, _, _ = G.decode_stream(data[2 * size:], fmt)
    assert not np.array_equal(fresh, b)  # (the state matters)
    assert Sa.words().size == G.STATE_WORDS and Sa.words().nbytes == gsm.STATE_BYTES


# ------------------------------------------------------------------ the library and its table
def test_library_exports_exactly_the_declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "mi_gsm.h")).read()
    declared = sorted(set(re.findall(r"\b(mi_gsm_[a-z0-9_]+)\s*\(", hdr)))
    L = C.CDLL(gsm.lib_path())
    for name in declared:
        assert hasattr(L, name), name
    assert sorted(gsm.EXPORTS) == declared and len(declared) == 14
    out = subprocess.run(["nm", "-D", "--defined-only", gsm.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = sorted(line.split()[-1] for line in out.splitlines() if " T " in line and "mi_gsm" in line)
    assert exported == declared


def test_signature_table_matches_the_header():
    declared = prototypes("mi_gsm.h", "mi_gsm_")
    assert len(declared) == 14
    assert list(gsm.SIGNATURES) == list(declared), "the header's order"
    for name, (ret, args) in declared.items():
        restype, argtypes = gsm.SIGNATURES[name]
        assert len(argtypes) == len(args), name
        assert ctypes_kind(restype) == ret, name
        assert [ctypes_kind(t) for t in argtypes] == args, name


def test_the_constants_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "mi_gsm.h")).read()
    for name, value in (("FRAME_BYTES", 33), ("BLOCK_BYTES", 65), ("FRAME_SAMPLES", 160), ("PARAMS", 76), ("STATE_BYTES", 288)):
        assert re.search(r"MI_GSM_%s = %d\b" % (name, value), hdr) and getattr(gsm, name) == value
    assert "MI_GSM_MAX_STREAMS = 1 << 20" in hdr and "MI_GSM_MAX_UNITS = 1 << 24" in hdr
    assert gsm.MAX_STREAMS == 1 << 20 and gsm.MAX_UNITS == 1 << 24 and G.STATE_WORDS * 2 == gsm.STATE_BYTES
