"""The host forms of every transform of libmi_pcm.so (csrc/pcm_format.h: the code k_pcm_decode runs on the device) under
AddressSanitizer and UndefinedBehaviorSanitizer: tests/harness/pcm_format_san.cpp is a program of its own, built here with
g++ and run as a child process.  Every codec takes seeded packets of every length from 0 to past three pieces a channel
count, each from a heap block of exactly the packet's length into one of exactly the result's: the 3-, 5-, 6-, 10- and
12-byte group tails are what it is after.  Nothing is loaded into this process, and nothing runs on a GPU."""
import json
import os
import shutil
import subprocess

import pytest

import pcmraw as R
from pkg import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/harness/pcm_format_san.cpp")
    out = str(tmp_path_factory.mktemp("pcm_san") / "pcm_format_san")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-Wextra", "-o", out,
                            os.path.join(ROOT, "tests", "harness", "pcm_format_san.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    assert "warning" not in build.stderr, build.stderr
    return out


def test_every_transform_reads_and_writes_no_byte_it_was_not_given(exe):
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, f"exit {run.returncode}\n{run.stdout}{run.stderr}"
    lines = run.stdout.split("\n")
    assert lines[0].startswith("packets ") and int(lines[0].split()[1]) > 5000 and lines[2:] == ["ok", ""]


def test_the_recorded_vectors_under_the_sanitizers(exe):
    """the short recorded inputs, the floats' edges among them, from heap blocks of exactly their length; what they give is
    held to upstream in tests/test_pcmraw_cpu.py, here it only has to run clean, the classifiers and codec_of included"""
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "pcm_vectors.json")))
    for v in golden["vectors"]:
        if isinstance(v[2], str):
            c = R.codec(v[0])
            data = bytes.fromhex(v[2])
            run = subprocess.run([exe, "decode", str(c), str(v[1])], input=data, capture_output=True, timeout=120)
            assert run.returncode == 0, f"{v[:2]}: exit {run.returncode}\n{run.stderr.decode()}"
            assert len(run.stdout) == 4 + R.layout(c, v[1], len(data))[3]
    text = "".join("%d %d %d %d %d %d\n" % (R.fourcc(f), bits, ch, end, hlen, flags) for f, bits, ch, end, hlen, flags, _ in golden["init"])
    run = subprocess.run([exe, "codec_of"], input=text, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and len(run.stdout.split("\n")) == len(golden["init"]) + 1, run.stderr
