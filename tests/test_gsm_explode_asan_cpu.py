"""The unpacker, the tables and the chain of libmi_gsm.so (csrc/gsm_format.h: the code mi_gsm_explode runs on the host and
k_gsm_decode on the device) under AddressSanitizer and UndefinedBehaviorSanitizer: tests/harness/gsm_explode_san.cpp is a
program of its own, built here with g++ and run as a child process; it unpacks seeded frames and blocks from heap blocks of
exactly 33 and 65 bytes, holds every field to a reader that takes a bit at a time, walks both tables and runs the chain,
with every index into the history checked.  Nothing is loaded into this process, and nothing runs on a GPU."""
import json
import os
import shutil
import subprocess

import pytest

from pkg import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/harness/gsm_explode_san.cpp")
    out = str(tmp_path_factory.mktemp("gsm_san") / "gsm_explode_san")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-Wextra", "-o", out,
                            os.path.join(ROOT, "tests", "harness", "gsm_explode_san.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    assert "warning" not in build.stderr, build.stderr
    return out


def test_the_unpacker_reads_no_byte_it_was_not_given(exe):
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, f"exit {run.returncode}\n{run.stdout}{run.stderr}"
    lines = run.stdout.split("\n")
    assert lines[:2] == ["frames 4000", "blocks 4000"] and lines[2].startswith("tables ") and lines[3:] == ["chain 600", "ok", ""]


def test_the_chain_over_a_recorded_stream_under_the_sanitizers(exe):
    """a stream that reaches both rails everywhere, from a heap block of exactly its length; what it gives is held to
    upstream in tests/test_gsmraw_cpu.py, here it only has to run clean"""
    vectors = json.load(open(os.path.join(ROOT, "tests", "golden", "gsm_vectors.json")))["vectors"]
    for name in ("rails", "rails_ms", "bad_magic"):
        v = [x for x in vectors if x["name"] == name][0]
        run = subprocess.run([exe, "decode", str(v["fmt"])], input=bytes.fromhex(v["input"]), capture_output=True, timeout=120)
        assert run.returncode == 0, f"{name}: exit {run.returncode}\n{run.stderr.decode()}"
        assert len(run.stdout.split()) == v["frames"] * 160 + 144 + 1
