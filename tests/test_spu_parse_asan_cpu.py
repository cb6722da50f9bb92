"""The control parser of libmi_spu.so (csrc/spu_format.h: the code mi_spu_parse runs on the host and k_spu_scan on the device)
under AddressSanitizer and UndefinedBehaviorSanitizer: tests/harness/spu_parse_san.cpp is a program of its own, built here
with g++ and run as a child process; it parses every truncation of six packets from heap blocks of exactly their length,
every command byte in front of every count of operand bytes, control offsets that point anywhere, and noise.  Nothing is
loaded into this process, and nothing runs on a GPU."""
import os
import shutil
import subprocess

import pytest

from pkg import ROOT


def test_the_parser_reads_no_byte_it_was_not_given(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/harness/spu_parse_san.cpp")
    exe = str(tmp_path / "spu_parse_san")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-Wextra", "-o", exe,
                            os.path.join(ROOT, "tests", "harness", "spu_parse_san.cpp")], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    assert "warning" not in build.stderr, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, f"exit {run.returncode}\n{run.stdout}{run.stderr}"
    lines = run.stdout.split("\n")
    assert lines[-2] == "ok" and lines[0].startswith("truncations ") and int(lines[0].split()[1]) > 500
    assert lines[1] == "commands 4608" and lines[2].startswith("offsets ") and lines[3] == "noise 20000"
