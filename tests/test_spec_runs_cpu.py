"""The run list of the speculative index (csrc/rtj_spec_kernels.h: spec_packet_runs, spec_run_length), as the host makes
it when a plan is made: a small host program includes the header, builds the list for packets of given lengths exactly
as prepare_index does (a chunk per 2048 bytes and one more, the packets' chunks numbered through the plan) and prints it.

What the kernels need (read from spec_walk_body and k_spec_verify, not assumed): every chunk of the plan belongs to
exactly one run — the run walker is the only writer of the chunk's records — ; a run's chunks are consecutive chunks of ONE
packet, at most S of them; a packet's first run starts at its chunk 0 (byte 0: on the true chain); and only a packet's
last run is shorter than S."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import launch_shapes as LS

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CHUNK = 2048

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rtj_spec_kernels.h"
int main(int argc, char** argv) {
  using namespace mirtj;
  const uint32_t S = (uint32_t)atoi(argv[1]);
  printf("C %d %d %d %llu %llu\n", kSpecChunk, kSpecLead, kSpecRunMax, (unsigned long long)kSpecGeneration,
         (unsigned long long)kSpecRunMinGens);
  for (uint32_t s = 1; s <= (uint32_t)kSpecRunMax; s++) printf("T %u %u\n", s, spec_run_tiles(s));
  std::vector<SpecRunDev> runs;
  uint32_t base = 0;
  for (int i = 2; i < argc; i++) {
    const uint32_t len = (uint32_t)strtoul(argv[i], nullptr, 10);
    const uint32_t nsc = len / (uint32_t)kSpecChunk + 1u;  // prepare_index: spec_chunks_of
    spec_packet_runs((uint32_t)(i - 2), base, nsc, S, runs);
    base += nsc;
  }
  for (const SpecRunDev& r : runs) printf("R %u %u %u %u\n", r.frame, r.c, r.n, r.chunk);
  const unsigned long long gen = kSpecGeneration, g = kSpecRunMinGens;
  for (unsigned long long k = 1; k <= 5; k++)
    for (long long d = -1; d <= 1; d++) {
      const unsigned long long chunks = k * g * gen + (unsigned long long)d;
      printf("L %llu %u %u %u\n", chunks, spec_run_length(chunks, 0), spec_run_length(chunks, 1), spec_run_length(chunks, 9));
    }
  printf("L 40000 %u %u %u\n", spec_run_length(40000, 0), spec_run_length(40000, 3), spec_run_length(40000, -1));
  return 0;
}
"""

LENGTHS = [0, 1, 2047, 2048, 2049, 4095, 4096, 4097, 6143, 6144, 6145, 8191, 8192, 8193, 10240, 12288, 16384, 16385, 24576,
           100000, 590000, 1, 2048 * 12, 2048 * 12 + 1, 2048 * 12 - 1]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc: the header cannot be compiled here")
    d = tmp_path_factory.mktemp("spec_runs")
    src, exe = str(d / "spec_runs_host.hip"), str(d / "spec_runs_host")
    with open(src, "w") as f:
        f.write(PROGRAM)
    inc = os.path.join(os.path.dirname(os.path.dirname(LS.CSRC)), "include")
    # (the header has HIP's builtins and vector types: hipcc, the device side is compiled and never run)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-I", LS.CSRC, "-I", inc, "-o", exe, src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]

    def run(S, lengths):
        r = subprocess.run([exe, str(S)] + [str(x) for x in lengths], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        out = {"C": [], "T": [], "R": [], "L": []}
        for ln in r.stdout.splitlines():
            k, *v = ln.split()
            out[k].append([int(x) for x in v])
        return out
    return run


@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_the_run_list_covers_every_chunk_once_and_never_crosses_a_packet(host, S):
    rng = np.random.default_rng(S)
    lengths = LENGTHS + [int(x) for x in rng.integers(0, 40 * CHUNK, 300)]
    out = host(S, lengths)
    assert out["C"][0][0] == CHUNK
    nsc = [n // CHUNK + 1 for n in lengths]
    base = np.concatenate([[0], np.cumsum(nsc)])
    owner = np.zeros(base[-1], int)
    at = 0  # runs come packet by packet, chunk by chunk: the plan's order
    per_packet = [[] for _ in lengths]
    for frame, c, n, chunk in out["R"]:
        assert 1 <= n <= S and chunk == at == base[frame] + c, (frame, c, n, chunk)
        assert c + n <= nsc[frame], "a run leaves its packet"
        owner[chunk:chunk + n] += 1
        at += n
        per_packet[frame].append((c, n))
    assert (owner == 1).all() and at == base[-1]
    for f, runs in enumerate(per_packet):
        assert runs[0][0] == 0, "a packet's first run starts at byte 0"
        assert all(n == S for _, n in runs[:-1]), "only the last run of a packet is the shorter one"
        assert len(runs) == (nsc[f] + S - 1) // S


def test_run_tiles_and_the_bit_buffer_hold_a_run(host):
    out = host(1, [1])
    chunk, lead, smax, gen, gens = out["C"][0]
    assert [t for _, t in out["T"]] == [(lead + s * chunk) // 128 for s in range(1, smax + 1)]
    assert (lead + smax * chunk) < 65536  # positions and block counts of a run are 16-bit in the hand-over words


def test_the_run_length_follows_the_number_of_chunks(host):
    out = host(1, [1])
    _, _, smax, gen, gens = out["C"][0]
    assert smax == 4 and gen == 256 * 4 * 5 * 64
    for chunks, auto, one, nine in out["L"]:
        want = 1
        for k in range(2, smax + 1):
            if chunks // k >= gens * gen:
                want = k
        assert auto == want and one == (3 if chunks == 40000 else 1), (chunks, auto, one)
        if chunks != 40000:
            assert nine == smax  # forced values are clipped to the longest run
        else:
            assert nine == 1     # (the third column of that line is spec_run_length(40000, -1): not forced)
    by = {c: a for c, a, _, _ in out["L"]}
    assert by[40000] == 1 and by[2 * gens * gen - 1] == 1 and by[2 * gens * gen] == 2 and by[3 * gens * gen] == 3
    # the bench's launch (4,714,741 chunks) and the sweep's largest below it (4096 pictures, a quarter of that)
    assert 3 * gens * gen <= 4714741 < 4 * gens * gen and 4714741 // 4 < 2 * gens * gen


def test_the_host_builds_its_list_with_these_functions():
    host_src = open(os.path.join(LS.CSRC, "mi_rtjpeg.hip")).read()
    assert "spec_packet_runs((uint32_t)i, sp.h_base[i], sp.h_base[i + 1] - sp.h_base[i], sp.run_s, sp.h_runs)" in host_src
    assert "spec_run_length(sp.n, p->sw.spec_run)" in host_src
    assert 'getenv("MI_RTJ_SPEC_RUN")' in open(os.path.join(LS.CSRC, "rtj_host_switches.h")).read()
