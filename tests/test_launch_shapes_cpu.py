"""tests/launch_shapes.py against the headers it restates, and the covering invariants of every launch shape.

What the kernels need for a correct picture (read from decode_wave, chroma_pool_wave and k_decode_split, not assumed):

* the split form (k_decode_split): a luma wave (decode_wave<kSuper>) and a pooling chroma wave (chroma_pool_wave) start at
  super group x + kXcds * r and step by kXcds * waves UNTIL THE PICTURE ENDS: neither loop is bounded by
  kSplitLumaSuperGroups or kPoolItersMax.  Those two constants size the launch for speed only, so
  `kXcds * lw * kSplitLumaSuperGroups >= super groups` and `kXcds * cw * kPoolItersMax >= super groups` are NOT needed
  for correctness (they are asserted below all the same, as statements about split_*_waves), and `lw + cw` odd is a
  speed rule.  What correctness needs is that the first super groups of the kXcds * waves waves of one kind are a
  permutation of 0 .. kXcds * waves - 1 for every picture of the launch, whatever the rotation: then every super group
  has exactly one luma and one chroma owner for ANY wave counts >= 1.  That is asserted by enumeration, for the
  computed counts and for the overridden ones tests/test_gpu_launch_shapes.py runs in the experiments build.
* the classic forms (k_decode, span 3 and span 1): a wave takes at most kDecIters groups, so
  `slots * kDecIters >= groups` IS needed, and is asserted with exact ownership by enumeration.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import launch_shapes as LS

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MAX_GROUPS = 40000   # 65520x16 has 128 groups, 3840x2160 has 1013: room to spare
PROGRAM_GROUPS = 1100
FRAMES = (1, 2, 9, 31, 32, 33, 128, 129, 256, 4096, 16384)

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "rtj_decode_chroma.h"
int main(int argc, char** argv) {
  using namespace mirtj;
  const unsigned top = (unsigned)atoi(argv[1]);
  printf("C %d %d %d %d %u %u %d %u %u\n", kMbPerGroup, kPoolGroups, kPoolItersMax, kSplitLumaSuperGroups, kXcds, kSplitXcdRot,
         kDecIters, kDecMinWaves, kDecRotateMinGroups);
  for (unsigned g = 1; g <= top; g++) {
    printf("W %u %u %u\n", g, split_luma_waves(g), split_chroma_waves(g));
    for (int i = 2; i < argc; i++) {
      const unsigned f = (unsigned)atoi(argv[i]);
      printf("S %u %u %u %u\n", g, f, decode_slots(g, f, 1u), decode_slots(g, f, 3u));
    }
    // frames on both sides of the span rule's threshold for this group count
    const unsigned f0 = kDecRotateMinGroups / g;
    for (unsigned f = f0 ? f0 - 1 : 0; f <= f0 + 1; f++)
      printf("S %u %u %u %u\n", g, f, decode_slots(g, f, 1u), decode_slots(g, f, 3u));
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def S():
    return LS.Shapes()


def host_values(csrc, workdir):
    """What the headers' own functions give, from a small host program (the headers use HIP's builtins and vector types:
    hipcc, not g++; the device side of the translation unit is compiled and never run)."""
    src = os.path.join(workdir, "launch_shapes_host.hip")
    exe = os.path.join(workdir, "launch_shapes_host")
    with open(src, "w") as f:
        f.write(PROGRAM)
    inc = os.path.join(os.path.dirname(os.path.dirname(csrc)), "include")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-w", "-I", csrc, "-I", inc, "-o", exe, src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    r = subprocess.run([exe, str(PROGRAM_GROUPS)] + [str(f) for f in FRAMES], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


def compare_with_host(S, lines):
    seen = {"C": 0, "W": 0, "S": 0}
    for ln in lines:
        k, *v = ln.split()
        v = [int(x) for x in v]
        seen[k] += 1
        if k == "C":
            assert v == [S.kMbPerGroup, S.kPoolGroups, S.kPoolItersMax, S.kSplitLumaSuperGroups, S.kXcds, S.kSplitXcdRot,
                         S.kDecIters, S.kDecMinWaves, S.kDecRotateMinGroups], "the regular expressions read other constants than the compiler"
        elif k == "W":
            g, lw, cw = v
            assert (S.split_luma_waves(g), S.split_chroma_waves(g)) == (lw, cw), \
                f"groups {g}: header gives lw {lw} cw {cw}, launch_shapes {S.split_luma_waves(g)} {S.split_chroma_waves(g)}"
        else:
            g, f, s1, s3 = v
            assert (S.decode_slots(g, f, 1), S.decode_slots(g, f, 3)) == (s1, s3), \
                f"groups {g} frames {f}: header gives slots {s1} / {s3}, launch_shapes {S.decode_slots(g, f, 1)} / {S.decode_slots(g, f, 3)}"
    assert seen["C"] == 1 and seen["W"] == PROGRAM_GROUPS and seen["S"] == PROGRAM_GROUPS * (len(FRAMES) + 3), seen


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="no hipcc: the headers cannot be compiled here")
def test_restatement_equals_the_headers_functions(S, tmp_path):
    compare_with_host(S, host_values(S.csrc, str(tmp_path)))


def test_the_kernels_still_read_as_the_model_says(S):
    """The model's structural assumptions, where a constant cannot carry them: the luma waves' super group is the literal 3
    of decode_wave's group_of(), the loops of both kinds of wave are bounded by the picture alone, the classic form by
    kDecIters, and the span rule and the stripe formula are the ones restated."""
    dec = open(os.path.join(S.csrc, "rtj_decode_kernels.h")).read()
    chroma = open(os.path.join(S.csrc, "rtj_decode_chroma.h")).read()
    host = open(os.path.join(S.csrc, "mi_rtjpeg.hip")).read()
    assert S.kPoolGroups == 3 and "return 3u * (slot + q * slots) + (g - 3u * q);" in dec
    assert "return (kSuper || g < (uint32_t)kDecIters) && group_of(g) < ngroups;" in dec
    assert "r.valid = (kSuper || g < (uint32_t)kDecIters) && r.grp < ngroups && r.mb < f.nmb;" in dec
    assert "for (uint32_t sg = slot;; sg += slots) {" in chroma and "const bool have_n = sg + slots < nsg;" in chroma
    assert "const uint32_t x = (blockIdx.x + blockIdx.y * (xcd_rot & 7u)) % kXcds;" in chroma
    assert "const uint32_t r = blockIdx.x / kXcds;" in chroma
    assert "x + kXcds * r, kXcds * luma_waves" in chroma and "x + kXcds * (r - luma_waves), kXcds * chroma_waves" in chroma
    assert "(uint64_t)drows * p->max_groups >= (uint64_t)kDecRotateMinGroups ? 3u : 1u" in host
    assert "dim3(kXcds * (lw + cw), drows)" in host
    assert "const dim3 grid(span == 3u ? dslots : dslots * 3u, drows)" in host


def test_sizing_invariants_for_every_group_count(S):
    for g in range(1, MAX_GROUPS + 1):
        sg, lw, cw = S.super_groups(g), S.split_luma_waves(g), S.split_chroma_waves(g)
        # statements about the sizing functions (speed: a wave's share stays within what it was tuned for)
        assert S.kXcds * lw * S.kSplitLumaSuperGroups >= sg, g
        assert S.kXcds * cw * S.kPoolItersMax >= sg, g
        assert (lw + cw) & 1, g
        assert lw >= 1 and cw >= 1, g
        # no wave more than the odd rule asks for
        assert lw - S.luma_waves_before_odd_rule(g) in (0, 1), g
        assert S.kXcds * (cw - 1) * S.kPoolItersMax < sg, g
        for frames in FRAMES:
            for span in (1, 3):
                slots = S.decode_slots(g, frames, span)
                assert slots * S.kDecIters >= g, (g, frames, span)  # needed: k_decode stops after kDecIters rounds
                assert slots & 1, (g, frames, span)


def test_every_group_has_one_luma_and_one_chroma_owner_in_the_split_form(S):
    """(XCD, wave, round) enumerated as k_decode_split states it, for every rotation 0..7 and the pictures 0..8 of a
    launch (picture * rotation mod 8 is all that enters: eight distinct shifts), for every group count: the counts depend
    on the number of super groups and the waves alone, so each (super groups, waves, shift) is enumerated once."""
    seen = {}

    def owners(nsg, waves, shift):
        key = (nsg, waves, shift)
        if key not in seen:
            seen[key] = bool((S.split_owner_counts(nsg, waves, shift, 1) == 1).all())
        return seen[key]

    for g in range(1, MAX_GROUPS + 1):
        nsg = S.super_groups(g)
        for waves in (S.split_luma_waves(g), S.split_chroma_waves(g)):
            for shift in range(8):
                assert owners(nsg, waves, shift), (g, waves, shift)
    # rotation and picture number enter as a product: spot-check the full (rot, frame) grid, and group-level counts
    for g in list(range(1, 120)) + [255, 272, 1013, 1020]:
        nsg = S.super_groups(g)
        for rot in range(8):
            for frame in range(9):
                for waves in (S.split_luma_waves(g), S.split_chroma_waves(g)):
                    per_group = np.repeat(S.split_owner_counts(nsg, waves, rot, frame), S.kPoolGroups)[:g]
                    assert per_group.size == g and (per_group == 1).all(), (g, rot, frame, waves)
                # the same from the workgroup list, the way the kernel walks it
                lw, cw = S.split_luma_waves(g), S.split_chroma_waves(g)
                count = {"luma": np.zeros(g, int), "chroma": np.zeros(g, int)}
                for kind, x, r, first, step in S.split_workgroups(lw, cw, rot, frame):
                    for sg in range(first, nsg, step):
                        for q in range(S.kPoolGroups):
                            if sg * S.kPoolGroups + q < g:
                                count[kind][sg * S.kPoolGroups + q] += 1
                assert (count["luma"] == 1).all() and (count["chroma"] == 1).all(), (g, rot, frame)
                if g > 119 and frame > 1:
                    break


def test_any_wave_counts_cover_the_picture_in_the_split_form(S):
    """Both kinds of wave loop over their stripe until the picture ends, so wave counts other than the computed ones
    (MI_RTJ_LUMA_WAVES / MI_RTJ_CHROMA_WAVES of the experiments build) cover every super group exactly once as well,
    even sums included: all of them are run on the device."""
    for g in (1, 2, 10, 29, 255, 272, 1013):
        nsg = S.super_groups(g)
        for waves in range(1, max(S.split_luma_waves(g), S.split_chroma_waves(g)) + 3):
            for rot in range(8):
                for frame in (0, 1, 5, 8):
                    assert (S.split_owner_counts(nsg, waves, rot, frame) == 1).all(), (g, waves, rot, frame)
                    o = S.split_owner(nsg - 1, waves, rot, frame)
                    assert 0 <= o["xcd"] < S.kXcds and o["workgroup"] < S.kXcds * waves


def test_every_group_has_one_owner_in_the_classic_forms(S):
    for g in list(range(1, 600)) + [1013, 4096, MAX_GROUPS]:
        for frames in (1, 9, 129, 4096, 16384):
            for span in (1, 3):
                c = S.classic_owner_counts(g, S.decode_slots(g, frames, span))
                assert (c == 1).all(), (g, frames, span)
    # and one wave too few does not cover: the bound is tight where by_iters decides
    g = 1013
    fewest = (g + S.kDecIters - 1) // S.kDecIters
    assert (S.classic_owner_counts(g, fewest) == 1).all() and not (S.classic_owner_counts(g, fewest - 1) == 1).all()


def test_span_rule(S):
    T = S.kDecRotateMinGroups
    for g in (1, 29, 255, 1013):
        f = (T + g - 1) // g
        assert S.span(f, g) == 3 and S.span(f - 1, g) == 1
    assert S.span(1, 1, rotate=1) == 3 and S.span(10 ** 6, 255, rotate=0) == 1


def test_geometry_list_holds_every_class_the_sweep_promises(S):
    cls = S.geometry_classes()
    names = "__".join(n for n, _, _ in cls)
    assert len({(w, h) for _, w, h in cls}) == len(cls)
    for _, w, h in cls:
        assert w % 16 == 0 and h % 16 == 0 and 16 <= w <= 65520 and 16 <= h <= 65520
    by = {}
    for n, w, h in cls:
        for part in n.split("__"):
            by[part] = (w, h)
    assert S.groups(*by["1-group"]) == 1 and S.groups(*by["2-groups"]) == 2
    for s in range(1, S.kXcds + 2):
        for o in ("", "-narrow", "-wide"):
            w, h = by[f"{s}-super-groups{o}"]
            assert S.super_groups(S.groups(w, h)) == s
            assert o != "-narrow" or w == 16
            assert o != "-wide" or h == 16
    M = S.kMbPerGroup
    for r in range(S.kPoolGroups):
        for lname, last in (("full", M), ("1mb", 1), (f"{M - 1}mb", M - 1)):
            w, h = by[f"groups-{S.kPoolGroups}k+{r}-last-{lname}"]
            assert S.groups(w, h) % S.kPoolGroups == r and S.last_group_mbs(w, h) == last
    p4k = S.per_xcd(S.groups(3840, 2160))
    L = S.kSplitLumaSuperGroups
    have = {int(p.split("-")[2]): p for p in by if p.startswith("per-xcd-") and p.split("-")[2].isdigit()}
    for m in range(1, p4k // L + 1):
        for p in (m * L, m * L + 1):
            if p <= p4k:
                assert p in have and S.per_xcd(S.groups(*by[have[p]])) == p, p
    assert p4k in have
    assert "odd-rule-adds" in names and "odd-rule-keeps" in names
    assert S.per_xcd(S.groups(*by["per-xcd-pool-iters-max"])) == S.kPoolItersMax
    assert S.per_xcd(S.groups(*by["per-xcd-pool-iters-max+1"])) == S.kPoolItersMax + 1
    assert S.split_chroma_waves(S.groups(*by["per-xcd-pool-iters-max"])) == 1
    assert S.split_chroma_waves(S.groups(*by["per-xcd-pool-iters-max+1"])) == 2
    assert S.split_chroma_waves(S.groups(3840, 2160)) == (p4k + S.kPoolItersMax - 1) // S.kPoolItersMax
    for n in ("strip-narrow", "strip-wide"):
        assert S.super_groups(S.groups(*by[n])) >= S.kXcds + 1 and 16 in by[n]
    assert by["strip-wide-16-bit-limit"] == (65520, 16) and by["strip-narrow-16-bit-limit"] == (16, 65520)
    assert by["640x368"] == (640, 368) and by["3840x2160"] == (3840, 2160)
