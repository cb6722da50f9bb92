"""Which kind of plan honours which environment switch (csrc/rtj_host_switches.h, the table in DESIGN.md): a small host
program includes the header — it has no HIP types — and prints plan_switches_from_env() for the four kinds; it is run
under a handful of environments and every field is held to the table.

    batch (mi_rtj_plan_create)    reads MI_RTJ_INDEX, _EMIT, _SPEC, _DEC_SLOTS, _ROTATE, _SERIAL_MIN, _SPLIT, _OVERLAP
    one packet (mi_rtj_decode*)   reads MI_RTJ_INDEX, _EMIT, _SPEC; the rest at their defaults
    session slot, session group   read MI_RTJ_INDEX, _EMIT; spec_mode 0; the rest at their defaults
"""
import os
import shutil
import subprocess

import pytest

import launch_shapes as LS

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
COMPILER = HIPCC if (os.path.exists(HIPCC) or shutil.which(HIPCC)) else (shutil.which("c++") or shutil.which("g++"))

PROGRAM = r"""
#include <cstdio>
#include "rtj_host_switches.h"
int main() {
  using namespace mirtj;
  const PlanKind kinds[] = {kPlanBatch, kPlanOnePacket, kPlanSessionSlot, kPlanSessionGroup};
  const char* names[] = {"batch", "one_packet", "session_slot", "session_group"};
  for (int k = 0; k < 4; k++) {
    const PlanSwitches s = plan_switches_from_env(kinds[k]);
    printf("%s serial_index=%d emit_walk=%d spec_mode=%d dec_slots=%u rotate=%d serial_min=%u split=%d overlap_set=%d overlap=%d\n",
           names[k], (int)s.serial_index, (int)s.emit_walk, s.spec_mode, s.dec_slots, s.rotate, s.serial_min, s.split,
           (int)s.overlap_set, s.overlap);
  }
  return 0;
}
"""

DEFAULTS = dict(serial_index=0, emit_walk=0, spec_mode=-1, dec_slots=0, rotate=-1, serial_min=4096, split=-1, overlap_set=0,
                overlap=0)
# switch -> (a value that is not the default, the fields it sets)
SWITCHES = {
    "MI_RTJ_INDEX": ("serial", dict(serial_index=1)),
    "MI_RTJ_EMIT": ("walk", dict(emit_walk=1)),
    "MI_RTJ_SPEC": ("3", dict(spec_mode=3)),
    "MI_RTJ_DEC_SLOTS": ("7", dict(dec_slots=7)),
    "MI_RTJ_ROTATE": ("1", dict(rotate=1)),
    "MI_RTJ_SERIAL_MIN": ("17", dict(serial_min=17)),
    "MI_RTJ_SPLIT": ("0", dict(split=0)),
    "MI_RTJ_OVERLAP": ("2", dict(overlap_set=1, overlap=2)),
}
READS = {
    "batch": set(SWITCHES),
    "one_packet": {"MI_RTJ_INDEX", "MI_RTJ_EMIT", "MI_RTJ_SPEC"},
    "session_slot": {"MI_RTJ_INDEX", "MI_RTJ_EMIT"},
    "session_group": {"MI_RTJ_INDEX", "MI_RTJ_EMIT"},
}
FORCED = {"batch": {}, "one_packet": {}, "session_slot": dict(spec_mode=0), "session_group": dict(spec_mode=0)}


def expected(kind, env):
    want = dict(DEFAULTS)
    want.update(FORCED[kind])
    for name in sorted(READS[kind] & set(env)):
        value, fields = SWITCHES[name]
        assert env[name] == value
        want.update(fields)
    return want


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not COMPILER:
        pytest.skip("no C++ compiler: the header cannot be compiled here")
    d = tmp_path_factory.mktemp("plan_switches")
    src, exe = str(d / "plan_switches_host.cpp"), str(d / "plan_switches_host")
    with open(src, "w") as f:
        f.write(PROGRAM)
    # a plain host compile: no offload architecture, no HIP header — the header must stand without them
    r = subprocess.run([COMPILER, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", LS.CSRC, "-o", exe, src],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return exe


def table(exe, env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MI_RTJ_")}
    clean.update(env)
    r = subprocess.run([exe], capture_output=True, text=True, env=clean)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for ln in r.stdout.splitlines():
        kind, *fields = ln.split()
        out[kind] = {k: int(v) for k, v in (f.split("=") for f in fields)}
    assert sorted(out) == sorted(READS)
    return out


ENVIRONMENTS = {
    "nothing set": {},
    "every switch set": {k: v for k, (v, _) in SWITCHES.items()},
    "MI_RTJ_SPEC=1 alone": {"MI_RTJ_SPEC": "1"},
    "MI_RTJ_ROTATE=1 alone": {"MI_RTJ_ROTATE": "1"},
}


@pytest.mark.parametrize("name", list(ENVIRONMENTS))
def test_every_kind_of_plan_reads_the_switches_the_table_says(program, name):
    env = ENVIRONMENTS[name]
    got = table(program, env)
    for kind in READS:
        if name == "MI_RTJ_SPEC=1 alone":
            want = dict(DEFAULTS, spec_mode=1 if "MI_RTJ_SPEC" in READS[kind] else FORCED[kind]["spec_mode"])
        else:
            want = expected(kind, env)
        assert got[kind] == want, (kind, name)


@pytest.mark.parametrize("switch", list(SWITCHES))
def test_a_switch_reaches_only_the_kinds_that_read_it(program, switch):
    """one switch at a time: a kind that does not read it stays at nothing-set, field by field — a one-packet plan that
    began to honour MI_RTJ_ROTATE would take the split form"""
    base = table(program, {})
    got = table(program, {switch: SWITCHES[switch][0]})
    for kind in READS:
        if switch in READS[kind]:
            assert got[kind] == dict(base[kind], **SWITCHES[switch][1]), (kind, switch)
        else:
            assert got[kind] == base[kind], (kind, switch)


def test_the_values_that_are_not_numbers_as_they_are(program):
    """the words and the 'given at all' switches: anything but the word is the default; 0 is a value, not 'not given'"""
    got = table(program, {"MI_RTJ_INDEX": "parallel", "MI_RTJ_EMIT": "tables", "MI_RTJ_ROTATE": "0", "MI_RTJ_SPLIT": "5",
                          "MI_RTJ_OVERLAP": "0", "MI_RTJ_SERIAL_MIN": "0", "MI_RTJ_SPEC": "0"})
    assert got["batch"] == dict(DEFAULTS, rotate=0, split=1, overlap_set=1, overlap=0, serial_min=0, spec_mode=0)
    assert got["one_packet"] == dict(DEFAULTS, spec_mode=0)
    assert got["session_slot"] == got["session_group"] == dict(DEFAULTS, spec_mode=0)
