"""No-GPU checks of the product library: it builds, loads, exports every symbol that
include/mi_rtjpeg.h declares, builds the same quantiser tables as the reference, and refuses to run
without a device instead of falling back to a CPU path."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rtjlib as R
from pkg import P, ROOT


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "mi_rtjpeg.h")).read()
    declared = sorted(set(re.findall(r"\b(mi_rtj_[a-z0-9_]+)\s*\(", hdr)))
    assert len(declared) >= 20
    L = C.CDLL(P.lib_path())
    for name in declared:
        assert hasattr(L, name), name
    assert sorted(P.binding.EXPORTS) == declared


def test_product_tables_match_reference_golden():
    G = np.load(R.GOLDEN + "/rtjpeg_golden.npz")
    for Q in range(1, 256):
        l, c, lb8, cb8 = P.get_tables(Q)
        assert np.array_equal(l, G["tab_liqt"][Q - 1]), Q
        assert np.array_equal(c, G["tab_ciqt"][Q - 1]), Q
        assert (lb8, cb8) == tuple(G["tab_b8"][Q - 1]), Q


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful without a GPU")
def test_no_device_fails_loudly_and_never_decodes_on_cpu():
    assert P.device_count() == 0
    with pytest.raises(P.MiRtjError, match="no CPU path|no HIP device|gfx950"):
        P.MiRtj()


def test_product_does_not_link_or_import_the_oracle():
    # the oracle is test infrastructure: nothing under the package may mention it
    pkgdir = os.path.join(ROOT, "gmerlin-avdecoder_amd")
    for dp, _, fs in os.walk(pkgdir):
        for f in fs:
            if f.endswith((".py", ".h", ".hip", ".cpp", ".c")):
                txt = open(os.path.join(dp, f), errors="ignore").read()
                assert "rtj_oracle" not in txt and "rtjlib" not in txt and "oracle/" not in txt, f


@pytest.mark.skipif(os.path.exists("/dev/kfd") or not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="compiler check; run where the library is cross-compiled")
def test_hand_issued_loads_of_k_decode_are_not_touched_before_their_wait(tmp_path):
    """k_decode issues its look-ahead loads from inline assembly and waits for them by hand (a counted
    vmcnt behind the row stores); the compiler does not know those registers are still being filled.
    tools/check_async_loads.py reads the device assembly of the shipped sources and fails if anything
    touches them early, if a compiler-placed vmcnt wait sits in between, or if a transform variant does
    not issue exactly the eight stores the counted wait assumes."""
    import subprocess
    import sys
    csrc = os.path.join(ROOT, "gmerlin-avdecoder_amd", "csrc")
    # the shipped build and the test build of tests/test_gpu_variant_paths.py (its own flags, its own register allocation)
    for name, flags in (("product", []), ("general", ["-DMIRTJ_TEST_GENERIC_PATHS"])):
        d = tmp_path / name
        d.mkdir()
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        "-Wno-unused-function", "-save-temps=obj", *flags, "-o", str(d / "lib.so"),
                        os.path.join(csrc, "mi_rtjpeg.hip")], check=True, capture_output=True, cwd=str(d))
        asm = d / "mi_rtjpeg-hip-amdgcn-amd-amdhsa-gfx950.s"
        assert asm.exists()
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_async_loads.py"), str(asm)],
                           capture_output=True, text=True)
        assert r.returncode == 0, name + ": " + r.stdout + r.stderr


# every MIRTJ_ name the kernel sources test in a preprocessor conditional: the size parameters a build may override,
# and the two builds build.py knows besides the product.  A compile-time form switch is code that nothing builds or
# tests; one that is added has to be added here, where someone reviews it.
CONDITIONAL_NAMES = {
    "MIRTJ_DEC_ITERS", "MIRTJ_DEC_WAVES", "MIRTJ_COEF_STRIDE", "MIRTJ_DEC_LDS_PAD", "MIRTJ_SPLIT_LUMA_SG",
    "MIRTJ_NOP_ROW", "MIRTJ_NOP_COL", "MIRTJ_NOP_PX", "MIRTJ_NOP_LO3",
    "MIRTJ_SPEC_CHUNK", "MIRTJ_SPEC_LEAD", "MIRTJ_SPEC_LEAD_LONG", "MIRTJ_SPEC_LEAD_VERY", "MIRTJ_SPEC_VER_THREADS",
    "MIRTJ_SPEC_VER_BATCH",
    "MIRTJ_SEARCH_UNROLL", "MIRTJ_F_CHAINS", "MIRTJ_SUM_WAVES", "MIRTJ_EMIT_THREADS",
    "MIRTJ_TEST_GENERIC_PATHS", "MIRTJ_EXPERIMENTS",
}


def test_kernel_sources_test_no_macro_outside_the_reviewed_list():
    csrc = os.path.join(ROOT, "gmerlin-avdecoder_amd", "csrc")
    found = set()
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".h", ".hip")):
            continue
        txt = open(os.path.join(csrc, f), errors="ignore").read().replace("\\\n", " ")
        for line in re.findall(r"^[ \t]*#[ \t]*(?:if|ifdef|ifndef|elif)\b(.*)$", txt, re.M):
            found |= set(re.findall(r"\bMIRTJ_\w+", line.split("//")[0]))
    assert found == CONDITIONAL_NAMES, (sorted(found - CONDITIONAL_NAMES), sorted(CONDITIONAL_NAMES - found))
