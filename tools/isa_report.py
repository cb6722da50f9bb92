"""Static resource and instruction-class report of the compiled gfx950 kernels.

    python tools/isa_report.py [--unit rtjpeg|dv|tga|spu|gsm|pcm][--kernel k_decode] [--cflags "..."] [--keep DIR] [--json] [--digest]
                               [--opcodes] [--src DIR] [--bodies FILE]

Compiles csrc/mi_rtjpeg.hip (--unit dv: csrc/mi_dv.hip) with -save-temps (device assembly) and prints, per kernel, what the
code object's metadata says (VGPR / SGPR count, scalar-register spills, LDS bytes, scratch) and a
static census of the instruction stream: vector / scalar / LDS / vector-memory instructions and —
the figure VERDICT r2 asked to track — v_readlane_b32 / v_writelane_b32 (scalar spills are paid in
those).  Numbers are static (program text), not dynamic counts.  --digest adds a hash of each kernel's instruction
text, so that two builds can be shown to compile a kernel to the same code.  What is hashed: the kernel's instruction
lines and its labels, in order, with comments dropped and branch labels renumbered.  Lines that begin with `.` and are
no label (assembler directives: .amdhsa_kernel <mangled name>, .section .text.<mangled name>, the kernel descriptor)
are left out, so a kernel that is renamed or becomes a template instance keeps its hash when its code is the same; the
register, spill, LDS and scratch figures come from the metadata and are printed beside the hash.  --src compiles another
checkout's csrc/ (e.g. the parent commit's) with this tool; --bodies writes the hashed text of the selected kernels to a
file, so that `diff` can compare two builds line by line.  --opcodes adds a second hash, of the mnemonics and labels in
order with the operands dropped: two builds that differ only in register numbering keep it."""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gmerlin-avdecoder_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


UNITS = {"rtjpeg": ("mi_rtjpeg", ["mi_rtjpeg.hip", "rtj_tables.cpp"]), "dv": ("mi_dv", ["mi_dv.hip", "dv_tables.cpp"]),
         "tga": ("mi_tga", ["mi_tga.hip"]), "spu": ("mi_spu", ["mi_spu.hip"]),
         "gsm": ("mi_gsm", ["mi_gsm.hip"]), "pcm": ("mi_pcm", ["mi_pcm.hip"])}


def device_asm(cflags, keep=None, csrc=CSRC, unit="rtjpeg"):
    d = keep or tempfile.mkdtemp(prefix="mirtj_isa_")
    os.makedirs(d, exist_ok=True)
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-function",
           "-save-temps"] + cflags + ["-o", os.path.join(d, "lib.so")] + [os.path.join(csrc, f) for f in UNITS[unit][1]]
    r = subprocess.run(cmd, cwd=d, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stdout + r.stderr)
    for f in os.listdir(d):
        if f.startswith(UNITS[unit][0] + "-") and f.endswith("gfx950.s"):
            return os.path.join(d, f)
    raise RuntimeError("no device assembly in " + d)


def demangle(names):
    try:
        r = subprocess.run(["c++filt"] + names, capture_output=True, text=True)
        out = r.stdout.split("\n")
        return {n: (out[i] if i < len(out) and out[i] else n) for i, n in enumerate(names)}
    except OSError:
        return {n: n for n in names}


def parse(path):
    text = open(path).read().split("\n")
    kernels = {}
    cur = None
    for ln in text:
        m = re.match(r"^(_Z\w+):\s", ln)
        if m:
            cur = m.group(1)
            kernels[cur] = {"lines": []}
            continue
        if ln.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is not None:
            kernels[cur]["lines"].append(ln)
    # metadata
    meta = {}
    name = None
    block = {}
    for ln in text:
        s = ln.strip()
        if s.startswith("- .agpr_count") or s.startswith("- .args"):
            if name:
                meta[name] = block
            name, block = None, {}
        m = re.match(r"^(?:    |  - )\.(\w+):\s+(\S+)", ln)  # kernel-level keys only (argument entries sit deeper)
        if m:
            block[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                name = m.group(2)
    if name:
        meta[name] = block
    rep = {}
    for k, v in kernels.items():
        if k not in meta:
            continue
        c = {"valu": 0, "salu": 0, "lds": 0, "vmem": 0, "smem": 0, "v_readlane": 0, "v_writelane": 0, "waitcnt": 0,
             "s_nop": 0, "branch": 0}
        for ln in v["lines"]:
            s = ln.strip()
            if not s or s.startswith(";") or s.startswith("."):
                continue
            op = s.split()[0]
            if op.endswith(":"):
                continue
            if op.startswith("v_readlane") or op.startswith("v_readfirstlane"):
                c["v_readlane"] += 1
            if op.startswith("v_writelane"):
                c["v_writelane"] += 1
            if op.startswith("v_"):
                c["valu"] += 1
            elif op.startswith("s_waitcnt"):
                c["waitcnt"] += 1
            elif op.startswith("s_nop"):
                c["s_nop"] += 1
            elif op.startswith("s_cbranch") or op.startswith("s_branch"):
                c["branch"] += 1
            elif op.startswith("s_load") or op.startswith("s_buffer_load") or op.startswith("s_store"):
                c["smem"] += 1
            elif op.startswith("s_"):
                c["salu"] += 1
            elif op.startswith("ds_"):
                c["lds"] += 1
            elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
                c["vmem"] += 1
        body = [re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s*;.*$", "", ln.strip())) for ln in v["lines"]]
        # instructions and labels only: directives (.amdhsa_kernel <name>, .section .text.<name>, .p2align ...) carry
        # the kernel's mangled name and its descriptor, which the resource figures below report from the metadata
        body = [x for x in body if x and (not x.startswith(".") or x.endswith(":"))]
        digest = hashlib.sha1("\n".join(body).encode()).hexdigest()[:16]
        opcodes = hashlib.sha1("\n".join(x.split()[0] for x in body).encode()).hexdigest()[:16]
        m = meta[k]
        rep[k] = {"digest": digest, "opcodes": opcodes, "body": body, "vgpr": int(m.get("vgpr_count", 0)), "sgpr": int(m.get("sgpr_count", 0)),
                  "sgpr_spill": int(m.get("sgpr_spill_count", 0)), "vgpr_spill": int(m.get("vgpr_spill_count", 0)),
                  "lds_bytes": int(m.get("group_segment_fixed_size", 0)),
                  "scratch_bytes": int(m.get("private_segment_fixed_size", 0)), "static": c}
    return rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", default="")
    ap.add_argument("--cflags", default=os.environ.get("MI_RTJ_CFLAGS", ""))
    ap.add_argument("--keep", default=None)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--digest", action="store_true", help="print a hash of each kernel's instruction text")
    ap.add_argument("--opcodes", action="store_true", help="print a hash of each kernel's mnemonics and labels, operands dropped")
    ap.add_argument("--src", default=CSRC, help="the csrc/ directory to compile")
    ap.add_argument("--unit", choices=sorted(UNITS), default="rtjpeg", help="which library's kernels")
    ap.add_argument("--bodies", default=None, help="write the selected kernels' instruction text (as hashed) to this file")
    a = ap.parse_args()
    rep = parse(device_asm(a.cflags.split(), a.keep, a.src, a.unit))
    names = demangle(list(rep))
    out = {}
    for k, v in rep.items():
        short = re.sub(r"\(.*", "", names[k]).replace("mirtj::", "").replace("midv::", "").replace("void ", "")
        if a.kernel and a.kernel not in short:
            continue
        out[short] = v
    bodies = {k: v.pop("body") for k, v in out.items()}
    if a.bodies:
        with open(a.bodies, "w") as f:
            for k in sorted(bodies):
                f.write(f"==== {k} ({len(bodies[k])} lines)\n" + "\n".join(bodies[k]) + "\n")
    if a.json:
        print(json.dumps(out, indent=1))
        return
    for k, v in out.items():
        c = v["static"]
        print(f"{k}: vgpr {v['vgpr']} sgpr {v['sgpr']} sgpr_spill {v['sgpr_spill']} vgpr_spill {v['vgpr_spill']} "
              f"lds {v['lds_bytes']} scratch {v['scratch_bytes']} | valu {c['valu']} (readlane {c['v_readlane']} "
              f"writelane {c['v_writelane']}) salu {c['salu']} smem {c['smem']} lds {c['lds']} vmem {c['vmem']} "
              f"waitcnt {c['waitcnt']} s_nop {c['s_nop']} branch {c['branch']}" + (f" | text {v['digest']}" if a.digest else "") +
              (f" | opcodes {v['opcodes']}" if a.opcodes else ""))


if __name__ == "__main__":
    sys.exit(main())
