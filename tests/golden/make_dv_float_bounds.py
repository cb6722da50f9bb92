#!/usr/bin/env python3
"""Writes tests/golden/dv_float_bounds.json: how far the fixed-point DV statement (oracle/dv_oracle.c, dvo_*) is from
the floating-point one (oracle/dv_float.c, dvf_*) on exactly the seeded inputs tests/dvfloat.py builds for
tests/test_dv_float_cpu.py and tests/test_gpu_dv_float.py — and how far a deliberately wrong float model is on the same
inputs.  Nothing here is a tolerance somebody chose: a bound is the measured worst case rounded up to the next 0.25
level (absolute), 0.1 % (gain of a single-coefficient block) or 0.01 level (mean signed deviation), with no margin; the
GPU tests use the same numbers because the kernel has to equal the oracle bit for bit.  (PARITY UNPINNED: the file
says how well the fixed-point code realises the closed form, nothing about the standard.)"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import dvfloat as F  # noqa: E402

STEP = {"abs": 0.25, "gain": 0.001, "mean": 0.01}
BLOCK_INPUTS = {"position": F.position_sweep, "dc": F.dc_sweep, "random": F.random_blocks}


def r4(x):
    return round(float(x), 4)


def frames_measure(system, family, decoded):
    """worst |deviation|, largest |mean signed deviation| of a frame, blocks outside the range: over a family's frames"""
    worst, mean, out = 0.0, 0.0, 0
    for frame, got in decoded[system, family]:
        pic, n_out, _ = F.float_decode_info(system, frame)
        d = F.deviation(got, pic)
        worst, mean, out = max(worst, float(np.abs(d).max())), max(mean, abs(float(d.mean()))), out + n_out
    return {"abs": worst, "mean": mean, "out_of_range": out}


def main():
    oracle_px = {k: F.oracle_blocks(*f()) for k, f in BLOCK_INPUTS.items()}
    decoded = {(s, fam): [(fr, F.oracle_decode(s, fr)) for fr in F.frames(s, fam)] for s in (525, 625) for fam in "abc"}
    out = {"seeds": F.SEEDS, "pictures_525": F.PICTURES_525, "pictures_625": F.PICTURES_625, "target": F.TARGET, "step": STEP,
           "measured": {"blocks": {}, "frames": {"525": {}, "625": {}}}, "bounds": {"blocks": {}, "frames": {"525": {}, "625": {}}},
           "perturbations": {}}
    for k, f in BLOCK_INPUTS.items():
        m = F.measure_blocks(f(), oracle_px[k])
        assert m["out_of_range"] == 0, (k, m)
        out["measured"]["blocks"][k] = {q: r4(m[q]) for q in ("abs", "mean", "gain")}
        out["bounds"]["blocks"][k] = {"abs": F.up(m["abs"], STEP["abs"]), "mean": F.up(abs(m["mean"]), STEP["mean"])}
    out["bounds"]["blocks"]["position"]["gain"] = round(F.up(out["measured"]["blocks"]["position"]["gain"], STEP["gain"]), 3)
    del out["measured"]["blocks"]["dc"]["gain"], out["measured"]["blocks"]["random"]["gain"]  # one coefficient has a gain
    for s in (525, 625):
        for fam in "abc":
            m = frames_measure(s, fam, decoded)
            assert m["out_of_range"] == 0, (s, fam, m)
            out["measured"]["frames"][str(s)][fam] = {q: r4(m[q]) for q in ("abs", "mean")}
            out["bounds"]["frames"][str(s)][fam] = {"abs": F.up(m["abs"], STEP["abs"]), "mean": F.up(m["mean"], STEP["mean"])}
    # the deliberately wrong models, on the same inputs (525/60 frames: 625/50 carries the same segments)
    mode, k, cls, qno = F.sweep_index()
    for which, name in F.PERTURBATIONS.items():
        with F.perturbed(which):
            p = {"name": name}
            for key, f in BLOCK_INPUTS.items():
                m = F.measure_blocks(f(), oracle_px[key])
                p[key] = {"abs": r4(m["abs"])}
                if key == "position":
                    i = m["gain_at"]
                    p[key]["gain"] = r4(m["gain"])
                    p[key]["blamed"] = {"mode": int(mode[i]), "scan_position": int(k[i]), "class": int(cls[i]), "qno": int(qno[i])}
            for fam in "abc":
                p["frames_" + fam] = {"abs": r4(frames_measure(525, fam, decoded)["abs"])}
        out["perturbations"][str(which)] = p
    text = json.dumps(out, indent=1, sort_keys=True) + "\n"
    with open(F.BOUNDS, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
