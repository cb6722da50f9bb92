"""How a batch launch divides a picture among waves, restated in Python from the kernels' headers.

The constants are read from the headers by regular expression (nothing here is a copy of a number), the three host
functions that size a launch — split_luma_waves(), split_chroma_waves() (csrc/rtj_decode_chroma.h) and decode_slots()
(csrc/rtj_decode_kernels.h) — and the span rule of plan_launch (csrc/mi_rtjpeg.hip) are restated, and the ownership rule
of each kernel form is spelled out as an enumeration of its workgroups.  tests/test_launch_shapes_cpu.py pins all of it
to the headers; tests/test_gpu_launch_shapes.py takes its geometry list from geometry_classes() below, so the sweep
follows the constants when they are tuned.
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gmerlin-avdecoder_amd", "csrc")

# name -> (header, pattern whose group 1 is the value)
_PATTERNS = {
    "kMbPerGroup": ("rtj_common.h", r"constexpr int kMbPerGroup = (\d+);"),
    "kPoolGroups": ("rtj_decode_chroma.h", r"constexpr int kPoolGroups = (\d+);"),
    "kPoolItersMax": ("rtj_decode_chroma.h", r"constexpr int kPoolItersMax = (\d+);"),
    "kSplitLumaSuperGroups": ("rtj_decode_chroma.h", r"#define MIRTJ_SPLIT_LUMA_SG (\d+)"),
    "kXcds": ("rtj_decode_chroma.h", r"constexpr uint32_t kXcds = (\d+);"),
    "kSplitXcdRot": ("rtj_decode_chroma.h", r"constexpr uint32_t kSplitXcdRot = (\d+);"),
    "kDecIters": ("rtj_decode_kernels.h", r"#define MIRTJ_DEC_ITERS (\d+)"),
    "kDecMinWaves": ("rtj_decode_kernels.h", r"constexpr uint32_t kDecMinWaves = (\d+);"),
    "kDecRotateMinGroups": ("rtj_decode_kernels.h", r"constexpr uint32_t kDecRotateMinGroups = (\d+);"),
}


class Shapes:
    """The constants of one csrc directory and everything derived from them."""

    def __init__(self, csrc=CSRC):
        self.csrc = csrc
        text = {}
        for name, (hdr, pat) in _PATTERNS.items():
            if hdr not in text:
                text[hdr] = open(os.path.join(csrc, hdr)).read()
            m = re.search(pat, text[hdr])
            assert m, f"{hdr}: no match for {pat!r} ({name}): the header changed, restate it here"
            setattr(self, name, int(m.group(1)))

    # ------------------------------------------------------------------ sizes
    def groups(self, w, h):
        """macroblock groups of a w x h picture (multiples of 16): kMbPerGroup consecutive macroblocks each"""
        return ((w // 16) * (h // 16) + self.kMbPerGroup - 1) // self.kMbPerGroup

    def last_group_mbs(self, w, h):
        r = ((w // 16) * (h // 16)) % self.kMbPerGroup
        return r or self.kMbPerGroup

    def super_groups(self, groups):
        return (groups + self.kPoolGroups - 1) // self.kPoolGroups

    def per_xcd(self, groups):
        return (self.super_groups(groups) + self.kXcds - 1) // self.kXcds

    # ------------------------------------------------------------------ the three host functions
    def split_chroma_waves(self, groups):
        p = self.per_xcd(groups)
        return (p + self.kPoolItersMax - 1) // self.kPoolItersMax if p else 1

    def split_luma_waves(self, groups):
        p = self.per_xcd(groups)
        lw = (p + self.kSplitLumaSuperGroups - 1) // self.kSplitLumaSuperGroups if p else 1
        return lw if (lw + self.split_chroma_waves(groups)) & 1 else lw + 1

    def luma_waves_before_odd_rule(self, groups):
        p = self.per_xcd(groups)
        return (p + self.kSplitLumaSuperGroups - 1) // self.kSplitLumaSuperGroups if p else 1

    def decode_slots(self, groups, frames, span=1):
        by_iters = (groups + self.kDecIters - 1) // self.kDecIters
        per_slot = (1 if span == 3 else 3) * (frames if frames else 1)
        by_batch = min((self.kDecMinWaves + per_slot - 1) // per_slot, groups)
        return max(by_iters, by_batch) | 1

    def span(self, frames, max_groups, rotate=None):
        """plan_launch: MI_RTJ_ROTATE decides where it is set, the size of the batch otherwise"""
        if rotate is not None:
            return 3 if rotate else 1
        return 3 if frames * max_groups >= self.kDecRotateMinGroups else 1

    # ------------------------------------------------------------------ ownership, as the kernels state it
    def split_workgroups(self, luma_waves, chroma_waves, rot, frame):
        """k_decode_split, grid (kXcds * (L + C), frames): for every workgroup w of picture `frame`, in order,
        (kind, stripe x, wave r of its kind, first super group, step).  x = (w + frame * (rot & 7)) % kXcds,
        r = w / kXcds; waves r < L are luma waves, the others chroma waves numbered from 0."""
        out = []
        for w in range(self.kXcds * (luma_waves + chroma_waves)):
            x = (w + frame * (rot & 7)) % self.kXcds
            r = w // self.kXcds
            if r < luma_waves:
                out.append(("luma", x, r, x + self.kXcds * r, self.kXcds * luma_waves))
            else:
                out.append(("chroma", x, r - luma_waves, x + self.kXcds * (r - luma_waves), self.kXcds * chroma_waves))
        return out

    def split_owner_counts(self, nsg, waves, rot, frame):
        """How many waves of one kind (`waves` per XCD) take each of the nsg super groups of picture `frame`: a wave
        starts at its first super group and steps by kXcds * waves until the picture ends (decode_wave<kSuper> and
        chroma_pool_wave both loop over their stripe whatever its length)."""
        w = np.arange(self.kXcds * waves)
        first = (w + frame * (rot & 7)) % self.kXcds + self.kXcds * (w // self.kXcds)
        step = self.kXcds * waves
        waves_starting_at = np.bincount(first, minlength=step)  # (XCD, wave) ...
        return waves_starting_at[np.arange(nsg) % step]  # ... and its rounds: first, first + step, ... below nsg

    def split_owner(self, sg, waves, rot, frame):
        """(workgroup column within its kind, physical XCD, stripe, wave, round) of the wave that takes super group sg"""
        step = self.kXcds * waves
        first, rnd = sg % step, sg // step
        x, r = first % self.kXcds, first // self.kXcds
        xcd = (x - frame * (rot & 7)) % self.kXcds
        return dict(workgroup=self.kXcds * r + xcd, xcd=xcd, stripe=x, wave=r, round=rnd)

    def classic_owner_counts(self, groups, slots):
        """k_decode: slot s takes groups s, s + slots, ... for at most kDecIters rounds (span 3: all three parts; span 1:
        one wave per slot and part, the same groups)"""
        g = (np.arange(slots)[:, None] + np.arange(self.kDecIters)[None, :] * slots).reshape(-1)  # (slot, round)
        return np.bincount(g[g < groups], minlength=groups)

    # ------------------------------------------------------------------ where a byte of a picture belongs
    def describe_byte(self, w, h, off, form, frame=0, frames=1, max_groups=None, rot=None, lw=None, cw=None, slots=None):
        """plane, macroblock, group and owning wave (by the model above) of byte `off` of a w x h picture"""
        ysz = w * h
        mbw = w // 16
        if off < ysz:
            plane, y, x = "Y", off // w, off % w
            mb = (y // 16) * mbw + x // 16
            part = "luma"
        else:
            c = off - ysz
            plane = "Cb" if c < ysz // 4 else "Cr"
            c %= ysz // 4
            y, x = c // (w // 2), c % (w // 2)
            mb = (y // 8) * mbw + x // 8
            part = "chroma"
        g = mb // self.kMbPerGroup
        s = f"plane {plane} row {y} column {x}, macroblock {mb} (lane block {mb % self.kMbPerGroup} of group {g}"
        s += f", super group {g // self.kPoolGroups})"
        mg = max_groups or self.groups(w, h)
        if form == "split":
            waves = (lw or self.split_luma_waves(mg)) if part == "luma" else (cw or self.split_chroma_waves(mg))
            o = self.split_owner(g // self.kPoolGroups, waves, self.kSplitXcdRot if rot is None else rot, frame)
            s += f"; owner: {part} wave {o['wave']} of {waves} on XCD {o['xcd']} (stripe {o['stripe']}), round {o['round']}"
        else:
            span = 3 if form == "classic" else 1
            slots = slots or self.decode_slots(mg, frames, span)
            s += f"; owner: slot {g % slots} of {slots} (span {span}), round {g // slots}"
        return s

    # ------------------------------------------------------------------ the geometry list of the sweep
    def find_picture(self, pred, orient="any", limit=70000):
        """The smallest picture (fewest macroblocks; then the squarest, wider than high) whose macroblock count
        satisfies pred.  orient "wide": N x 16; "narrow": 16 x N; "any": no side longer than 16 times the other.
        Sides are limited to the header's 16 bits (4095 macroblocks).  None where there is none."""
        for nmb in range(1, limit):
            if not pred(nmb):
                continue
            if orient == "wide":
                if nmb <= 4095:
                    return 16 * nmb, 16
                return None
            if orient == "narrow":
                if nmb <= 4095:
                    return 16, 16 * nmb
                return None
            best = None
            for b in range(1, int(nmb ** 0.5) + 1):
                a = nmb // b
                if a * b == nmb and a <= 4095 and a <= 16 * b:
                    best = (a, b)
            if best:
                return 16 * best[0], 16 * best[1]
        return None

    def geometry_classes(self):
        """[(class name, w, h)] of tests/test_gpu_launch_shapes.py, derived from the constants; one picture may stand
        for several classes (names joined with '__')."""
        M, PG, X = self.kMbPerGroup, self.kPoolGroups, self.kXcds
        found = {}  # (w, h) -> [names], in order of first appearance

        def add(name, wh):
            if wh is not None:
                found.setdefault(wh, []).append(name)

        def groups_of(nmb):
            return (nmb + M - 1) // M

        def both(name, pred, strips=True):
            add(name, self.find_picture(pred, "any"))
            if strips:
                add(name + "-narrow", self.find_picture(pred, "narrow"))
                add(name + "-wide", self.find_picture(pred, "wide"))

        # fewer groups than a super group
        add("1-group", (16, 16))
        both("2-groups", lambda n: groups_of(n) == 2)
        # XCDs that own nothing / one super group each / one XCD with two
        for s in list(range(1, X)) + [X, X + 1]:
            both(f"{s}-super-groups", lambda n, s=s: self.super_groups(groups_of(n)) == s)
        # groups = 3k, 3k + 1, 3k + 2 with the last group full, with 1 and with 31 macroblocks
        for r in range(PG):
            for last, lname in ((M, "full"), (1, "1mb"), (M - 1, f"{M - 1}mb")):
                for k in range(2, 40):  # the first k for which such a picture exists
                    g = PG * k + r
                    wh = self.find_picture(lambda n, g=g, last=last: n == M * (g - 1) + last, "any")
                    if wh:
                        add(f"groups-{PG}k+{r}-last-{lname}", wh)
                        for o in ("narrow", "wide"):
                            add(f"groups-{PG}k+{r}-last-{lname}-{o}",
                                self.find_picture(lambda n, g=g, last=last: n == M * (g - 1) + last, o))
                        break
        # per_xcd on both sides of every step of lw up to the 4K value
        p4k = self.per_xcd(self.groups(3840, 2160))
        L = self.kSplitLumaSuperGroups
        steps = sorted({p for m in range(1, p4k // L + 2) for p in (m * L, m * L + 1) if p <= p4k} | {p4k})
        for p in steps:
            wh = self.find_picture(lambda n, p=p: self.per_xcd(groups_of(n)) == p, "any")
            if wh:
                g = self.groups(*wh)
                odd = "odd-rule-adds" if self.split_luma_waves(g) != self.luma_waves_before_odd_rule(g) else "odd-rule-keeps"
                add(f"per-xcd-{p}-{odd}", wh)
        # one, two and the 4K number of chroma waves per XCD; the pictures the project names where they still fit
        def prefer(name, named, pred):
            add(name, named if pred((named[0] // 16) * (named[1] // 16)) else self.find_picture(pred, "any"))

        prefer("per-xcd-pool-iters-max", (1920, 1088), lambda n: self.per_xcd(groups_of(n)) == self.kPoolItersMax)
        prefer("per-xcd-pool-iters-max+1", (2048, 1088), lambda n: self.per_xcd(groups_of(n)) == self.kPoolItersMax + 1)
        add("640x368", (640, 368))
        add("3840x2160", (3840, 2160))
        # strips: a group spans many macroblock rows / a fraction of one
        add("strip-narrow", self.find_picture(lambda n: self.super_groups(groups_of(n)) >= X + 1, "narrow"))
        add("strip-wide", self.find_picture(lambda n: self.super_groups(groups_of(n)) >= X + 1, "wide"))
        add("strip-wide-16-bit-limit", (65520, 16))
        add("strip-narrow-16-bit-limit", (16, 65520))
        return [("__".join(names), w, h) for (w, h), names in found.items()]

    def table_row(self, name, w, h, frames=9):
        g = self.groups(w, h)
        return dict(cls=name, w=w, h=h, groups=g, super_groups=self.super_groups(g), per_xcd=self.per_xcd(g),
                    last_mbs=self.last_group_mbs(w, h), lw=self.split_luma_waves(g), cw=self.split_chroma_waves(g),
                    slots_span3=self.decode_slots(g, frames, 3), slots_span1=self.decode_slots(g, frames, 1))


def print_table(frames=9):
    S = Shapes()
    print("| class | w x h | groups | super groups | per XCD | last group | lw | cw | slots span 3 | slots span 1 |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for name, w, h in S.geometry_classes():
        r = S.table_row(name, w, h, frames)
        print(f"| {name} | {w}x{h} | {r['groups']} | {r['super_groups']} | {r['per_xcd']} | {r['last_mbs']} | {r['lw']} | "
              f"{r['cw']} | {r['slots_span3']} | {r['slots_span1']} |")


if __name__ == "__main__":
    print_table()
