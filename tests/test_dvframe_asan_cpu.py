"""csrc/dvframe_host.c under AddressSanitizer + UndefinedBehaviorSanitizer in a small stand-alone program with its own
main, compiled together with the file (the sanitizers' runtimes linked in) and run directly: every profile x rate x quantisation x both
values of the 720p half-frame bits x the smallest and the largest sample count, each into frame and pair buffers
allocated at exactly their sizes, and the four metadata readers on the same frames.  What it is for: the 720p50 profile
has 12 DIF sequences and the 10-row 525/60 shuffle table; before a profile carried its row count the de-shuffle read rows
10 and 11 past the table (a global-buffer-overflow at the 16-bit read of audio_shuffle[q][j]), and no other test fed that
profile to the audio reader."""
import os
import shutil
import subprocess

import pytest

from pkg import ROOT

PROGRAM = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "mi_dvframe.h"

enum { PAIR_BYTES = 8192, SOURCE_PACK = 80 * 6 + 80 * 16 * 3 + 3 };

static uint32_t g_state = 12345u;
static uint8_t noise(void) { g_state = g_state * 1664525u + 1013904223u; return (uint8_t)(g_state >> 24); }

int main(void) {
  int calls = 0;
  setvbuf(stdout, NULL, _IOLBF, 0);
  for (int i = 0; i < mi_dv_num_profiles(); i++) {
    const mi_dv_profile *p = mi_dv_profile_at(i);
    uint8_t *frame = malloc((size_t)p->frame_size); /* exactly the frame: a read past it is a read past an allocation */
    for (int k = 0; k < p->frame_size; k++) frame[k] = noise();
    frame[3] = (uint8_t)((frame[3] & 0x7f) | p->dsf << 7);
    frame[5] = (uint8_t)((frame[5] & 0xf8) | (i == 2));
    frame[80 * 5 + 48 + 3] = (uint8_t)((frame[80 * 5 + 48 + 3] & 0xe0) | p->video_stype);
    if (i != 1 && i != 2 && mi_dv_frame_profile(frame) != p) { printf("FAILED: profile %d is not found from its own header\n", i); return 1; }
    if (p->audio_shuffle_rows != (p->audio_stride == 90 ? 10 : 12) || p->audio_shuffle_rows > p->difseg_size) {
      printf("FAILED: profile %d says its table has %d rows\n", i, p->audio_shuffle_rows);
      return 1;
    }
    for (int rate = 0; rate < 3; rate++)
      for (int quant = 0; quant < 2; quant++)
        for (int half = 0; half < 2; half++)
          for (int extra = 0; extra < 64; extra += 63)
            for (int pairs = 1; pairs <= 4; pairs++) {
              uint8_t *pcm[4] = {NULL, NULL, NULL, NULL};
              for (int k = 0; k < pairs; k++) pcm[k] = calloc(1, PAIR_BYTES);
              frame[1] = (uint8_t)((frame[1] & 0xf3) | half << 2);
              frame[SOURCE_PACK] = 0x50, frame[SOURCE_PACK + 1] = (uint8_t)extra, frame[SOURCE_PACK + 4] = (uint8_t)(rate << 3 | quant);
              const int n = mi_dv_extract_audio(p, frame, pcm);
              if (n != p->audio_min_samples[rate] + extra) { printf("FAILED: profile %d answers %d samples\n", i, n); return 1; }
              for (int k = 0; k < pairs; k++) free(pcm[k]);
              calls++;
            }
    int a, b, c, d;
    (void)mi_dv_timecode(p, frame, &a, &b, &c, &d), (void)mi_dv_date(p, frame, &a, &b, &c), (void)mi_dv_time(p, frame, &a, &b, &c);
    mi_dv_pixel_aspect(p, frame, &a, &b);
    free(frame);
    printf("ok profile %d\n", i);
  }
  printf("done: %d calls\n", calls);
  return 0;
}
"""

GCC = shutil.which(os.environ.get("CC", "gcc"))


def have_sanitizer_runtime():
    if not GCC:
        return False
    for name in ("libasan.a", "libubsan.a"):  # linked into the program: it does not depend on what the process preloads
        p = subprocess.run([GCC, "-print-file-name=" + name], capture_output=True, text=True).stdout.strip()
        if not (os.path.isabs(p) and os.path.exists(p)):
            return False
    return True


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if not have_sanitizer_runtime():
        pytest.skip("no gcc with a sanitizer runtime in this toolchain")
    d = tmp_path_factory.mktemp("dvframe_asan")
    src, exe = str(d / "dvframe_walk.c"), str(d / "dvframe_walk")
    with open(src, "w") as f:
        f.write(PROGRAM)
    r = subprocess.run([GCC, "-std=gnu99", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"), "-o", exe, src,
                        os.path.join(ROOT, "gmerlin-avdecoder_amd", "csrc", "dvframe_host.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)  # the binary itself, run directly
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout.splitlines()


def test_the_walk_ran_to_its_end_with_no_report(report):
    assert not [ln for ln in report if ln.startswith("FAILED")]
    # 9 profiles x 3 rates x 2 quantisations x 2 half-frame values x 2 sample counts x 1..4 pair buffers
    assert report[-1] == f"done: {9 * 3 * 2 * 2 * 2 * 4} calls"


@pytest.mark.parametrize("profile", range(9))
def test_every_profile_was_walked(report, profile):
    assert f"ok profile {profile}" in report
