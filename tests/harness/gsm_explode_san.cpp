// gsm_explode_san.cpp — the unpacker, the tables and the chain of libmi_gsm.so (csrc/gsm_format.h: the code mi_gsm_explode
// runs on the host and k_gsm_decode on the device) under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of
// its own: tests/test_gsm_explode_asan_cpu.py builds it with g++ and runs it as a child process.
//   (no argument)   unpacks seeded frames and blocks from heap blocks of exactly 33 and 65 bytes, so a read past the end is
//                   found, and holds every field to a reader that takes one bit at a time; walks both tables; decodes the
//                   same bytes through the chain.  Prints one line a group and "ok".
//   tables          prints the 512 values of xMp by (xmaxc, xMc), then the 512 of LARpp by (i, LARc)
//   decode FMT      reads a stream from standard input, decodes floor(len / 33) frames or floor(len / 65) blocks from a
//                   fresh state as the kernel does and writes the samples, then the 144 words of the state, then the count
//                   of bad magics, as decimal numbers
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../gmerlin-avdecoder_amd/csrc/gsm_format.h"

using namespace migsm;

namespace {
typedef std::vector<uint8_t> Bytes;

uint32_t rng_state = 610;
uint32_t rnd() {  // xorshift32
  rng_state ^= rng_state << 13, rng_state ^= rng_state >> 17, rng_state ^= rng_state << 5;
  return rng_state;
}

// as mi_gsm_explode: 1 for a bad magic
int explode(const uint8_t* block, int fmt, int16_t* params) {
  if (fmt == 0) {
    if ((block[0] >> 4) != 0xD) return 1;
    unpack([&](int b) { return (uint32_t)block[b]; }, true, 4, [&](int at, uint8_t v) { params[at] = v; });
    return 0;
  }
  unpack([&](int b) { return (uint32_t)block[b]; }, false, 0, [&](int at, uint8_t v) { params[at] = v; });
  unpack([&](int b) { return (uint32_t)block[32 + b]; }, false, 4, [&](int at, uint8_t v) { params[kParams + at] = v; });
  return 0;
}

// one bit at a time
void slow(const uint8_t* block, int fmt, int16_t* params) {
  int pos = fmt ? 0 : 4;
  for (int f = 0; f < kParams * (1 + fmt); f++) {
    const int w = width_of(f % kParams);
    int v = 0;
    for (int b = 0; b < w; b++, pos++) {
      const int bit = fmt ? (block[pos >> 3] >> (pos & 7)) & 1 : (block[pos >> 3] >> (7 - (pos & 7))) & 1;
      v = fmt ? v | bit << b : v << 1 | bit;
    }
    params[f] = (int16_t)v;
  }
}

struct Tab {
  int32_t xmp(int at) const { return tables().xmp[at]; }
  int32_t larpp(int at) const { return tables().larpp[at]; }
};
struct Hist {
  int16_t* p;
  int32_t get(int s) const {
    if (s < 0 || s >= kRing) exit(6);
    return p[s];
  }
  void set(int s, int32_t x) const {
    if (s < 0 || s >= kRing || x < -32768 || x > 32767) exit(7);
    p[s] = (int16_t)x;
  }
};

struct Decoder {
  Regs r;
  int16_t ring[kRing];
  uint32_t bad = 0;
  Decoder() {
    memset(&r, 0, sizeof r);
    memset(ring, 0, sizeof ring);
    r.nrp = 40, r.pos = 120;
  }
  // the frame of 33 bytes at p whose fields start `skip` bits in
  void frame(const uint8_t* p, bool msb, int skip, int16_t* pcm) {
    uint8_t par[kParams];
    unpack([&](int b) { return (uint32_t)p[b]; }, msb, skip, [&](int at, uint8_t v) { par[at] = v; });
    decode_frame(r, [&](int at) { return (uint32_t)par[at]; }, Tab(), Hist{ring}, [&](int at, const int32_t* s8) {
      for (int u = 0; u < 8; u++) pcm[at + u] = (int16_t)s8[u];
    });
  }
  void stream(const uint8_t* p, size_t len, int fmt, std::vector<int16_t>& pcm) {
    const size_t unit = fmt ? kBlockBytes : kFrameBytes;
    for (size_t at = 0; at + unit <= len; at += unit) {
      const size_t had = pcm.size();
      pcm.resize(had + (size_t)(kFrameSamples << fmt), 0);
      if (fmt) {
        frame(p + at, false, 0, pcm.data() + had);
        frame(p + at + 32, false, 4, pcm.data() + had + kFrameSamples);
      } else if ((p[at] >> 4) == 0xD) {
        frame(p + at, true, 4, pcm.data() + had);
      } else {
        bad++;
      }
    }
  }
  void words(int16_t* w) const {
    int at = r.pos - 120;
    if (at < 0) at += kRing;
    for (int k = 0; k < 120; k++, at = at + 1 == kRing ? 0 : at + 1) w[k] = ring[at];
    for (int k = 0; k < 9; k++) w[120 + k] = (int16_t)r.v[k];
    w[129] = (int16_t)r.msr, w[130] = (int16_t)r.nrp;
    for (int k = 0; k < 8; k++) w[131 + k] = (int16_t)r.prev[k];
    for (int k = 139; k < kStateWords; k++) w[k] = 0;
  }
};

int checks() {
  int frames = 0, blocks = 0;
  for (int fmt = 0; fmt < 2; fmt++)
    for (int t = 0; t < 4000; t++) {
      const size_t len = fmt ? kBlockBytes : kFrameBytes;
      uint8_t* block = (uint8_t*)malloc(len);  // exactly the unit: a read past it is the sanitizer's
      for (size_t k = 0; k < len; k++) block[k] = t == 0 ? 0x00 : t == 1 ? 0xFF : (uint8_t)rnd();
      if (!fmt && t % 8) block[0] = (uint8_t)(0xD0 | (block[0] & 15));
      int16_t got[2 * kParams], want[2 * kParams];
      const int rc = explode(block, fmt, got);
      if (rc != (!fmt && (block[0] >> 4) != 0xD)) return 2;
      if (rc == 0) {
        slow(block, fmt, want);
        if (memcmp(got, want, sizeof(int16_t) * (size_t)(kParams << fmt))) return 3;
        for (int f = 0; f < kParams << fmt; f++)
          if (got[f] < 0 || got[f] >= 1 << width_of(f % kParams)) return 4;
        Decoder d;
        std::vector<int16_t> pcm;
        d.stream(block, len, fmt, pcm);
        if (pcm.size() != (size_t)(kFrameSamples << fmt)) return 5;
      }
      free(block);
      fmt ? blocks++ : frames++;
    }
  printf("frames %d\nblocks %d\n", frames, blocks);
  long sum = 0;
  for (int k = 0; k < 512; k++) sum += tables().xmp[k] + tables().larpp[k];
  printf("tables %ld\n", sum);
  // a long seeded stream a format through the chain: every index into the ring and every word are checked by Hist
  for (int fmt = 0; fmt < 2; fmt++) {
    const size_t unit = fmt ? kBlockBytes : kFrameBytes, n = 300;
    uint8_t* s = (uint8_t*)malloc(unit * n);
    for (size_t k = 0; k < unit * n; k++) s[k] = (uint8_t)rnd();
    if (!fmt)
      for (size_t k = 0; k < n; k++) s[k * unit] = (uint8_t)(0xD0 | (s[k * unit] & 15));
    Decoder d;
    std::vector<int16_t> pcm;
    d.stream(s, unit * n, fmt, pcm);
    free(s);
    if (pcm.size() != n * (size_t)(kFrameSamples << fmt) || d.bad) return 8;
  }
  printf("chain 600\nok\n");
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 1) return checks();
  if (!strcmp(argv[1], "tables")) {
    for (int k = 0; k < 512; k++) printf("%d\n", tables().xmp[k]);
    for (int k = 0; k < 512; k++) printf("%d\n", tables().larpp[k]);
    return 0;
  }
  if (!strcmp(argv[1], "decode") && argc == 3) {
    const int fmt = atoi(argv[2]);
    Bytes in;
    uint8_t buf[4096];
    for (size_t got; (got = fread(buf, 1, sizeof buf, stdin)) > 0;) in.insert(in.end(), buf, buf + got);
    // from a heap block of exactly the stream's length
    uint8_t* s = (uint8_t*)malloc(in.size() ? in.size() : 1);
    if (!in.empty()) memcpy(s, in.data(), in.size());
    Decoder d;
    std::vector<int16_t> pcm;
    d.stream(s, in.size(), fmt != 0, pcm);
    free(s);
    int16_t w[kStateWords];
    d.words(w);
    for (int16_t x : pcm) printf("%d\n", x);
    for (int k = 0; k < kStateWords; k++) printf("%d\n", w[k]);
    printf("%u\n", d.bad);
    return 0;
  }
  return 64;
}
