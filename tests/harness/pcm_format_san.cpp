// pcm_format_san.cpp — the host forms of libmi_pcm.so (csrc/pcm_format.h: the transforms k_pcm_decode runs on the device,
// the G.711 tables, the float classifiers, layout_of, payload_of and codec_of) as a program of its own.
// tests/test_pcm_format_asan_cpu.py builds it with AddressSanitizer and UndefinedBehaviorSanitizer and runs it without
// arguments: every codec over seeded packets of every length around its groups, each from a heap block of exactly the
// packet's length into a heap block of exactly the result's, so a byte read behind a group tail or written behind the
// samples stops the run.  tests/test_pcmraw_cpu.py builds it plain and asks for single results:
//   tables                          the 512 table entries as text
//   f32 | f64                       binary words (pairs hi, lo) on stdin -> binary (class, bits) or (class, hi, lo)
//   layout LPCM_MAX PLAIN_MAX       binary uint64 x 5 (frames, written, consumed, out_bytes, valid_in) for every codec,
//                                   1..8 channels (mono: 1) and every length 0..max
//   decode CODEC CH                 the packet on stdin -> binary: the count, then the samples
//   codec_of                        lines "fourcc bits ch endianess header_len flags" -> "codec label align size" or "-1"
//   payload                         lines "len duration block_align" -> the clamp
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../gmerlin-avdecoder_amd/csrc/pcm_format.h"

using namespace mipcm;

static std::vector<uint8_t> read_all(FILE* f) {
  std::vector<uint8_t> v;
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
  return v;
}

// the packet from a heap block of exactly its length into one of exactly the result's
static bool decode_exact(int codec, uint32_t ch, const uint8_t* data, size_t len, std::vector<uint8_t>* out, uint32_t* outside) {
  if (codec < 0 || codec >= kCodecs || ch < 1 || ch > (uint32_t)kMaxChannels) return false;
  const Layout l = layout_of(codec, ch, len);
  uint8_t* in = (uint8_t*)malloc(len ? len : 1);
  uint8_t* o = (uint8_t*)malloc(l.out_bytes ? (size_t)l.out_bytes : 1);
  if (len) memcpy(in, data, len);
  const bool ok = decode_host(codec, ch, in, len, o, outside);
  if (ok) out->assign(o, o + l.out_bytes);
  free(in);
  free(o);
  return ok;
}

static int self_run() {
  uint32_t x = 12345u;
  unsigned long packets = 0, bytes = 0;
  for (int codec = 0; codec < kCodecs; codec++) {
    const Group& g = kGroups[codec];
    for (uint32_t ch : {1u, 2u, 3u, 6u}) {
      if (g.mono && ch != 1) continue;
      const size_t top = 3 * (size_t)g.piece_in * ch + 2 * g.in_bytes + 3;
      for (size_t len = 0; len <= top; len++) {
        std::vector<uint8_t> data(len), out;
        for (auto& b : data) b = (uint8_t)((x = x * 1664525u + 1013904223u) >> 24);
        uint32_t outside = 0;
        if (!decode_exact(codec, ch, data.data(), len, &out, &outside)) return 1;
        const Layout l = layout_of(codec, ch, len);
        if (out.size() != l.out_bytes || l.consumed > len || l.valid_in > l.consumed || l.written > l.frames * ch) return 1;
        if (!is_float(codec) && outside) return 1;
        // the samples upstream reports but does not write are zeros
        for (uint64_t b = l.written * sample_bytes(codec); b < l.out_bytes; b++)
          if (out[b]) return 1;
        packets++, bytes += len;
      }
    }
  }
  printf("packets %lu\nbytes %lu\nok\n", packets, bytes);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return self_run();
  const char* mode = argv[1];
  if (!strcmp(mode, "tables")) {
    for (int b = 0; b < 256; b++) printf("%d\n", kUlawTable.v[b]);
    for (int b = 0; b < 256; b++) printf("%d\n", kAlawTable.v[b]);
    return 0;
  }
  if (!strcmp(mode, "f32")) {
    const std::vector<uint8_t> in = read_all(stdin);
    for (size_t i = 0; i + 4 <= in.size(); i += 4) {
      uint32_t b;
      memcpy(&b, &in[i], 4);
      const uint32_t r[2] = {(uint32_t)classify32(b), read32(b)};
      fwrite(r, 4, 2, stdout);
    }
    return 0;
  }
  if (!strcmp(mode, "f64")) {
    const std::vector<uint8_t> in = read_all(stdin);
    for (size_t i = 0; i + 8 <= in.size(); i += 8) {
      uint32_t w[2];  // hi, lo
      memcpy(w, &in[i], 8);
      uint32_t o[4];
      uint8_t le[16] = {0};
      memcpy(le, &w[1], 4), memcpy(le + 4, &w[0], 4);
      piece<kF64le>([&](int k) { return (uint32_t)le[k]; }, o);
      const uint32_t r[3] = {(uint32_t)classify64(w[0], w[1]), o[1], o[0]};
      fwrite(r, 4, 3, stdout);
    }
    return 0;
  }
  if (!strcmp(mode, "layout") && argc == 4) {
    const uint64_t lpcm_max = strtoull(argv[2], nullptr, 10), plain_max = strtoull(argv[3], nullptr, 10);
    for (int codec = 0; codec < kCodecs; codec++)
      for (uint32_t ch = 1; ch <= (kGroups[codec].mono ? 1u : 8u); ch++)
        for (uint64_t len = 0; len <= (kGroups[codec].lpcm ? lpcm_max : plain_max); len++) {
          const Layout l = layout_of(codec, ch, len);
          const uint64_t r[5] = {l.frames, l.written, l.consumed, l.out_bytes, l.valid_in};
          fwrite(r, 8, 5, stdout);
        }
    return 0;
  }
  if (!strcmp(mode, "decode") && argc == 4) {
    const std::vector<uint8_t> in = read_all(stdin);
    std::vector<uint8_t> out;
    uint32_t outside = 0;
    if (!decode_exact(atoi(argv[2]), (uint32_t)atoi(argv[3]), in.data(), in.size(), &out, &outside)) return 3;
    fwrite(&outside, 4, 1, stdout);
    if (!out.empty()) fwrite(out.data(), 1, out.size(), stdout);
    return 0;
  }
  if (!strcmp(mode, "codec_of")) {
    unsigned long fcc, flags;
    int bits, ch, end, hlen;
    while (scanf("%lu %d %d %d %d %lu", &fcc, &bits, &ch, &end, &hlen, &flags) == 6) {
      const uint32_t f = (uint32_t)flags;
      uint8_t header[4];
      memcpy(header, &f, 4);
      Format fmt;
      if (codec_of((uint32_t)fcc, bits, ch, end, header, hlen, &fmt)) printf("%d %d %d %d\n", fmt.codec, fmt.label, fmt.block_align, fmt.sample_bytes);
      else printf("-1\n");
    }
    return 0;
  }
  if (!strcmp(mode, "payload")) {
    long long len, duration, align;
    while (scanf("%lld %lld %lld", &len, &duration, &align) == 3) printf("%lld\n", (long long)payload_of(len, duration, align));
    return 0;
  }
  return 2;
}
