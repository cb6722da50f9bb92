// tga_parse_san.cpp — the header parser of libmi_tga.so (csrc/tga_format.h) under AddressSanitizer and
// UndefinedBehaviorSanitizer, as a program of its own: tests/test_tga_parse_asan_cpu.py builds it with g++ and runs it as a
// child process.  Every packet is parsed from a heap block of exactly its length, so a read at or past the end is found;
// every truncation 0..len of a few packets, and headers with extreme fields.  Prints one line a group and "ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../gmerlin-avdecoder_amd/csrc/tga_format.h"

namespace {
std::vector<uint8_t> header(int type, int w, int h, int depth, int desc, int id_len, int map_type, int origin, int length, int map_depth) {
  const int f[18] = {id_len, map_type, type, origin & 255, origin >> 8, length & 255, length >> 8, map_depth, 0, 0, 0, 0,
                     w & 255, w >> 8, h & 255, h >> 8, depth, desc};
  return std::vector<uint8_t>(f, f + 18);
}

// parses the first `len` bytes from a block of exactly that size; returns the status
int parse_exact(const std::vector<uint8_t>& p, size_t len, uint32_t entries, mi_tga_info* info) {
  uint8_t* block = (uint8_t*)malloc(len ? len : 1);
  if (len) memcpy(block, p.data(), len);
  const int st = mitga::parse_header(len ? block : block + 1, len, entries, info);  // (len 0: a pointer that may not be read at all)
  free(block);
  if (st != info->status) exit(2);
  if (st == MI_TGA_ST_OK && (info->data_offset > len || info->map_offset > info->data_offset)) exit(3);
  return st;
}
}  // namespace

int main() {
  mi_tga_info info;
  // a few packets with an id and a map, every truncation
  const int kinds[][7] = {{2, 24, 0, 0, 0, 0, 0}, {1, 8, 1, 3, 10, 24, 7}, {9, 8, 1, 0, 256, 32, 255}, {10, 32, 1, 0, 5, 15, 1}, {11, 8, 0, 0, 0, 0, 0},
                          {1, 8, 0, 0, 2, 16, 3}};
  int truncations = 0;
  for (const auto& k : kinds) {
    std::vector<uint8_t> p = header(k[0], 5, 3, k[1], 0x20, k[6], k[2], k[3], k[4], k[5]);
    p.resize(p.size() + (size_t)k[6] + (size_t)k[4] * (size_t)k[5] / 8u + 5u * 3u * 4u, 0x5a);
    const int whole = parse_exact(p, p.size(), 0, &info);
    if (whole != MI_TGA_ST_OK) return 4;
    for (size_t len = 0; len <= p.size(); len++, truncations++) {
      const int st = parse_exact(p, len, 0, &info);
      if (st != MI_TGA_ST_OK && st != MI_TGA_ST_EOF) return 5;
      if (st == MI_TGA_ST_OK && len < 18u + (size_t)k[6] + (size_t)k[4] * (size_t)k[5] / 8u) return 6;
    }
  }
  printf("truncations %d\n", truncations);
  // extreme fields: every value of the byte fields that decide something, the largest 16-bit fields, with and without a palette
  int extremes = 0;
  for (int type : {0, 1, 2, 3, 4, 8, 9, 10, 11, 12, 255})
    for (int map_type = 0; map_type < 3; map_type++)
      for (int depth : {0, 8, 15, 16, 24, 32, 255})
        for (int map_depth : {0, 8, 15, 16, 24, 32, 255})
          for (int length : {0, 1, 65535})
            for (uint32_t entries : {0u, 1u, 65535u}) {
              std::vector<uint8_t> p = header(type, 65535, 65535, depth, 0xff, 255, map_type, 65535, length, map_depth);
              const int st = parse_exact(p, p.size(), entries, &info);
              if (st == MI_TGA_ST_OK) return 7;  // (255 id bytes are missing)
              if (st == MI_TGA_ST_EOF) {  // the header is good: with the id and the largest map this header can ask for
                p.resize(18u + 255u + (size_t)length * (size_t)map_depth / 8u, 1);
                const int whole = parse_exact(p, p.size(), entries, &info);
                if (whole != MI_TGA_ST_OK || info.data_offset > p.size()) return 8;
                const size_t data = info.data_offset;  // one byte less than the header, the id and the map take
                if (parse_exact(p, data - 1u, entries, &info) != MI_TGA_ST_EOF) return 9;
              }
              extremes++;
            }
  printf("extremes %d\n", extremes);
  printf("ok\n");
  return 0;
}
