// spu_parse_san.cpp — the control parser of libmi_spu.so (csrc/spu_format.h) under AddressSanitizer and
// UndefinedBehaviorSanitizer, as a program of its own: tests/test_spu_parse_asan_cpu.py builds it with g++ and runs it as a
// child process.  Every packet is parsed from a heap block of exactly its length, so a read at or past the end is found:
// every truncation of a few packets, every command byte in front of every count of operand bytes, control offsets that
// point anywhere, and bytes nobody wrote.  Prints one line a group and "ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../gmerlin-avdecoder_amd/csrc/spu_format.h"

namespace {
typedef std::vector<uint8_t> Bytes;

// parses the first `len` bytes from a block of exactly that size; returns the status
int parse_exact(const Bytes& p, size_t len, int w, int h, mi_spu_info* info) {
  uint8_t* block = (uint8_t*)malloc(len ? len : 1);
  if (len) memcpy(block, p.data(), len);
  const int st = mispu::parse_control(len ? block : block + 1, len, w, h, info);  // (len 0: a pointer that may not be read at all)
  free(block);
  if (st != info->status) exit(2);
  if (st < MI_SPU_ST_OK || st > MI_SPU_ST_RECT) exit(3);
  if (st != MI_SPU_ST_SHORT && info->ctrl_end > len && info->ctrl_end != info->ctrl_start) exit(4);
  if (st == MI_SPU_ST_OK && (info->src_w < 1 || info->src_w > w || info->ctrl_end > len || info->sequences < 1)) exit(5);
  return st;
}

void put(Bytes& p, std::initializer_list<int> b) {
  for (int v : b) p.push_back((uint8_t)v);
}

// size, control offset, `data` bytes of fields, then sequences
Bytes packet(size_t data, const std::vector<Bytes>& seqs) {
  Bytes p;
  const size_t ctrl = 4 + data;
  put(p, {0, 0, (int)(ctrl >> 8), (int)(ctrl & 255)});
  p.resize(ctrl, 0x5a);
  size_t at = ctrl;
  for (size_t k = 0; k < seqs.size(); k++) {
    const size_t next = k + 1 < seqs.size() ? at + 4 + seqs[k].size() : at;
    put(p, {0, (int)k, (int)(next >> 8), (int)(next & 255)});
    p.insert(p.end(), seqs[k].begin(), seqs[k].end());
    at += 4 + seqs[k].size();
  }
  return p;
}
}  // namespace

int main() {
  mi_spu_info info;
  const Bytes usual = {0x03, 0x32, 0x10, 0x04, 0xff, 0xf0, 0x05, 0x00, 0x00, 0x13, 0x00, 0x00, 0x05, 0x06, 0x00, 0x04, 0x00, 0x0a, 0x01, 0xff};
  const Bytes second = {0x02, 0x03, 0x12, 0x34, 0x04, 0x56, 0x78, 0x85, 0x01, 0x00, 0x20, 0x00, 0x10, 0x09, 0xff};
  const Bytes unknown = {0x07, 0x04, 0x43, 0x21, 0x00, 0x05, 0x00, 0x00, 0x07, 0x00, 0x00, 0x03, 0xff};
  const std::vector<Bytes> packets = {packet(12, {usual}),           packet(12, {usual, second}), packet(0, {unknown}),
                                      packet(40, {usual, usual, second}), packet(1, {second}),         packet(300, {unknown, usual})};
  int truncations = 0;
  for (const Bytes& p : packets) {
    if (parse_exact(p, p.size(), 64, 32, &info) != MI_SPU_ST_OK) return 6;
    const size_t end = info.ctrl_end;
    for (size_t len = 0; len <= p.size(); len++, truncations++) {
      const int st = parse_exact(p, len, 64, 32, &info);
      const int want = len < 4 ? MI_SPU_ST_SHORT : len < end ? MI_SPU_ST_CTRL_RANGE : MI_SPU_ST_OK;
      if (st != want) return 7;
    }
  }
  printf("truncations %d\n", truncations);
  // every command byte, with 0 to 8 bytes behind it and no ff: the walk must stop at the end; and with an ff behind them
  int commands = 0;
  for (int cmd = 0; cmd < 256; cmd++)
    for (int operands = 0; operands <= 8; operands++)
      for (int closed = 0; closed < 2; closed++) {
        Bytes seq = {(uint8_t)cmd};
        for (int k = 0; k < operands; k++) seq.push_back((uint8_t)(0x11 * k + 1));
        if (closed) seq.push_back(0xff);
        const Bytes p = packet(3, {seq});
        const int st = parse_exact(p, p.size(), 4096, 4096, &info);
        if (!closed && cmd != 0xff && st != MI_SPU_ST_CTRL_RANGE) return 8;
        commands++;
      }
  printf("commands %d\n", commands);
  // control offsets that point anywhere in and past a short packet, and every next offset
  int offsets = 0;
  for (int ctrl = 0; ctrl < 70000; ctrl += (ctrl < 80 ? 1 : 997))
    for (size_t len = 4; len <= 64; len += 5) {
      Bytes p(len, 0xff);
      p[0] = 0, p[1] = (uint8_t)len, p[2] = (uint8_t)((ctrl >> 8) & 255), p[3] = (uint8_t)(ctrl & 255);
      parse_exact(p, len, 720, 576, &info);
      offsets++;
    }
  printf("offsets %d\n", offsets);
  // bytes nobody wrote
  uint32_t seed = 12345;
  int noise = 0;
  for (int k = 0; k < 20000; k++, noise++) {
    seed = seed * 1664525u + 1013904223u;
    Bytes p(seed >> 26);
    for (uint8_t& b : p) {
      seed = seed * 1664525u + 1013904223u;
      b = (uint8_t)(seed >> 24);
      if ((seed >> 8 & 7) == 0) b = 0xff;
    }
    if (p.size() >= 4) p[2] = 0, p[3] = (uint8_t)(p[3] % p.size());
    parse_exact(p, p.size(), 720, 576, &info);
  }
  printf("noise %d\n", noise);
  printf("ok\n");
  return 0;
}
