// spu_format.h — the control section of a DVD subpicture as lib/subovl_dvd.c reads it (S:186-256, S:311-323;
// include/mi_spu.h states the rules): mi_spu_info (its layout is the public header's) and the one parser, which
// mi_spu_parse runs on the host and k_spu_scan runs on the device.  Plain C++ that g++ compiles too:
// tests/harness/spu_parse_san.cpp builds it with the sanitizers.
#pragma once
#include <stdint.h>

#include "../../include/mi_spu.h"

#if defined(__HIPCC__)
#define MI_SPU_HD __host__ __device__
#else
#define MI_SPU_HD
#endif

static_assert(sizeof(mi_spu_info) == 56, "mi_spu_info is the scan kernel's descriptor: 56 bytes");

namespace mispu {

MI_SPU_HD inline uint32_t be16(const uint8_t* p) { return (uint32_t)p[0] << 8 | (uint32_t)p[1]; }

// The control walk of the packet of `len` bytes at p for a video of w x h, in upstream's order; reads no byte at or
// past p + len.  Returns the status and leaves it in o->status.
MI_SPU_HD inline int32_t parse_control(const uint8_t* p, uint64_t len, int32_t w, int32_t h, mi_spu_info* o) {
  *o = mi_spu_info{};
  if (len < 4) return o->status = MI_SPU_ST_SHORT;
  uint64_t pos = be16(p + 2);  // S:186-190
  uint32_t ctrl_offset = (uint32_t)pos;
  o->ctrl_start = (uint16_t)pos;
#define MI_SPU_NEED(n)                                                    \
  do {                                                                    \
    if (pos > len || len - pos < (uint64_t)(n)) {                         \
      o->ctrl_end = (uint32_t)pos;                                        \
      return o->status = MI_SPU_ST_CTRL_RANGE;                            \
    }                                                                     \
  } while (0)
  for (;;) {
    MI_SPU_NEED(4);  // S:195-197: the date is skipped, next_ctrl_offset is read
    const uint32_t next = be16(p + pos + 2);
    pos += 4;
    o->sequences++;
    for (bool end = false; !end;) {  // S:201-251
      MI_SPU_NEED(1);
      const uint8_t cmd = p[pos];
      const uint8_t* q = p + pos + 1;
      switch (cmd) {
        case 0x03:
          MI_SPU_NEED(3);
          o->palette[3] = q[0] >> 4, o->palette[2] = q[0] & 15, o->palette[1] = q[1] >> 4, o->palette[0] = q[1] & 15;
          pos += 3;
          break;
        case 0x04:
          MI_SPU_NEED(3);
          o->alpha[3] = q[0] >> 4, o->alpha[2] = q[0] & 15, o->alpha[1] = q[1] >> 4, o->alpha[0] = q[1] & 15;
          pos += 3;
          break;
        case 0x05:
        case 0x85:
          MI_SPU_NEED(7);
          o->x1 = (uint16_t)(q[0] << 4 | q[1] >> 4), o->x2 = (uint16_t)((q[1] & 15) << 8 | q[2]);
          o->y1 = (uint16_t)(q[3] << 4 | q[4] >> 4), o->y2 = (uint16_t)((q[4] & 15) << 8 | q[5]);
          pos += 7;
          break;
        case 0x06:
          MI_SPU_NEED(5);
          o->offset1 = (uint16_t)be16(q), o->offset2 = (uint16_t)be16(q + 2);
          pos += 5;
          break;
        case 0xff:
          end = true;
          pos += 1;
          break;
        default:  // 00, 01, 02 and every unknown command: one byte
          pos += 1;
          break;
      }
    }
    if (ctrl_offset == next) break;  // S:253-255: pos is not set from next
    ctrl_offset = next;
  }
#undef MI_SPU_NEED
  o->ctrl_end = (uint32_t)pos;
  o->src_w = (int32_t)o->x2 - (int32_t)o->x1 + 1, o->src_h = (int32_t)o->y2 - (int32_t)o->y1 + 1;  // S:311-323
  o->dst_x = o->x1, o->dst_y = o->y1;
  if (o->dst_x + o->src_w > w) o->dst_x = w - o->src_w;
  if (o->dst_y + o->src_h > h) o->dst_y = h - o->src_h;
  if (o->src_w < 1 || o->src_w > w) return o->status = MI_SPU_ST_RECT;
  return o->status = MI_SPU_ST_OK;
}

}  // namespace mispu
