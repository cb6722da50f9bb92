// tga_format.h — the Targa header as lib/targa.c reads it (T:239-329; include/mi_tga.h states the rules): mi_tga_info
// (its layout is the public header's) and the one parser, which mi_tga_parse runs on the host and k_tga_scan runs on the
// device.  Plain C++ that g++ compiles too: tests/harness/tga_parse_san.cpp builds it with the sanitizers.
#pragma once
#include <stdint.h>

#include "../../include/mi_tga.h"

#if defined(__HIPCC__)
#define MI_TGA_HD __host__ __device__
#else
#define MI_TGA_HD
#endif

static_assert(sizeof(mi_tga_info) == 40, "mi_tga_info is the scan kernel's descriptor: 40 bytes");

namespace mitga {

MI_TGA_HD inline bool is_mapped_type(uint32_t t) { return t == 1 || t == 9; }  // tga_is_colormapped
MI_TGA_HD inline bool is_rle_type(uint32_t t) { return t == 9 || t == 10 || t == 11; }  // tga_is_rle
MI_TGA_HD inline uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }

// The header of the packet of `len` bytes at p, in upstream's order; reads no byte at or past p + len.  Returns the
// status and leaves it in o->status; what was not reached stays 0.
MI_TGA_HD inline int32_t parse_header(const uint8_t* p, uint64_t len, uint32_t palette_entries, mi_tga_info* o) {
  *o = mi_tga_info{};
  uint64_t pos = 0;
#define MI_TGA_NEED(n)                                  \
  do {                                                  \
    if (len - pos < (uint64_t)(n)) return o->status = MI_TGA_ST_EOF; \
  } while (0)
  MI_TGA_NEED(1);  // T:239
  o->id_length = p[0];
  pos = 1;
  MI_TGA_NEED(1);  // T:240-243
  o->map_type = p[1];
  pos = 2;
  if (o->map_type > 1) return o->status = MI_TGA_ST_CMAP_TYPE;
  MI_TGA_NEED(1);  // T:245-255
  o->image_type = p[2];
  pos = 3;
  if (o->image_type == 0) return o->status = MI_TGA_ST_NO_IMG;
  if (!(o->image_type >= 1 && o->image_type <= 3) && !(o->image_type >= 9 && o->image_type <= 11))
    return o->status = MI_TGA_ST_IMG_TYPE;
  MI_TGA_NEED(2);  // T:262-264
  o->map_origin = (uint16_t)le16(p + 3);
  pos = 5;
  MI_TGA_NEED(2);
  o->map_length = (uint16_t)le16(p + 5);
  pos = 7;
  MI_TGA_NEED(1);
  o->map_depth = p[7];
  pos = 8;
  const bool mapped = is_mapped_type(o->image_type);
  if (mapped && o->map_type == 0) {  // T:267-287
    if (o->map_length) o->map_type = 1;
    else if (!palette_entries) return o->status = MI_TGA_ST_CMAP_MISSING;
    else {
      o->map_origin = 0, o->map_length = (uint16_t)palette_entries, o->map_depth = 32;
      o->map_type = 1, o->from_palette = 1;
    }
  }
  if (o->map_type == 1 && mapped) {  // T:289-296
    if (o->map_length == 0) return o->status = MI_TGA_ST_CMAP_LENGTH;
    if (o->map_depth != 16 && o->map_depth != 24 && o->map_depth != 32) return o->status = MI_TGA_ST_CMAP_DEPTH;
  }
  MI_TGA_NEED(2);  // T:298-304
  o->x_origin = (uint16_t)le16(p + 8);
  pos = 10;
  MI_TGA_NEED(2);
  o->y_origin = (uint16_t)le16(p + 10);
  pos = 12;
  MI_TGA_NEED(2);
  o->width = (uint16_t)le16(p + 12);
  pos = 14;
  MI_TGA_NEED(2);
  o->height = (uint16_t)le16(p + 14);
  pos = 16;
  if (o->width == 0 || o->height == 0) return o->status = MI_TGA_ST_ZERO_SIZE;
  MI_TGA_NEED(1);  // T:306-309
  o->pixel_depth = p[16];
  pos = 17;
  const uint32_t d = o->pixel_depth;
  if ((d != 8 && d != 16 && d != 24 && d != 32) || (d != 8 && mapped)) return o->status = MI_TGA_ST_PIXEL_DEPTH;
  MI_TGA_NEED(1);  // T:311
  o->descriptor = p[17];
  pos = 18;
  MI_TGA_NEED(o->id_length);  // T:313-318
  pos += o->id_length;
  if (o->map_type == 1 && !o->from_palette) {  // T:320-329
    o->map_offset = (uint32_t)pos;
    const uint32_t bytes = (uint32_t)o->map_length * o->map_depth / 8u;
    MI_TGA_NEED(bytes);
    pos += bytes;
  }
#undef MI_TGA_NEED
  o->data_offset = (uint32_t)pos;
  const uint32_t depth = mapped ? o->map_depth : o->pixel_depth;  // V:170-183, V:53-77
  o->format = (uint8_t)(depth / 8u - 1u), o->bytes_per_pixel = (uint8_t)(depth / 8u);
  o->rle = is_rle_type(o->image_type), o->mapped = mapped;
  o->flip_x = (o->descriptor >> 4) & 1, o->flip_y = !((o->descriptor >> 5) & 1);  // V:220-245
  return o->status = MI_TGA_ST_OK;
}

}  // namespace mitga
