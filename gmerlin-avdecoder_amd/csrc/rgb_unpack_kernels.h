// rgb_unpack_kernels.h — the raw RGB family of QuickTime and AVI (lib/video_qtraw.c, lib/video_aviraw.c) on gfx950: the
// format table, which host and device code share, the mover with a row map k_rgb_move<Perm> (plain for QT24, AVI8_GRAY,
// AVI16, AVI24, AVI32; with a byte permute for QT16, MTV16, QT32) and the palette expansion k_rgb_palette<Bits> (QT1,
// QT2, QT4, QT8, AVI8).  include/mi_rgb.h states the formats with the upstream lines; DESIGN.md section 13 the kernel
// shapes.
//
// Addressing: a packet and a picture are found as a 64-bit wave-uniform base (blockIdx.y * stride) plus a 32-bit lane
// offset inside the frame; the host layer refuses packets and pictures of 2^31 bytes or more.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "yuv_unpack_kernels.h"  // get16, byte_at

namespace mirgb {

using miyuv::byte_at;
using miyuv::get16;

enum Codec : int { kQt1 = 0, kQt2, kQt4, kQt8, kQt16, kQt24, kQt32, kAvi8, kAvi8Gray, kAvi16, kMtv16, kAvi24, kAvi32, kCodecs };
enum Kind : int { kMove, kSwap16, kRot32, kPalette };  // the kernel: k_rgb_move<None / Swap16 / Rot32>, k_rgb_palette<bits>

// ---- the format table ----
struct Format {
  const char* name;
  Kind kind;
  uint32_t bits;     // of a pixel in the packet
  uint32_t bpp;      // bytes of a pixel in the picture
  uint32_t w_mult;   // the widths upstream's row loop stays inside the row with: multiples of this
  uint32_t row_pad;  // a packet row is made even (2: video_qtraw.c:365-366) or padded to 4 (video_aviraw.c:273-279)
  bool bottom_up;    // video_aviraw.c:183-192
  uint32_t palette;  // entries, 0 without
};
constexpr Format kFormats[kCodecs] = {
    {"QT1", kPalette, 1, 3, 8, 2, false, 2},     {"QT2", kPalette, 2, 3, 4, 2, false, 4},
    {"QT4", kPalette, 4, 3, 2, 2, false, 16},    {"QT8", kPalette, 8, 3, 1, 2, false, 256},
    {"QT16", kSwap16, 16, 2, 1, 2, false, 0},    {"QT24", kMove, 24, 3, 1, 2, false, 0},
    {"QT32", kRot32, 32, 4, 1, 2, false, 0},     {"AVI8", kPalette, 8, 3, 1, 4, true, 256},
    {"AVI8_GRAY", kMove, 8, 1, 1, 4, true, 0},   {"AVI16", kMove, 16, 2, 1, 4, true, 0},
    {"MTV16", kSwap16, 16, 2, 1, 4, true, 0},    {"AVI24", kMove, 24, 3, 1, 4, true, 0},
    {"AVI32", kMove, 32, 4, 1, 4, true, 0},
};

// what a codec makes of a size it accepts: packet rows of in_bytes used bytes, in_stride apart; picture rows of row_bytes
struct Shape {
  uint64_t packet_bytes, picture_bytes;
  uint32_t w, h, in_bytes, in_stride, row_bytes;
};
constexpr Shape shape_of(int codec, uint64_t w, uint64_t h) {
  const Format& f = kFormats[codec];
  Shape s{};
  const uint64_t used = (w * f.bits + 7) / 8, stride = (used + f.row_pad - 1) / f.row_pad * f.row_pad;
  s.w = (uint32_t)w, s.h = (uint32_t)h, s.in_bytes = (uint32_t)used, s.in_stride = (uint32_t)stride;
  s.row_bytes = (uint32_t)(w * f.bpp);
  s.packet_bytes = stride * h, s.picture_bytes = w * f.bpp * h;
  return s;
}

constexpr uint32_t kThreads = 256, kMaxGridX = 4096;

// ---- the mover with a row map: padded rows of the packet -> tight rows of the picture, for AVI in reverse order, each
// aligned 4 (Rot32) or 2 (Swap16) bytes permuted on the way ----
// One item is one 16-byte aligned piece of the picture.  A piece that lies whole inside one row is one 16-byte load (by
// words or bytes where the source is not aligned: get16) and one 16-byte store; the pieces across the ends of rows and
// the picture's last go byte by byte and write the picture's own bytes only.  (Rows that lie back to back in the packet
// in the picture's order are one row to this kernel: the host says so.)
struct None {  // video_qtraw.c:137-143, video_aviraw.c:62-89, :108-118
  __device__ static uint32_t word(uint32_t x) { return x; }
  __device__ static uint32_t source(uint32_t col) { return col; }
};
struct Swap16 {  // video_qtraw.c:120-135 (on a little-endian host), video_aviraw.c:91-104
  __device__ static uint32_t word(uint32_t x) { return __builtin_amdgcn_perm(x, x, 0x02030001u); }
  __device__ static uint32_t source(uint32_t col) { return col ^ 1u; }
};
struct Rot32 {  // video_qtraw.c:145-160: A R G B -> R G B A
  __device__ static uint32_t word(uint32_t x) { return __builtin_amdgcn_perm(x, x, 0x00030201u); }
  __device__ static uint32_t source(uint32_t col) { return (col & ~3u) | ((col + 1u) & 3u); }
};

struct MoveGeo {
  uint32_t items, rows, row_bytes, in_stride, bytes;  // bytes: the picture's
  uint32_t bottom_up;
};
inline MoveGeo move_geo(int codec, const Shape& s) {
  MoveGeo g{};
  const bool one_row = s.in_stride == s.row_bytes && !kFormats[codec].bottom_up;
  g.bytes = (uint32_t)s.picture_bytes;
  g.rows = one_row ? 1u : s.h, g.row_bytes = one_row ? g.bytes : s.row_bytes, g.in_stride = one_row ? g.bytes : s.in_stride;
  g.bottom_up = kFormats[codec].bottom_up;
  g.items = (g.bytes + 15u) / 16u;
  return g;
}

template <class P>
__global__ __launch_bounds__(256) void k_rgb_move(const uint8_t* __restrict__ packets, uint64_t packet_stride,
                                                  uint8_t* __restrict__ pics, uint64_t pic_stride, MoveGeo g) {
  const uint8_t* __restrict__ in = packets + (uint64_t)blockIdx.y * packet_stride;
  uint8_t* __restrict__ out = pics + (uint64_t)blockIdx.y * pic_stride;
  for (uint32_t item = blockIdx.x * kThreads + threadIdx.x; item < g.items; item += gridDim.x * kThreads) {
    const uint32_t d = item * 16u, hi = d + 16u < g.bytes ? d + 16u : g.bytes;
    uint32_t row = g.rows == 1 ? 0u : d / g.row_bytes, col = d - row * g.row_bytes;
    if (hi - d == 16u && col + 16u <= g.row_bytes) {
      const uint4 v = get16(in, (g.bottom_up ? g.rows - 1u - row : row) * g.in_stride + col);
      *(uint4*)(out + d) = make_uint4(P::word(v.x), P::word(v.y), P::word(v.z), P::word(v.w));
    } else {
      for (uint32_t b = d; b < hi; b++) {
        out[b] = in[(g.bottom_up ? g.rows - 1u - row : row) * g.in_stride + P::source(col)];
        if (++col == g.row_bytes) col = 0, row++;
      }
    }
  }
}

// ---- the palette expansion: 1, 2, 4 or 8 bits a pixel -> 3 bytes a pixel ----
// The picture is tight, so pixel p of the frame (row p / w, column p % w) is output bytes 3p .. 3p + 2.  A CHUNK is
// kChunkPixels consecutive pixels of the frame, 12,288 output bytes from a multiple of 16; a workgroup takes chunks in a
// stride loop that is uniform over its lanes.  A lane expands 16 consecutive pixels: where they lie in one row it loads
// their 2, 4, 8 or 16 packet bytes at once and takes the indices out of registers; at a row's end (w is no multiple of
// 16) and behind the picture's last pixel it walks pixel by pixel.  The colours come from the packet's palette in LDS
// (256 x R G B 0, reduced on the host); the lane's 48 bytes go to LDS as three 16-byte pieces, and after a barrier lane t
// stores pieces t, t + 256, t + 512 of the chunk: a wave's stores are 1,024 consecutive bytes.  A row's tail and the next
// row's head share a piece like any two neighbours; only the picture's last piece can be partial and goes byte by byte.
constexpr uint32_t kChunkPixels = kThreads * 16u, kChunkPieces = kChunkPixels * 3u / 16u;

struct PaletteGeo {
  uint32_t chunks, pixels, w, h, in_stride, bottom_up;
};
inline PaletteGeo palette_geo(int codec, const Shape& s) {
  PaletteGeo g{};
  g.pixels = s.w * s.h, g.w = s.w, g.h = s.h, g.in_stride = s.in_stride, g.bottom_up = kFormats[codec].bottom_up;
  g.chunks = (g.pixels + kChunkPixels - 1u) / kChunkPixels;
  return g;
}

// 2 * Bits bytes of a packet at an offset of any alignment, little-endian, into v[0 .. Bits / 2] (Bits 1: v[0]'s low half)
template <int Bits>
__device__ __forceinline__ void load_indices(uint32_t* v, const uint8_t* __restrict__ in, uint32_t off) {
  if constexpr (Bits == 8) {
    const uint4 q = get16(in, off);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else if constexpr (Bits == 1) {
    v[0] = (uint32_t)in[off] | (uint32_t)in[off + 1] << 8;
  } else {
    constexpr int kWords = Bits / 2;  // 1 or 2
    if ((off & 3u) == 0) {
#pragma unroll
      for (int i = 0; i < kWords; i++) v[i] = *(const uint32_t*)(in + off + 4 * i);
    } else {
#pragma unroll
      for (int i = 0; i < kWords; i++)
        v[i] = (uint32_t)in[off + 4 * i] | (uint32_t)in[off + 4 * i + 1] << 8 | (uint32_t)in[off + 4 * i + 2] << 16 |
               (uint32_t)in[off + 4 * i + 3] << 24;
    }
  }
}

template <int Bits>
__global__ __launch_bounds__(256) void k_rgb_palette(const uint8_t* __restrict__ packets, uint64_t packet_stride,
                                                     uint8_t* __restrict__ pics, uint64_t pic_stride,
                                                     const uint32_t* __restrict__ palettes, const uint16_t* __restrict__ palette_of,
                                                     PaletteGeo g) {
  __shared__ uint32_t pal[256];
  __shared__ uint4 stage[kChunkPieces];
  const uint8_t* __restrict__ in = packets + (uint64_t)blockIdx.y * packet_stride;
  uint8_t* __restrict__ out = pics + (uint64_t)blockIdx.y * pic_stride;
  const uint32_t t = threadIdx.x, bytes = 3u * g.pixels;
  pal[t] = palettes[(palette_of ? (uint32_t)palette_of[blockIdx.y] : 0u) * 256u + t];
  constexpr uint32_t kMask = (1u << Bits) - 1u;
  for (uint32_t chunk = blockIdx.x; chunk < g.chunks; chunk += gridDim.x) {
    __syncthreads();  // the palette is there; the last chunk's pieces have been read
    const uint32_t p0 = chunk * kChunkPixels + 16u * t;
    uint32_t row = p0 / g.w, x = p0 - row * g.w;
    uint32_t c[16];
    if (p0 + 16u <= g.pixels && x + 16u <= g.w) {
      uint32_t v[4];
      load_indices<Bits>(v, in, (g.bottom_up ? g.h - 1u - row : row) * g.in_stride + x * Bits / 8u);
#pragma unroll
      for (int i = 0; i < 16; i++) c[i] = pal[(byte_at(v, i * Bits / 8) >> (8 - Bits - i * Bits % 8)) & kMask];
    } else {
#pragma unroll
      for (int i = 0; i < 16; i++) {
        c[i] = 0;
        if (p0 + i < g.pixels) {
          const uint32_t byte = in[(g.bottom_up ? g.h - 1u - row : row) * g.in_stride + x * Bits / 8u];
          c[i] = pal[(byte >> (8u - Bits - x * Bits % 8u)) & kMask];
          if (++x == g.w) x = 0, row++;
        }
      }
    }
    // four pixels R G B 0 -> three words of R G B R G B ...
#pragma unroll
    for (int q = 0; q < 3; q++) {
      uint32_t d[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int j = 4 * q + k, px = j / 3 * 4, part = j % 3;  // word j of the lane's 12
        d[k] = part == 0 ? c[px] | c[px + 1] << 24 : part == 1 ? c[px + 1] >> 8 | c[px + 2] << 16 : c[px + 2] >> 16 | c[px + 3] << 8;
      }
      stage[3u * t + q] = make_uint4(d[0], d[1], d[2], d[3]);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) {
      const uint32_t piece = k * kThreads + t, at = chunk * (kChunkPixels * 3u) + 16u * piece;
      if (at + 16u <= bytes) {
        *(uint4*)(out + at) = stage[piece];
      } else if (at < bytes) {
        const uint8_t* s = (const uint8_t*)&stage[piece];
        for (uint32_t b = 0; at + b < bytes; b++) out[at + b] = s[b];
      }
    }
  }
}

}  // namespace mirgb
