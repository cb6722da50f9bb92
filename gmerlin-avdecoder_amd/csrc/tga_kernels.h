// tga_kernels.h — the three kernels of libmi_tga.so (include/mi_tga.h states the rules and cites upstream):
//   k_tga_scan    one lane a packet: the header (tga_format.h), the call's size and format, the length of plain data
//   k_tga_index   one wave a picture, run-length packets only: walks the packet chain once and leaves a checkpoint for
//                 every tile of kTile stored pixels; finds RLE, EOF and SHORT where upstream's loop would
//   k_tga_expand  one workgroup a (tile, picture): stages the tile's bytes of the stream in LDS, resolves its packets
//                 from the checkpoint, and writes every stored pixel where the orientation puts it
// Addresses are a 64-bit wave-uniform base (packet, picture) plus a 32-bit lane offset everywhere but in the scan, where
// every lane has a packet of its own.  Plain C++.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tga_format.h"

namespace mitga {

constexpr uint32_t kTile = 2048;      // stored pixels a checkpoint and a workgroup of k_tga_expand
constexpr uint32_t kThreads = 256;    // k_tga_expand
constexpr uint32_t kWindow = 1024;    // bytes of the stream k_tga_index holds in LDS: 64 lanes x 16
// the most bytes of the stream a tile can need, from the header of the packet that holds its first pixel: every packet
// that gives the tile k pixels costs at most 1 + k * sb bytes, the first one up to 127 pixels more
constexpr uint32_t tile_span(uint32_t sb) { return kTile * (sb + 1u) + 128u * sb; }
// the staging buffer: the span, up to 15 bytes in front of it (pieces of 16 bytes at aligned addresses), rounded up
constexpr uint32_t stage_bytes(uint32_t sb) { return (tile_span(sb) + 15u + 15u) / 16u * 16u; }

struct Call {
  const uint8_t* stream;
  const uint64_t* offsets;   // n, on the device
  const uint32_t* lengths;   // n
  uint32_t n, w, h, format, palette_entries;
  mi_tga_info* info;         // n descriptors: the scan writes them
  int32_t* status;           // n: the caller's
  uint2* index;              // n x tiles checkpoints: (byte of the packet's header from the data's start, its pixels before the tile)
  uint32_t tiles;
  uint8_t* pics;
  uint64_t pic_stride;
  const uint8_t* palettes;   // pal_entries x 4 bytes a palette (V:111-117), or nullptr
  uint32_t pal_entries;      // min(palette_entries, 256): no pixel byte indexes further
  const uint16_t* palette_of;  // n, or nullptr
};

__global__ __launch_bounds__(64) void k_tga_scan(const Call c) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= c.n) return;
  const uint8_t* p = c.stream + c.offsets[i];
  const uint32_t len = c.lengths[i];
  mi_tga_info d;
  int32_t st = parse_header(p, len, c.palette_entries, &d);
  if (st == MI_TGA_ST_OK) {
    if (d.width != c.w || d.height != c.h || d.format != c.format) st = MI_TGA_ST_MISMATCH;
    else if (!d.rle && (uint64_t)(len - d.data_offset) < (uint64_t)c.w * c.h * (d.pixel_depth >> 3)) st = MI_TGA_ST_EOF;  // T:345-346
  }
  d.status = st;
  c.info[i] = d;
  c.status[i] = st;
}

// T:385-433, without the copies: one wave, every value wave-uniform.  The stream comes through a window of kWindow bytes
// in LDS, fetched as 16-byte pieces at aligned addresses when the next header lies outside it.
__global__ __launch_bounds__(64) void k_tga_index(const Call c) {
  __shared__ uint4 win[kWindow / 16u];
  const uint32_t pic = blockIdx.x, lane = threadIdx.x;
  const mi_tga_info d = c.info[pic];
  if (d.status != MI_TGA_ST_OK || !d.rle) return;
  const uint8_t* data = c.stream + c.offsets[pic] + d.data_offset;
  const uint32_t len = c.lengths[pic] - d.data_offset, sb = d.pixel_depth >> 3, npix = c.w * c.h;
  const uint32_t mis = (uint32_t)((uintptr_t)data & 15u);  // window offsets count from the aligned address below the data
  const uint4* g = (const uint4*)(data - mis);
  const uint32_t pieces = (mis + len + 15u) / 16u;
  uint2* out = c.index + (uint64_t)pic * c.tiles;
  uint32_t wbase = 0, pos = 0, loaded = 0, tile = 0;
  int32_t st = MI_TGA_ST_OK;
  bool have = false;
  while (loaded < npix && pos < len) {
    const uint32_t apos = mis + pos;
    if (!have || apos - wbase >= kWindow) {
      wbase = apos & ~15u, have = true;
      const uint32_t piece = wbase / 16u + lane;
      __syncthreads();
      if (piece < pieces) win[lane] = g[piece];
      __syncthreads();
    }
    const uint32_t b = __builtin_amdgcn_readfirstlane(((const uint8_t*)win)[apos - wbase]);
    const uint32_t hdr = pos++, count = (b & 127u) + 1u, run = b & 128u;
    const uint32_t bytes = run ? sb : sb * count, end = loaded + count;
    const bool past = end > npix, cut = len - pos < bytes;
    if (past || cut) {  // one rarely taken branch; inside it the loop's order: a run reads its pixel, then its repeats
      // are counted; a raw packet's count is checked before its bytes are read
      st = run ? (cut ? MI_TGA_ST_EOF : MI_TGA_ST_RLE) : (past ? MI_TGA_ST_RLE : MI_TGA_ST_EOF);
      break;
    }
    if (tile * kTile < end) {  // (loaded <= tile * kTile, and a packet has at most 128 pixels: at most one tile begins in it)
      if (lane == 0) out[tile] = make_uint2(hdr, tile * kTile - loaded);
      tile++;
    }
    loaded = end, pos += bytes;
  }
  if (st == MI_TGA_ST_OK && loaded < npix) st = MI_TGA_ST_SHORT;  // T:398 with the stream empty
  if (st != MI_TGA_ST_OK && lane == 0) c.status[pic] = st, c.info[pic].status = st;  // (the expansion reads the descriptor's)
}

// floor(r / w) for r < 2^24 through the reciprocal, corrected
__device__ __forceinline__ uint32_t div_small(uint32_t r, uint32_t w, float rcp) {
  uint32_t q = (uint32_t)((float)r * rcp);
  if (q * w > r) q--;
  else if ((q + 1u) * w <= r) q++;
  return q;
}

// One tile of one packet: SB stored bytes a pixel, OB output bytes a pixel, MAPPED: SB is 1 and the pixel indexes a map.
template <uint32_t SB, bool MAPPED, uint32_t OB>
__device__ __forceinline__ void expand_tile(const Call& c, const mi_tga_info& d, uint32_t pic, uint32_t t, uint8_t* stage, uint16_t* src,
                                            uint8_t* lmap) {
  constexpr uint32_t kSpan = tile_span(SB), kStage = stage_bytes(SB);
  const uint32_t tid = threadIdx.x, w = c.w, npix = c.w * c.h;
  const uint32_t p0 = t * kTile, tile_n = npix - p0 < kTile ? npix - p0 : kTile;
  const uint8_t* pkt = c.stream + c.offsets[pic];
  const uint8_t* data = pkt + d.data_offset;
  const uint32_t dlen = c.lengths[pic] - d.data_offset;
  const bool rle = d.rle;

  // the tile's bytes of the stream: [first, last) of the data
  uint32_t first, last, skip = 0;
  if (rle) {
    const uint2* idx = c.index + (uint64_t)pic * c.tiles;
    const uint2 ck = idx[t];
    first = ck.x, skip = ck.y;
    last = first + kSpan;
    if (t + 1u < c.tiles) {  // up to the next tile's packet, and into it as far as this tile's pixels can reach
      const uint2 nx = idx[t + 1u];
      const uint32_t to = nx.x + (nx.y ? 1u + nx.y * SB : 0u);
      last = to < last ? to : last;
    }
    last = last < dlen ? last : dlen;
  } else {
    first = p0 * SB, last = first + tile_n * SB;
  }
  const uint32_t nbytes = last > first ? last - first : 0u;
  const uint32_t mis = (uint32_t)((uintptr_t)(data + first) & 15u);
  const uint4* g = (const uint4*)(data + first - mis);
  const uint32_t pieces = nbytes ? (mis + nbytes + 15u) / 16u : 0u;  // <= kStage / 16
  for (uint32_t k = tid; k < pieces; k += kThreads) ((uint4*)stage)[k] = g[k];

  uint32_t origin = 0, limit = 0;
  if (MAPPED) {
    origin = d.map_origin, limit = origin + d.map_length;  // T:894
    const uint32_t nent = limit < 256u ? limit : 256u;
    if (d.from_palette) {
      const uint8_t* pal = c.palettes + (uint64_t)(c.palette_of ? c.palette_of[pic] : 0u) * c.pal_entries * 4u;
      for (uint32_t k = tid; k < nent * OB; k += kThreads) lmap[k] = pal[k];
    } else {
      const uint8_t* map = pkt + d.map_offset;
      for (uint32_t k = tid; k < nent * OB; k += kThreads)
        if (k >= origin * OB) lmap[k] = map[k - origin * OB];  // T:326-328: the map's bytes begin at its origin
    }
  }
  __syncthreads();

  // the tile's packets, from the checkpoint: wave 0 steps the headers and notes where every pixel's bytes lie
  if (rle && tid < 64u) {
    int32_t pix = -(int32_t)skip;
    uint32_t pos = 0;
    while (pix < (int32_t)tile_n && pos < nbytes) {
      const uint32_t b = __builtin_amdgcn_readfirstlane(stage[mis + pos]);
      const uint32_t count = (b & 127u) + 1u, run = b >> 7;
      for (uint32_t l = tid; l < count; l += 64u) {
        const int32_t q = pix + (int32_t)l;
        if (q >= 0 && q < (int32_t)tile_n) src[q] = (uint16_t)(mis + pos + 1u + (run ? 0u : l * SB));
      }
      pix += (int32_t)count, pos += 1u + (run ? SB : SB * count);
    }
  }
  __syncthreads();

  uint8_t* out = c.pics + (uint64_t)pic * c.pic_stride;
  const float rcp = 1.0f / (float)w;
  const uint32_t y0 = p0 / w, x0 = p0 - y0 * w;
  for (uint32_t q = tid; q < tile_n; q += kThreads) {
    uint32_t off = rle ? src[q] : mis + q * SB;
    off = off < kStage - SB ? off : kStage - SB;
    uint8_t v[4];
    if (MAPPED) {
      const uint32_t i = stage[off];
      if (i >= limit) {  // T:894-895; upstream finds it whatever else the picture holds
        atomicExch(&c.status[pic], (int32_t)MI_TGA_ST_INDEX_RANGE);
        continue;
      }
      if (i < origin) {
        atomicCAS(&c.status[pic], (int32_t)MI_TGA_ST_OK, (int32_t)MI_TGA_ST_BELOW_ORIGIN);
        continue;
      }
#pragma unroll
      for (uint32_t k = 0; k < OB; k++) v[k] = lmap[i * OB + k];
    } else {
#pragma unroll
      for (uint32_t k = 0; k < OB; k++) v[k] = stage[off + k];
    }
    const uint32_t p = p0 + q;
    if (OB == 4u && p != npix - 1u) {  // T:1179-1181: every pixel but the last
      const uint8_t s = v[0];
      v[0] = v[2], v[2] = s;
    }
    const uint32_t r = x0 + q, dy = div_small(r, w, rcp);  // r < kTile + 65535
    uint32_t y = y0 + dy, x = r - dy * w;
    if (d.flip_x) x = w - 1u - x;
    if (d.flip_y) y = c.h - 1u - y;
    const uint32_t o = (y * w + x) * OB;
    if (OB == 4u) *(uint32_t*)(out + o) = (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
    else if (OB == 2u) *(uint16_t*)(out + o) = (uint16_t)((uint32_t)v[0] | (uint32_t)v[1] << 8);
    else {
#pragma unroll
      for (uint32_t k = 0; k < OB; k++) out[o + k] = v[k];
    }
  }
}

// blockIdx.x: the tile, blockIdx.y: the picture.  OB is the call's format; a packet stores OB bytes a pixel, or one byte
// that indexes a map of OB bytes an entry (there is no map of 8 bits: T:294).
template <uint32_t OB>
__global__ __launch_bounds__(kThreads) void k_tga_expand(const Call c) {
  __shared__ uint4 stage[stage_bytes(OB) / 16u];
  __shared__ uint16_t src[kTile];
  __shared__ uint8_t lmap[OB > 1u ? 256u * OB : 4u];
  const uint32_t t = blockIdx.x, pic = blockIdx.y;
  const mi_tga_info d = c.info[pic];
  if (d.status != MI_TGA_ST_OK) return;  // (scan's and index's: what this launch adds to c.status is not read here)
  if (OB > 1u && d.mapped) expand_tile<1u, true, OB>(c, d, pic, t, (uint8_t*)stage, src, lmap);
  else expand_tile<OB, false, OB>(c, d, pic, t, (uint8_t*)stage, src, lmap);
}

}  // namespace mitga
