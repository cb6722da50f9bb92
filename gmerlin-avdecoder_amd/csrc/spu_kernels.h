// spu_kernels.h — the two kernels of libmi_spu.so (include/mi_spu.h states the rules and cites upstream):
//   k_spu_scan    one lane a packet: the control walk (spu_format.h), the rectangle, the info
//   k_spu_decode  one wave a (packet, field): a field's lines are one serial chain, line k + 1 starts where line k ended,
//                 so the two fields of all n packets walk at once.  Inside a line the walk is lane-parallel over a window
//                 of 64 nibbles: lane p classifies the code that would start at nibble p, a wave scan over the
//                 four-state "nibbles left of the code I am in" maps marks the true starts, a second scan sums their
//                 lengths, and the first start at which x reaches the width cuts the window.  The line's runs go to LDS
//                 and the row leaves as 16-byte pieces a lane over the whole W * 4 bytes, zeros past the width included.
// Addresses are a 64-bit wave-uniform base (packet, picture) plus a 32-bit lane offset everywhere but in the scan, where
// every lane has a packet of its own.  Plain C++.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spu_format.h"

namespace mispu {

constexpr uint32_t kWindow = 1024;  // bytes of the packet k_spu_decode holds in LDS: 64 lanes x 16
constexpr uint32_t kStep = 34;      // bytes one step of 64 nibbles can look at: 64 + 3 nibbles from any nibble phase
constexpr uint32_t kMaxW = 4096;    // the widest frame; a line has at most as many runs as pixels
constexpr uint32_t kFill = 2 * kMaxW;  // what a fill code counts for: reaches any width, and 64 of them fit 32 bits

struct Call {
  const uint8_t* stream;
  const uint64_t* offsets;     // n, on the device
  const uint32_t* lengths;     // n
  uint32_t n, w, h;
  mi_spu_info* info;           // n: the caller's; the scan writes them, the decoder the lines and DATA_RANGE
  uint8_t* pics;
  uint64_t pic_stride;
  const uint32_t* palettes;    // 16 entries a palette, on the device
  const uint16_t* palette_of;  // n, or nullptr
};

__global__ __launch_bounds__(64) void k_spu_scan(const Call c) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= c.n) return;
  mi_spu_info d;
  parse_control(c.stream + c.offsets[i], c.lengths[i], (int32_t)c.w, (int32_t)c.h, &d);
  c.info[i] = d;
}

// g after f, both maps of the four states to the four states, two bits an entry
__device__ __forceinline__ uint32_t compose(uint32_t f, uint32_t g) {
  uint32_t r = 0;
#pragma unroll
  for (uint32_t s = 0; s < 4u; s++) r |= ((g >> (2u * ((f >> (2u * s)) & 3u))) & 3u) << (2u * s);
  return r;
}

__device__ __forceinline__ uint32_t pick(uint32_t c, uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3) {
  return c == 0u ? p0 : c == 1u ? p1 : c == 2u ? p2 : p3;
}

// Row `rowpix / w` of the slot: the `nruns` runs of LDS (end of the run << 2 | colour, ends ascending, the last one
// `width`) as pixels, zeros from `width` to w.  A row begins at a multiple of 4 bytes: the pieces are the aligned 16
// bytes the row touches, the first and the last stored a pixel at a time where they are shared with a neighbouring row.
__device__ __forceinline__ void store_row(uint8_t* slot, uint32_t rowpix, uint32_t w, uint32_t width, const uint16_t* runs, uint32_t nruns,
                                          uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3) {
  const uint32_t shift = rowpix & 3u;
  uint32_t* base = (uint32_t*)slot + (rowpix - shift);
  const uint32_t pieces = (shift + w + 3u) / 4u;
  const uint32_t top = nruns ? 1u << (31u - (uint32_t)__builtin_clz(nruns)) : 0u;
  for (uint32_t j = threadIdx.x; j < pieces; j += 64u) {
    const int32_t x0 = (int32_t)(j * 4u) - (int32_t)shift;
    uint32_t px[4] = {0u, 0u, 0u, 0u};
    if (x0 < (int32_t)width) {
      const uint32_t xq = x0 < 0 ? 0u : (uint32_t)x0;
      uint32_t r = 0;  // the runs that end at or before xq: the index of the run xq lies in
      for (uint32_t s = top; s; s >>= 1) {
        const uint32_t t = r + s;
        if (t <= nruns && (uint32_t)(runs[t - 1u] >> 2) <= xq) r = t;
      }
      uint32_t cur = runs[r];
#pragma unroll
      for (int32_t k = 0; k < 4; k++) {
        const int32_t x = x0 + k;
        if (x >= 0 && x < (int32_t)width) {
          px[k] = pick(cur & 3u, p0, p1, p2, p3);
          if ((uint32_t)x + 1u >= (cur >> 2) && (uint32_t)x + 1u < width) cur = runs[++r];
        }
      }
    }
    if (x0 >= 0 && (uint32_t)x0 + 4u <= w) *(uint4*)(base + j * 4u) = make_uint4(px[0], px[1], px[2], px[3]);
    else {
#pragma unroll
      for (int32_t k = 0; k < 4; k++)
        if (x0 + k >= 0 && x0 + k < (int32_t)w) base[j * 4u + (uint32_t)k] = px[k];
    }
  }
}

// blockIdx.x: the field, blockIdx.y: the packet.  S:132-147 over S:77-130.
__global__ __launch_bounds__(64) void k_spu_decode(const Call c) {
  __shared__ uint4 win[kWindow / 16u];
  __shared__ uint16_t runs[kMaxW];
  const uint32_t field = blockIdx.x, pic = blockIdx.y, lane = threadIdx.x;
  const mi_spu_info d = c.info[pic];
  if (d.status != MI_SPU_ST_OK) return;  // (the scan's, or the other field's DATA_RANGE)
  const uint8_t* pkt = c.stream + c.offsets[pic];
  const uint32_t plen = c.lengths[pic];
  const uint32_t w = c.w, width = (uint32_t)d.x2 - (uint32_t)d.x1 + 1u;  // 1 .. w: the scan refused the others
  const uint32_t off = field ? d.offset2 : d.offset1;                                               // S:294-304
  const int32_t flen = field ? (int32_t)d.ctrl_start - (int32_t)d.offset2 : (int32_t)d.offset2 - (int32_t)d.offset1;
  const uint32_t max_lines = c.h / 2u;
  uint32_t pal[4];  // S:260-266
  {
    const uint32_t* ifo = c.palettes + 16u * (c.palette_of ? (uint32_t)c.palette_of[pic] : 0u);
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
      const uint32_t e = ifo[d.palette[k] & 15u];
      pal[k] = ((e >> 16) & 255u) | ((e >> 8) & 255u) << 8 | (e & 255u) << 16 | ((uint32_t)d.alpha[k] * 17u) << 24;
    }
  }
  uint8_t* slot = c.pics + (uint64_t)pic * c.pic_stride;
  const uint32_t mis = (uint32_t)((uintptr_t)pkt & 15u);  // window offsets count from the aligned address below the packet
  const uint4* g = (const uint4*)(pkt - mis);
  const uint32_t pieces = (mis + plen + 15u) / 16u;
  const uint8_t* wb = (const uint8_t*)win;
  uint32_t wbase = 0, pos = 0, lines = 0;
  bool have = false, bad = false;

  while ((int32_t)pos < flen && lines < max_lines && !bad) {
    uint32_t q = 2u * (off + pos);  // the nibble of the packet the window begins at: a code's first
    uint32_t x = 0, nruns = 0;
    for (;;) {
      const uint32_t apos = mis + (q >> 1);
      if (!have || apos + kStep > wbase + kWindow) {
        wbase = apos & ~15u, have = true;
        const uint32_t piece = wbase / 16u + lane;
        __syncthreads();
        if (piece < pieces) win[lane] = g[piece];
        __syncthreads();
      }
      // lane p: the code that would start at nibble q + p.  A byte at or past the packet's length reads as 0.
      const uint32_t qp = q + lane, bi = qp >> 1, li = mis + bi - wbase;
      const uint32_t t = (bi < plen ? (uint32_t)wb[li] : 0u) << 16 | (bi + 1u < plen ? (uint32_t)wb[li + 1u] : 0u) << 8 |
                         (bi + 2u < plen ? (uint32_t)wb[li + 2u] : 0u);
      const uint32_t v16 = (t >> ((qp & 1u) ? 4u : 8u)) & 0xffffu, n0 = v16 >> 12;
      uint32_t clen, v;  // S:92-108
      if (n0 >= 4u) clen = 1u, v = n0;
      else if (n0) clen = 2u, v = v16 >> 8;
      else if ((v16 >> 4) >= 0x40u) clen = 3u, v = v16 >> 4;
      else clen = 4u, v = v16;
      const bool fill = clen == 4u && v < 4u;
      // state: the nibbles still to skip before the next code starts.  Nibble p maps 0 to clen - 1 and s to s - 1.
      uint32_t m = 0x90u | (clen - 1u);
#pragma unroll
      for (uint32_t s = 1; s < 64u; s <<= 1) {
        const uint32_t before = (uint32_t)__shfl_up((int)m, s);
        if (lane >= s) m = compose(before, m);
      }
      const uint32_t state_in = (uint32_t)__shfl_up((int)(m & 3u), 1u);
      const bool start = lane == 0u || state_in == 0u;
      uint32_t xs = start ? (fill ? kFill : v >> 2) : 0u;  // x after the code, from here on
#pragma unroll
      for (uint32_t s = 1; s < 64u; s <<= 1) {
        const uint32_t before = (uint32_t)__shfl_up((int)xs, s);
        if (lane >= s) xs += before;
      }
      xs += x;
      const uint64_t ends = __ballot(start && xs >= width);  // S:126
      const uint32_t e = ends ? (uint32_t)__ffsll((unsigned long long)ends) - 1u : 64u;
      const bool used = start && lane <= e;
      if (__ballot(used && ((qp + clen - 1u) >> 1) >= plen)) {  // upstream would read outside the packet
        bad = true;
        break;
      }
      const uint64_t um = __ballot(used);
      if (used) {
        const uint32_t rank = (uint32_t)__popcll(um & ((1ull << lane) - 1ull));
        runs[nruns + rank] = (uint16_t)((xs < width ? xs : width) << 2 | (v & 3u));  // S:114-118
      }
      nruns += (uint32_t)__popcll(um);
      if (e < 64u) {  // S:127: the next line starts at the next whole byte
        const uint32_t qend = q + e + (uint32_t)__builtin_amdgcn_readlane((int)clen, (int)e);
        pos = ((qend + 1u) >> 1) - off;
        break;
      }
      x = (uint32_t)__builtin_amdgcn_readlane((int)xs, 63);
      q += 64u + ((uint32_t)__builtin_amdgcn_readlane((int)m, 63) & 3u);
    }
    if (bad) break;
    __syncthreads();
    store_row(slot, (field + 2u * lines) * w, w, width, runs, nruns, pal[0], pal[1], pal[2], pal[3]);
    __syncthreads();
    lines++;
  }
  if (bad) {
    if (lane == 0u) c.info[pic].status = MI_SPU_ST_DATA_RANGE;
    return;
  }
  for (uint32_t r = field + 2u * lines; r < c.h; r += 2u) store_row(slot, r * w, w, 0u, runs, 0u, 0u, 0u, 0u, 0u);
  if (lane == 0u) {
    if (field) c.info[pic].lines2 = (int32_t)lines;
    else c.info[pic].lines1 = (int32_t)lines;
  }
}

}  // namespace mispu
