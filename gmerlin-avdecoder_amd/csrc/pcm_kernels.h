// pcm_kernels.h — the kernels of libmi_pcm.so (include/mi_pcm.h states the rules and cites upstream):
//   k_pcm_decode<C>  one workgroup a (packet, tile): a tile is kTileBytes of a packet's output, from a multiple of 16
//   k_pcm_zero       the counts of a call that asks for them, before k_pcm_decode adds to them
// The transforms are pcm_format.h's, which the host runs too.  DESIGN.md section 17 has the shapes and the figures.
//
// A PIECE is 16 bytes of the output and piece_in (16, 12, 10 or 8) bytes of the packet, a whole number of the codec's
// groups: every tile starts on a group boundary.  A lane makes a piece out of registers: the one or two aligned 16-byte
// words that hold the piece's packet bytes (the second only where the bytes reach into it, so no word without a byte of
// the packet is read), shifted by whole words with selects and by bytes with v_alignbyte, then one aligned 16-byte store.
// A wave's loads and stores are consecutive.  The last piece of a packet (the output ends inside it, or upstream's loops
// stop short of its bytes: the LPCM tails) reads the bytes it may read one by one and writes its own bytes only.
//
// Addressing: a 64-bit base plus the packet's 64-bit offset; inside a packet byte positions are below 2^32 (a packet is
// below 2^31 bytes and no codec more than doubles it) and are widened before they are added.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pcm_format.h"

namespace mipcm {

constexpr uint32_t kThreads = 256, kLanePieces = 4;
constexpr uint32_t kTilePieces = kThreads * kLanePieces, kTileBytes = 16u * kTilePieces;

// What a call brings: per packet, where it lies and where its samples go, the bytes upstream's loops read (valid_in), the
// bytes of its samples (out_bytes) and the call's tiles before its first (tile_first, ascending: a packet without samples
// has none).
struct Call {
  const uint8_t* packets;
  uint8_t* samples;
  const uint64_t* offsets;
  const uint64_t* sample_offsets;
  const uint32_t* valid_in;
  const uint32_t* out_bytes;
  const uint32_t* tile_first;
  uint32_t* outside;  // or NULL
  uint32_t n;
};

__device__ __forceinline__ uint32_t pick(uint32_t ws, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  return ws == 0 ? a : ws == 1 ? b : ws == 2 ? c : d;
}

// the kIn bytes at p, which lie inside the packet, as words in v (bytes behind the kIn are whatever the words held)
template <uint32_t kIn>
__device__ __forceinline__ void load_piece(const uint8_t* __restrict__ p, uint32_t v[4]) {
  const uint32_t m = (uint32_t)(uintptr_t)p & 15u;
  const uint4* __restrict__ w = (const uint4*)(p - m);
  const uint4 lo = w[0];
  uint4 hi = make_uint4(0, 0, 0, 0);
  if (m + kIn > 16u) hi = w[1];  // the piece reaches into the next word: that word holds a byte of the packet
  const uint32_t W[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  constexpr int kWords = (kIn + 3) / 4;
  const uint32_t ws = m >> 2, bs = m & 3u;
  uint32_t x[kWords + 1];
#pragma unroll
  for (int i = 0; i <= kWords; i++) x[i] = pick(ws, W[i], W[i + 1], W[i + 2], W[i + 3]);
#pragma unroll
  for (int i = 0; i < 4; i++) v[i] = i < kWords ? __builtin_amdgcn_alignbyte(x[i + 1], x[i], bs) : 0u;
}

template <int C>
__global__ __launch_bounds__(256) void k_pcm_decode(const Call c) {
  constexpr uint32_t kIn = kGroups[C].piece_in;
  // the packet of this tile: the last one whose first tile is not behind it (uniform over the workgroup)
  const uint32_t b = blockIdx.x;
  uint32_t pkt = 0, end = c.n;
  while (end - pkt > 1u) {
    const uint32_t mid = pkt + (end - pkt) / 2u;
    if (c.tile_first[mid] <= b) pkt = mid;
    else end = mid;
  }
  const uint32_t tile = b - c.tile_first[pkt];
  const uint8_t* __restrict__ in = c.packets + c.offsets[pkt];
  uint8_t* __restrict__ out = c.samples + c.sample_offsets[pkt];
  const uint64_t valid = c.valid_in[pkt], bytes = c.out_bytes[pkt];
  uint32_t outside = 0;
#pragma unroll
  for (uint32_t k = 0; k < kLanePieces; k++) {
    const uint64_t q = (uint64_t)tile * kTilePieces + k * kThreads + threadIdx.x, at = 16u * q, from = kIn * q;
    if (at >= bytes) continue;
    uint32_t o[4];
    if (at + 16u <= bytes && from + kIn <= valid) {
      uint32_t v[4];
      load_piece<kIn>(in + from, v);
      outside += piece<C>([&](int i) { return (v[i >> 2] >> (8 * (i & 3))) & 0xffu; }, o);
      *(uint4*)(out + at) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
      uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
      for (uint32_t i = 0; i < kIn; i++)
        if (from + i < valid) v[i >> 2] |= (uint32_t)in[from + i] << (8u * (i & 3u));
      outside += piece<C>([&](int i) { return (v[i >> 2] >> (8 * (i & 3))) & 0xffu; }, o);
      if (at + 16u <= bytes) {
        *(uint4*)(out + at) = make_uint4(o[0], o[1], o[2], o[3]);
      } else {
        const uint32_t left = (uint32_t)(bytes - at);
#pragma unroll
        for (uint32_t i = 0; i < 16u; i++)
          if (i < left) out[at + i] = (uint8_t)(o[i >> 2] >> (8u * (i & 3u)));
      }
    }
  }
  if constexpr (is_float(C)) {
    // an integer sum: exact in any order.  One atomic a wave, and only where the wave counted something.
    if (c.outside) {
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) outside += __shfl_xor(outside, s);
      if ((threadIdx.x & 63u) == 0 && outside) atomicAdd(c.outside + pkt, outside);
    }
  }
}

__global__ __launch_bounds__(256) void k_pcm_zero(uint32_t* __restrict__ counts, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n) counts[i] = 0u;
}

}  // namespace mipcm
