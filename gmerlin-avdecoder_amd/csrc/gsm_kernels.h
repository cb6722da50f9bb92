// gsm_kernels.h — the kernels of libmi_gsm.so (include/mi_gsm.h states the rules and cites upstream):
//   k_gsm_decode       one lane a stream, 64 streams a wave and a workgroup.  A frame's chain is serial in its samples and
//                      every step is a select or a clamp, so the 64 lanes walk their frames in lockstep; a lane whose
//                      stream has ended, or whose frame has a bad magic, sits the frame out.  The lane fetches its frame
//                      as the nine aligned words that hold its 33 bytes, unpacks them (gsm_format.h) into its row of
//                      parameters in LDS and runs gsm_format.h's chain: the lattice's v[9], the eight reflection
//                      coefficients and the rest of the state are registers, the history is a ring of 160 words a stream
//                      in LDS, sample-major ([sample][lane]), so that the long-term filter's gather at k - Nr, with Nr
//                      the lane's own, lands in bank (32 sample + lane / 2) mod 64: only the two lanes of one 32-bit word
//                      can meet, two ways at the worst.  Samples leave the registers as 16-byte pieces, five a subframe.
//   k_gsm_state_reset  16 bytes a lane
// Every lane has a stream of its own: its addresses are 64-bit, made of the call's base and the stream's 64-bit offset.
// LDS: 29,696 bytes a wave (the ring is 20,480 of them), which lets a CU's 160 KiB hold five waves.  Plain C++.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsm_format.h"

namespace migsm {

constexpr uint32_t kLanes = 64;
constexpr uint32_t kStateBytes = 2 * kStateWords;

struct Call {
  const uint8_t* stream;
  const uint64_t* offsets;      // n, on the device
  const uint64_t* pcm_offsets;  // n
  const uint32_t* units;        // n
  uint32_t n, fmt;
  uint8_t* pcm;
  uint8_t* state;  // n states, or nullptr
  uint32_t* bad;   // n counts, or nullptr
};

struct Lds {
  int16_t ring[kRing * kLanes];    // [sample][lane]
  uint8_t par[kLanes * kParams];   // a lane's row is 19 words: rows start in different banks
  uint32_t raw[kLanes * 9];        // the nine words around a lane's frame
  int16_t xmp[64 * 8], larpp[8 * 64];
};
static_assert(sizeof(Lds) == 29696, "five workgroups fit a CU's LDS");

__device__ __forceinline__ uint32_t pack2(int32_t lo, int32_t hi) { return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16); }

__global__ __launch_bounds__(64) void k_gsm_decode(const Call c) {
  __shared__ Lds L;
  const uint32_t lane = threadIdx.x, i = blockIdx.x * kLanes + lane;
  const Tables& T = tables();
  for (uint32_t k = lane; k < 512u; k += kLanes) L.xmp[k] = T.xmp[k], L.larpp[k] = T.larpp[k];
  __syncthreads();
  if (i >= c.n) return;

  const uint32_t frames = c.units[i] << c.fmt;
  const uint8_t* src = c.stream + c.offsets[i];
  uint8_t* dst = c.pcm + c.pcm_offsets[i];
  uint8_t* const state = c.state ? c.state + (uint64_t)i * kStateBytes : nullptr;
  int16_t* const ring = L.ring + lane;

  // the state: fresh (gsm_create: zeros, nrp 40), or the caller's
  Regs r;
  uint32_t w[12] = {0u, 0u, 0u, 0u, 0u, 40u, 0u, 0u, 0u, 0u, 0u, 0u};  // words 120 .. 143, two a word
  if (state) {
    const uint4* s = (const uint4*)state;
    for (uint32_t p = 0; p < 15u; p++) {
      const uint4 q = s[p];
      const uint32_t x[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (uint32_t e = 0; e < 4u; e++) {
        ring[(p * 8u + 2u * e) * kLanes] = (int16_t)(x[e] & 0xFFFFu);
        ring[(p * 8u + 2u * e + 1u) * kLanes] = (int16_t)(x[e] >> 16);
      }
    }
#pragma unroll
    for (uint32_t p = 0; p < 3u; p++) {
      const uint4 q = s[15u + p];
      w[4u * p] = q.x, w[4u * p + 1u] = q.y, w[4u * p + 2u] = q.z, w[4u * p + 3u] = q.w;
    }
  } else {
    for (uint32_t k = 0; k < 120u; k++) ring[k * kLanes] = 0;
  }
#pragma unroll
  for (uint32_t k = 0; k < 9u; k++) r.v[k] = (int16_t)(w[k >> 1] >> (16u * (k & 1u)));
  r.msr = (int16_t)(w[4] >> 16);
  r.nrp = (int16_t)(w[5] & 0xFFFFu);
  if (r.nrp < 40 || r.nrp > 120) r.nrp = 40;  // (no state upstream can be in; the lag indexes the ring)
#pragma unroll
  for (uint32_t k = 0; k < 8u; k++) r.prev[k] = (int16_t)(w[(11u + k) >> 1] >> (16u * ((11u + k) & 1u)));
  r.pos = 120;

  uint8_t* const par = L.par + lane * kParams;
  uint32_t* const raw = L.raw + lane * 9u;
  uint32_t bad = 0;
  for (uint32_t f = 0; f < frames; f++) {
    const bool second = c.fmt && (f & 1u);
    const uint32_t shift = (uint32_t)(uintptr_t)src & 3u;
    const uint32_t* words = (const uint32_t*)(src - shift);  // every one of the nine holds a byte of the frame
#pragma unroll
    for (uint32_t d = 0; d < 9u; d++) raw[d] = words[d];
    const uint8_t* row = (const uint8_t*)raw + shift;
    if (c.fmt || (row[0] >> 4) == 0xD) {
      unpack([&](int b) { return (uint32_t)row[b]; }, !c.fmt, (c.fmt && !second) ? 0 : 4, [&](int at, uint8_t v) { par[at] = v; });
      struct {
        const Lds* l;
        __device__ int32_t xmp(int at) const { return l->xmp[at]; }
        __device__ int32_t larpp(int at) const { return l->larpp[at]; }
      } tab = {&L};
      struct {
        int16_t* p;
        __device__ int32_t get(int s) const { return p[s * (int)kLanes]; }
        __device__ void set(int s, int32_t x) const { p[s * (int)kLanes] = (int16_t)x; }
      } hist = {ring};
      decode_frame(r, [&](int at) { return (uint32_t)par[at]; }, tab, hist, [&](int at, const int32_t* s8) {
        *(uint4*)(dst + 2 * at) = make_uint4(pack2(s8[0], s8[1]), pack2(s8[2], s8[3]), pack2(s8[4], s8[5]), pack2(s8[6], s8[7]));
      });
    } else {  // the state stays, the frame's samples are zeros
      bad++;
      for (uint32_t p = 0; p < 20u; p++) ((uint4*)dst)[p] = make_uint4(0u, 0u, 0u, 0u);
    }
    src += c.fmt ? (second ? 33 : 32) : 33;
    dst += 2 * kFrameSamples;
  }

  if (c.bad) c.bad[i] = bad;
  if (state) {
    uint4* s = (uint4*)state;
    int32_t at = r.pos - 120;  // the oldest of the 120
    if (at < 0) at += kRing;
    for (uint32_t p = 0; p < 15u; p++) {
      uint32_t x[4];
#pragma unroll
      for (uint32_t e = 0; e < 4u; e++) {
        const int32_t lo = ring[at * (int)kLanes];
        at = at + 1 == kRing ? 0 : at + 1;
        const int32_t hi = ring[at * (int)kLanes];
        at = at + 1 == kRing ? 0 : at + 1;
        x[e] = pack2(lo, hi);
      }
      s[p] = make_uint4(x[0], x[1], x[2], x[3]);
    }
    s[15] = make_uint4(pack2(r.v[0], r.v[1]), pack2(r.v[2], r.v[3]), pack2(r.v[4], r.v[5]), pack2(r.v[6], r.v[7]));
    s[16] = make_uint4(pack2(r.v[8], r.msr), pack2(r.nrp, r.prev[0]), pack2(r.prev[1], r.prev[2]), pack2(r.prev[3], r.prev[4]));
    s[17] = make_uint4(pack2(r.prev[5], r.prev[6]), pack2(r.prev[7], 0), 0u, 0u);
  }
}

// n fresh states: 18 pieces of 16 bytes a state, all zeros but nrp (word 130) = 40
__global__ __launch_bounds__(256) void k_gsm_state_reset(uint4* state, uint32_t pieces) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p < pieces) state[p] = make_uint4(0u, p % 18u == 16u ? 40u : 0u, 0u, 0u);
}

}  // namespace migsm
