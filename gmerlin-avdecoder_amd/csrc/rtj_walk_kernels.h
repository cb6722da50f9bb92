// rtj_walk_kernels.h — gfx950 walkers of the RTjpeg block chain: where every block of a packet starts.
//
//   BlockWalker    the stream as one wave sees it, 64 bytes to a window, and RTjpeg_s2b's length rule
//                  (lib/RTjpeg.c:157-186) as one step from a block's start to the next one's.
//   walk_blocks    a stretch of a packet's chain by block count (k_index_emit_walk, rtj_index_kernels.h).
//   walk_record    the same by position, marking the starts in LDS (k_spec_repair, rtj_spec_kernels.h).
//   walk_packet    a whole packet, written for the issue rates of the scalar and the vector unit, per format.
//   k_index_walk   block-start index of every packet: walk_packet driven by RTjpeg_decompressYUV420's block order
//                  (lib/RTjpeg.c:2688-2749); k_index_walk_todo: the same for the packets of a to-do list.
#pragma once
#include <hip/hip_runtime.h>

#include "rtj_common.h"

namespace mirtj {

// ---------------------------------------------------------------------------------------
// wave64 inclusive prefix sum with DPP row shifts + row broadcasts (no LDS)
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) {
  // within each row of 16 lanes: Hillis-Steele with row_shr 1,2,4,8 (out-of-row sources read 0)
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false);
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, false);
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, false);
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, false);
  // lane 15 of rows 0 and 2 into every lane of rows 1 and 3
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);
  // lane 31 into every lane of rows 2 and 3
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);
  return x;
}

// number of coefficient slots a stream byte covers when it is read as a token (lib/RTjpeg.c:171-182):
// 64..127 (int8 > 63) is a zero run of b-63, anything else is one coefficient
__device__ __forceinline__ uint32_t token_weight(uint32_t b) {
  return (b - 64u < 64u) ? b - 63u : 1u;
}

// ---------------------------------------------------------------------------------------
// BlockWalker: what one wave holds of a packet while it walks the packet's block chain.
//
// Lane i of the wave holds byte base+i of the stream (two 64-byte windows, "cur" and "nxt", and three more in
// flight) and the running sum W of token weights.  A block that starts at p with bt8 raw bytes ends at
// the first byte e whose W reaches W[p+bt8] + (63-bt8): one compare + find-first-set per block.
// The chain itself is serial (a block's length is only known once it has been read), so the
// position lives in scalar registers and the vector unit is used 64 bytes at a time.
// A block whose 63 coefficients behind DC are all raw bytes (63 - bt8 == 0) would need a step of its own; no stream
// reaches it: the host refuses tables with more than kMaxRawBytes = 15 raw coefficients, so bt8 <= 15, and the last
// non-token byte of a block that starts in the first window lies in the two windows.
// ---------------------------------------------------------------------------------------
struct BlockWalker {
  const uint8_t* g;  // the packet's first data byte
  uint32_t len;
  int lane;
  uint32_t base;                      // stream position of the first window's lane 0
  uint32_t cur, nxt, pf1, pf2, pf3;   // this lane's byte of the windows at base, base + 64, ... base + 256
  uint32_t Wc, Wn;                    // weight sums over cur and nxt, inclusive, counted from `base`

  __device__ __forceinline__ uint32_t fetch(uint32_t pos) const {
    const uint32_t i = pos + lane;
    return i < len ? (uint32_t)g[i] : 0u;
  }
  __device__ __forceinline__ BlockWalker(const FrameDev& f, const uint8_t* __restrict__ stream, uint32_t p_start)
      : g(stream + f.data_off), len(f.data_len), lane(threadIdx.x & 63), base(p_start), cur(fetch(base)),
        nxt(fetch(base + 64u)), pf1(fetch(base + 128u)), pf2(fetch(base + 192u)), pf3(fetch(base + 256u)) {
    Wc = wave_incl_scan(token_weight(cur));
    Wn = wave_incl_scan(token_weight(nxt)) + (uint32_t)__builtin_amdgcn_readlane((int)Wc, 63);
  }
  // slide the windows forward until position p (wave-uniform) lies in the first one
  __device__ __forceinline__ void slide_to(uint32_t p) {
    while (p - base >= 64u) {
      base += 64u;
      cur = nxt;
      Wc = Wn;
      nxt = pf1;
      pf1 = pf2;
      pf2 = pf3;
      pf3 = fetch(base + 256u);
      Wn = wave_incl_scan(token_weight(nxt)) + (uint32_t)__builtin_amdgcn_readlane((int)Wc, 63);
    }
  }
  // the start of the block behind the one that starts at p (in the first window) and has bt8 raw bytes
  __device__ __forceinline__ uint32_t next(uint32_t p, uint32_t bt8) const {
    const uint32_t lp = p - base;
    const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)cur, (int)lp);
    if (b0 == 0xFFu) return p + 1u;  // "unchanged" block: a single byte
    const uint32_t need = 63u - bt8;
    const uint32_t iq = lp + bt8;  // last non-token byte of the block, 0..78 (bt8 <= 15)
    const uint32_t Wq = iq < 64u ? (uint32_t)__builtin_amdgcn_readlane((int)Wc, (int)iq)
                                 : (uint32_t)__builtin_amdgcn_readlane((int)Wn, (int)(iq - 64u));
    const uint32_t target = Wq + need;
    const unsigned long long mc = __ballot(Wc >= target);
    uint32_t e;
    if (mc) {
      e = (uint32_t)__builtin_ctzll(mc);
    } else {
      const unsigned long long mn = __ballot(Wn >= target);
      e = 64u + (uint32_t)__builtin_ctzll(mn);  // W grows by >= 1 per byte, so mn != 0
    }
    return base + e + 1u;
  }
};

// walk_blocks: one wave walks blocks k0..k1-1 (k0 a multiple of 6) of one packet starting at byte p_start and writes
// out[k] = byte offset of block k relative to the first data byte; with write_end also out[k1] = end position.
__device__ __forceinline__ void walk_blocks(const FrameDev& f, const uint8_t* __restrict__ stream,
                                            const QTab* __restrict__ lut, uint32_t p_start, uint32_t k0,
                                            uint32_t k1, bool write_end, uint32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const uint32_t lb8 = (uint32_t)lut[f.qidx].lb8, cb8 = (uint32_t)lut[f.qidx].cb8;
  BlockWalker w(f, stream, p_start);
  uint32_t p = p_start;  // current block start (uniform)
  uint32_t ph = 0;       // block number within the macroblock, 0..5
  uint32_t acc = 0;      // up to 64 offsets gathered one lane at a time, stored 256 B at once

  for (uint32_t k = k0;; ++k) {
    w.slide_to(p);
    const bool last = k == k1;
    if (!last || write_end) acc = (uint32_t)lane == (k & 63u) ? p : acc;
    if ((k & 63u) == 63u || last) {
      const uint32_t idx = (k & ~63u) + (uint32_t)lane;
      const uint32_t top = last && !write_end ? k - 1u : k;  // k1 > k0 >= 0, so no wrap
      if (idx >= k0 && idx <= top) out[idx] = acc;
    }
    if (last) break;
    const uint32_t bt8 = ph >= 4u ? cb8 : lb8;
    ph = ph == 5u ? 0u : ph + 1u;
    p = w.next(p, bt8);
  }
}

// The same walk, bounded by position instead of block count, for the speculative index's repairs
// (rtj_spec_kernels.h): from byte p_start, taken to start a macroblock, every block start below `limit` sets its bit in
// `bits` (LDS, zeroed by the caller; bit 31 - i of dword k = position 32 k + i relative to p_start, the first start
// is position 0; starts at or past `span` relative positions are counted but not marked).  Returns the number of blocks.
// take / tail: (index << 16 | offset) of the last unit-aligned start below `mid` / below `limit`, the unit being
// the macroblock, or the block when lb8 == cb8.
__device__ __forceinline__ uint32_t walk_record(const FrameDev& f, const uint8_t* __restrict__ stream,
                                                const QTab* __restrict__ lut, uint32_t p_start, uint32_t mid,
                                                uint32_t limit, uint32_t* bits, uint32_t span, uint32_t& take,
                                                uint32_t& tail) {
  const int lane = threadIdx.x & 63;
  const uint32_t lb8 = (uint32_t)lut[f.qidx].lb8, cb8 = (uint32_t)lut[f.qidx].cb8;
  BlockWalker w(f, stream, p_start);
  uint32_t p = p_start, ph = 0, k = 0;
  const bool by_block = lb8 == cb8;
  take = tail = 0;
  while (p < limit) {
    if (by_block || ph == 0u) {  // a unit-aligned record
      const uint32_t v = (k << 16) | (p - p_start);
      if (p < mid) take = v;
      tail = v;
    }
    w.slide_to(p);
    {
      const uint32_t rel = p - p_start;  // wave-uniform: one lane marks it
      if (lane == 0 && rel < span) bits[rel >> 5] |= 0x80000000u >> (rel & 31u);
    }
    k++;
    const uint32_t bt8 = ph >= 4u ? cb8 : lb8;
    ph = ph == 5u ? 0u : ph + 1u;
    p = w.next(p, bt8);
  }
  return k;
}

// walk_packet: walk_blocks for a whole packet, written for the issue rates of the scalar and the vector unit.  With
// thousands of walkers resident the serial walk is bound by instruction issue (a SIMD issues one scalar and one vector
// instruction per four cycles; walk_blocks' early-outs compile to ~46 scalar instructions per block, half of them
// branches and flag shuffling).  Here:
//   * a block is ONE straight path: the next position is selected between its two cases (unchanged block: 1 byte; else
//     behind the byte whose weight sum reaches the target — tables whose blocks are all raw bytes are refused by the host,
//     kMaxRawBytes) with scalar selects, and both windows are searched at once;
//   * the macroblock's blocks are unrolled from FmtShape<Fmt> (kBlkPerMb - kChromaPlanes luma steps, then kChromaPlanes
//     chroma steps: Y Y Y Y Cb Cr, Y Y Cb Cr, or Y alone), so the raw-byte count of a block is a loop constant;
//   * of the window's bytes only "is 0xFF" is kept, as a lane mask in scalar registers (one compare per 64 bytes instead of
//     a lane read per block), so nothing but the weight sums and the bytes in flight rotates when the window slides;
//   * the stream is read through a buffer descriptor that returns 0 past the packet's end (no exec masking);
//   * the offsets are gathered with v_writelane at a running lane and stored 64 at a time.
// Bounds no stream reaches, for all three block patterns: the search of a block is entered with lp < 64, and a block is
// at most 64 bytes (the host refuses tables with more than kMaxRawBytes raw coefficients, so a block always ends behind
// a byte of the two windows), so the next lp is at most 127 and the slide loop runs at most once per block; the
// macroblock loop runs f.nmb times.
template <int Fmt>
__device__ __forceinline__ void walk_packet(const FrameDev& f, const uint8_t* __restrict__ stream,
                                            const QTab* __restrict__ lut, uint32_t* __restrict__ out) {
  constexpr uint32_t kB = FmtShape<Fmt>::kBlkPerMb, kLuma = kB - FmtShape<Fmt>::kChromaPlanes;
  static_assert((kLuma == 1u || kLuma == 2u || kLuma == 4u) && (kB == kLuma || kB == kLuma + 2u), "the step list below");
  const uint32_t lane = threadIdx.x & 63u;
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)(stream + f.data_off), 0, (int)f.data_len, 0x00020000);
  // a stream byte as int8 (the range check of a raw buffer covers the vector offset only: the position goes there)
  auto fetch = [&](uint32_t pos) -> int {
    return (int)(int8_t)__builtin_amdgcn_raw_buffer_load_b8(rs, (int)(pos + lane), 0, 0);
  };
  // token_weight() of an int8: 64..127 is a zero run of b - 63, anything else (<= 63, negative) one coefficient
  auto weight = [](int b) -> uint32_t {
    const int x = b - 63;
    return (uint32_t)(x < 1 ? 1 : x > 64 ? 64 : x);
  };
  const uint32_t lb8 = (uint32_t)lut[f.qidx].lb8, cb8 = (uint32_t)lut[f.qidx].cb8;
  const uint32_t need_l = 63u - lb8, need_c = 63u - cb8;
  uint32_t base = 0, Wc, Wn;
  int pf1, pf2, pf3;
  unsigned long long ffc, ffn;  // lanes of the two windows that hold 0xFF ("unchanged block" where a block starts)
  {
    const int cur = fetch(0u), nxt = fetch(64u);
    pf1 = fetch(128u);
    pf2 = fetch(192u);
    pf3 = fetch(256u);
    Wc = wave_incl_scan(weight(cur));
    Wn = wave_incl_scan(weight(nxt)) + (uint32_t)__builtin_amdgcn_readlane((int)Wc, 63);
    ffc = __ballot(cur == -1);
    ffn = __ballot(nxt == -1);
  }
  uint32_t lp = 0;     // the current block's start, relative to base
  uint32_t j = 0;      // offsets gathered in acc since the last store
  uint32_t acc = 0;
  uint32_t* o = out;   // where acc's lane 0 goes
  auto flush = [&]() {
    if (lane < j) o[lane] = acc;
    o += j;
    j = 0;
  };
  auto step = [&](const uint32_t bt8, const uint32_t need, const int c) {  // c: the block's number in its macroblock
    while (lp >= 64u) {  // slide the two windows forward
      base += 64u;
      lp -= 64u;
      const int b = pf1;
      pf1 = pf2;
      pf2 = pf3;
      pf3 = fetch(base + 256u);
      Wc = Wn;
      ffc = ffn;
      Wn = wave_incl_scan(weight(b)) + (uint32_t)__builtin_amdgcn_readlane((int)Wc, 63);
      ffn = __ballot(b == -1);
    }
    asm("s_add_i32 m0, %2, %3\n\tv_writelane_b32 %0, %1, m0" : "+v"(acc) : "s"(base + lp), "s"(j), "n"(c) : "m0", "scc");
    const uint32_t iq = lp + bt8;  // last non-token byte of the block, 0..78
    const uint32_t wq_c = (uint32_t)__builtin_amdgcn_readlane((int)Wc, (int)(iq & 63u));
    const uint32_t wq_n = (uint32_t)__builtin_amdgcn_readlane((int)Wn, (int)(iq & 63u));
    const uint32_t target = (iq < 64u ? wq_c : wq_n) + need;
    // first byte whose sum reaches the target: in the first window, else in the second (W grows by >= 1 per byte, so
    // it is there); find-first-set of nothing is 0xFFFFFFFF
    const unsigned long long mc = __ballot(Wc >= target), mn = __ballot(Wn >= target);
    uint32_t ec, en;
    asm("s_ff1_i32_b64 %0, %1" : "=s"(ec) : "s"(mc));
    asm("s_ff1_i32_b64 %0, %1" : "=s"(en) : "s"(mn));
    en |= 64u;
    const uint32_t e = ec < en ? ec : en;
    asm("s_bitcmp1_b64 %1, %2\n\ts_cselect_b32 %0, %3, %4" : "=s"(lp) : "s"(ffc), "s"(lp), "s"(lp + 1u), "s"(e + 1u) : "scc");
  };
  for (uint32_t mb = 0; mb < f.nmb; ++mb) {
    if (j > 64u - kB) flush();
    // kLuma (4, 2 or 1) luma steps, then the chroma pair.  Written out: as a loop over the block number, unrolled by
    // the compiler, every step of the 4:2:0 walker compiles to one more scalar instruction.
    step(lb8, need_l, 0);
    if constexpr (kLuma > 1u) step(lb8, need_l, 1);
    if constexpr (kLuma > 2u) {
      step(lb8, need_l, 2);
      step(lb8, need_l, 3);
    }
    if constexpr (kB > kLuma) {
      step(cb8, need_c, (int)kLuma);
      step(cb8, need_c, (int)kLuma + 1);
    }
    j += kB;
  }
  if (j > 63u) flush();
  asm("s_mov_b32 m0, %2\n\tv_writelane_b32 %0, %1, m0" : "+v"(acc) : "s"(base + lp), "s"(j) : "m0");  // the end
  j += 1u;
  flush();
}

// Whole packet by one wave: the simple (serial) index, kept as the A/B baseline of the parallel one.
__global__ __launch_bounds__(64) void k_index_walk(const FrameDev* __restrict__ frames,
                                                    const uint8_t* __restrict__ stream,
                                                    const QTab* __restrict__ lut,
                                                    uint32_t* __restrict__ blkoff) {
  const FrameDev f = frames[blockIdx.x];
  walk_packet<kFmtYUV420>(f, stream, lut, blkoff + f.blk_base);
}

// The packets of a to-do list, a wave each (grid-stride): what k_spec_policy hands the serial walker when the list is long.
__global__ __launch_bounds__(64) void k_index_walk_todo(const FrameDev* __restrict__ frames,
                                                         const uint8_t* __restrict__ stream,
                                                         const QTab* __restrict__ lut, uint32_t* __restrict__ blkoff,
                                                         const uint32_t* __restrict__ todo,
                                                         const uint32_t* __restrict__ ntodo) {
  const uint32_t n = *ntodo;
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
    const FrameDev f = frames[todo[i]];
    walk_packet<kFmtYUV420>(f, stream, lut, blkoff + f.blk_base);
  }
}

}  // namespace mirtj
