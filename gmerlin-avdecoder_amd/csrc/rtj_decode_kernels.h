// rtj_decode_kernels.h — gfx950 kernels of the RTjpeg decode path: the transform.
//
//   k_decode       dequantise + 8x8 AAN inverse transform + plane scatter
//                  (lib/RTjpeg.c:157-186, 2209-2332, 2688-2749), one lane per 8x8 block.
//   transform_lo, transform_full   the transform of a live block, shared with k_decode_fmt (rtj_format_kernels.h).
//
// The block-start index the transform reads (k_index_walk and the walkers) is in rtj_walk_kernels.h.
//
// Integer only; no MFMA: the transform is a fixed 8-point butterfly network with rounding
// after every product, not a contraction.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "rtj_common.h"
#include "rtj_idct_asm.h"
#include "rtj_idct_pk.h"

namespace mirtj {

__constant__ uint8_t c_zz[64] = MIRTJ_ZZ_INIT;

// ---------------------------------------------------------------------------------------
// 8-point inverse AAN butterfly (lib/RTjpeg.c:2240-2283 for columns, :2290-2327 for rows;
// constants :1196-1199, MULTIPLY :1206).  Every multiplicand stays below 2^23 in magnitude
// for any int16 input block (tests/test_bounds.py), so the 24-bit multiplier is exact and
// wraps like the reference's 32-bit product.
// ---------------------------------------------------------------------------------------
// v_mad_i32_i24 is spelled out: hipcc's value tracking cannot see the 2^23 bound and would
// otherwise fall back to the quarter-rate 32-bit multiplier for the whole row pass.
__device__ __forceinline__ int mulr8(int x, int c) {
  int r;
  asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(x), "s"(c), "v"(128));
  return r >> 8;
}

__device__ __forceinline__ int mul24(int a, int b) {  // both operands inside the signed 24-bit range
  int r;
  asm("v_mul_i32_i24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// The readable statement of the butterfly.  No kernel calls it (the passes of rtj_idct_asm.h and rtj_idct_pk.h compute
// the same in their own instruction order); tools/ubench/idct_rate.hip and idct_asm_rate.hip keep it as the comparator.
__device__ __forceinline__ void idct8(int x0, int x1, int x2, int x3, int x4, int x5, int x6, int x7,
                                      int (&y)[8]) {
  const int s04 = x0 + x4, d04 = x0 - x4;
  const int s26 = x2 + x6;
  const int r26 = mulr8(x2 - x6, 362) - s26;
  const int e0 = s04 + s26, e3 = s04 - s26, e1 = d04 + r26, e2 = d04 - r26;
  const int s53 = x5 + x3, d53 = x5 - x3, s17 = x1 + x7, d17 = x1 - x7;
  const int o7 = s17 + s53;
  const int m = mulr8(s17 - s53, 362);
  const int z5 = mulr8(d53 + d17, 473);
  const int o6 = mulr8(d53, -669) + z5 - o7;
  const int o5 = m - o6;
  const int o4 = mulr8(d17, 277) - z5 + o5;
  y[0] = e0 + o7; y[7] = e0 - o7;
  y[1] = e1 + o6; y[6] = e1 - o6;
  y[2] = e2 + o5; y[5] = e2 - o5;
  y[4] = e3 + o4; y[3] = e3 - o4;
}

// The same transform when x4..x7 are zero (every term they feed vanishes exactly: M(0,c) == 0 and
// (-x)*(-669) == x*669), used when a whole wave's blocks keep their coefficients in the low 4x4.
__device__ __forceinline__ void idct8_lo(int x0, int x1, int x2, int x3, int (&y)[8]) {
  const int r26 = mulr8(x2, 362) - x2;
  const int e0 = x0 + x2, e3 = x0 - x2, e1 = x0 + r26, e2 = x0 - r26;
  const int o7 = x1 + x3, d13 = x1 - x3;
  const int m = mulr8(d13, 362);
  const int z5 = mulr8(d13, 473);
  const int o6 = mulr8(x3, 669) + z5 - o7;
  const int o5 = m - o6;
  const int o4 = mulr8(x1, 277) - z5 + o5;
  y[0] = e0 + o7; y[7] = e0 - o7;
  y[1] = e1 + o6; y[6] = e1 - o6;
  y[2] = e2 + o5; y[5] = e2 - o5;
  y[4] = e3 + o4; y[3] = e3 - o4;
}

// DESCALE + int16 narrowing + clamp 16..235 (lib/RTjpeg.c:1201-1205).  The +4 rounding term
// was folded into the DC coefficient before the column pass, so only the shift remains:
// bits [18:3] sign-extended == (int16_t)(v >> 3).
__device__ __forceinline__ uint32_t px(int v) {
  int s = (int)((uint32_t)v << 13) >> 16;
  s = s > 235 ? 235 : s;
  s = s < 16 ? 16 : s;
  return (uint32_t)s;
}

__device__ __forceinline__ uint32_t lshl_or(uint32_t a, int sh, uint32_t b) {  // (a << sh) | b
  uint32_t r;
  asm("v_lshl_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "n"(sh), "v"(b));
  return r;
}

// LDS accesses by 32-bit byte address (the parse loop keeps addresses, not indices, in registers)
typedef __attribute__((address_space(3))) uint32_t lds_u32_t;
typedef __attribute__((address_space(3))) int16_t lds_i16_t;
__device__ __forceinline__ uint32_t lds_address(const void* p) {
  return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void*)p;
}

// (signed or unsigned byte b of w) * (bits 31:16 of e): byte select, sign extension and the 16-bit
// field select ride on the multiply (SDWA), so a coefficient costs one vector instruction
__device__ __forceinline__ int mul_byte_hi16(uint32_t w, uint32_t e, int b, bool sign) {
  int r;
#define MIRTJ_MUL_SDWA(SRC0, SEL) \
  asm("v_mul_i32_i24_sdwa %0, " SRC0 ", %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:" SEL " src1_sel:WORD_1" \
      : "=v"(r) : "v"(w), "v"(e))
  if (sign) {
    switch (b) {
      case 0: MIRTJ_MUL_SDWA("sext(%1)", "BYTE_0"); break;
      case 1: MIRTJ_MUL_SDWA("sext(%1)", "BYTE_1"); break;
      case 2: MIRTJ_MUL_SDWA("sext(%1)", "BYTE_2"); break;
      default: MIRTJ_MUL_SDWA("sext(%1)", "BYTE_3"); break;
    }
  } else {
    switch (b) {
      case 0: MIRTJ_MUL_SDWA("%1", "BYTE_0"); break;
      case 1: MIRTJ_MUL_SDWA("%1", "BYTE_1"); break;
      case 2: MIRTJ_MUL_SDWA("%1", "BYTE_2"); break;
      default: MIRTJ_MUL_SDWA("%1", "BYTE_3"); break;
    }
  }
#undef MIRTJ_MUL_SDWA
  return r;
}

// (signed byte b of w) - k: extraction, sign extension and the bias in one instruction
__device__ __forceinline__ int sbyte_minus(uint32_t w, int b, int k) {
  int r;
#define MIRTJ_SUB_SDWA(SEL) \
  asm("v_sub_u32_sdwa %0, sext(%1), %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:" SEL " src1_sel:DWORD" \
      : "=v"(r) : "v"(w), "v"(k))
  switch (b) {
    case 0: MIRTJ_SUB_SDWA("BYTE_0"); break;
    case 1: MIRTJ_SUB_SDWA("BYTE_1"); break;
    case 2: MIRTJ_SUB_SDWA("BYTE_2"); break;
    default: MIRTJ_SUB_SDWA("BYTE_3"); break;
  }
#undef MIRTJ_SUB_SDWA
  return r;
}

__device__ __forceinline__ int med3_i32(int a, int b, int c) {
  int r;
  asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
  return r;
}

// A lane's coefficient scratch: dword 8 j + r = coefficient (row r, column 2j) | coefficient (row r, column 2j + 1) << 16,
// so that the 16-byte pieces 2j and 2j + 1 are rows 0-3 and 4-7 of the column pair j, two columns to a register as
// the packed column pass takes them (rtj_idct_pk.h).  Byte offset of natural index `nat` = 8 row + column:
__host__ __device__ constexpr int coef_byte(int nat) {
  return 4 * (((nat & 7) >> 1) * 8 + (nat >> 3)) + 2 * (nat & 1);
}
// ... and of zig-zag slot k
__host__ __device__ constexpr int slot_byte(int k) {
  constexpr uint8_t z[64] = MIRTJ_ZZ_INIT;
  return coef_byte(z[k]);
}

constexpr int kDecThreads = 64;
#ifndef MIRTJ_COEF_STRIDE
#define MIRTJ_COEF_STRIDE 72
#endif
#ifndef MIRTJ_DEC_WAVES
#define MIRTJ_DEC_WAVES 1
#endif
#ifndef MIRTJ_DEC_ITERS
#define MIRTJ_DEC_ITERS 11
#endif
constexpr int kCoefStride = MIRTJ_COEF_STRIDE;  // int16 per lane: 64 + 8 pad (144 B, conflict-free b128 reads)
constexpr int kDecIters = MIRTJ_DEC_ITERS;      // macroblock groups a wave works through, one after the other (at most)
constexpr int kSlotTabN = 64 + 16;              // slot table: 64 coefficient slots, then "block finished" entries
constexpr int kMaxRawBytes = 15;                // the host refuses tables with more leading 8-bit coefficients
#ifdef MIRTJ_TEST_GENERIC_PATHS  // test build: always take the paths real tables and whole packets rarely reach
constexpr bool kForceGenericPaths = true;
#else
constexpr bool kForceGenericPaths = false;
#endif
// waves per part (span 1) or per frame (span 3: a wave takes all three parts of its groups) of a picture with `groups`
// macroblock groups: enough for kDecIters groups per wave and, for small batches, enough that `frames` pictures
// still make kDecMinWaves waves (one packet: a wave per group and part; a wave then works through fewer groups than
// kDecIters).  With a wave per part, which XCD the three parts of a group run on matters more than their number.  With part-major block numbering, measured at 1080p x 4096 (tools/ab_slots.sh,
// profiles/r01/v19_waves_per_part_ab.txt): 25..45 odd 5.17-5.30 ms, 24 / 40 / 48 / 56 5.42-5.72, 32 and 64
// 5.73-5.98 — with a multiple of 8 the three parts of a group share an XCD (workgroups are dealt round-robin to
// the 8 XCDs) and their stream bytes and block offsets come from HBM once, and that is the SLOW arrangement;
// spreading the parts over XCDs reads them three times (HBM traffic 1.17x -> 1.5x the algorithmic bytes) and is
// 5 % faster all the same.  k_decode therefore numbers its blocks slot-major (5.23-5.25 ms whatever the count,
// v19_block_numbering_ab.txt); the count is kept odd for good measure.  With a wave per frame slot (span 3) nothing
// is read twice, and 32 / 64 / 128 waves per frame are still 9 % slower than 24, 25, 43 or 51
// (profiles/r02/ab_waves_per_frame_rotate.txt; cause not established): the count stays odd.
constexpr uint32_t kDecMinWaves = 65536;
__host__ __device__ constexpr uint32_t decode_slots(uint32_t groups, uint32_t frames, uint32_t span = 1u) {
  const uint32_t by_iters = (groups + (uint32_t)kDecIters - 1u) / (uint32_t)kDecIters;
  const uint32_t per_slot = (span == 3u ? 1u : 3u) * (frames ? frames : 1u);  // waves a slot makes
  uint32_t by_batch = (kDecMinWaves + per_slot - 1u) / per_slot;
  if (by_batch > groups) by_batch = groups;
  return (by_iters > by_batch ? by_iters : by_batch) | 1u;
}
constexpr uint32_t kDecRotateMinGroups = 32768;  // groups in a batch from which a wave takes all three parts (span 3): 129 pictures of 1080p
constexpr uint32_t kFetchSpan = 72;             // a block's loads stay below its start + this (64 + alignment + look-ahead)

// ---------------------------------------------------------------------------------------
// k_decode: one wave per workgroup; slots = decode_slots().  A group is kMbPerGroup consecutive macroblocks and
// has three PARTS of 64 blocks:
//   part 0: the 64 upper luma blocks (Y0,Y1 of each MB), part 1: the 64 lower ones,
//   part 2: 32 Cb + 32 Cr blocks.
// span 3 (batches): grid (slots, frames); a wave takes the three parts of each of its up to kDecIters groups
// (slot, slot + slots, ...) in turn.  span 1 (small batches, one packet): grid (3 * slots, frames); a wave owns one
// part of its groups.
// Lanes of a wave hold horizontally adjacent blocks, so every row store of a wave covers 512
// (luma) or 2x256 (chroma) contiguous bytes.  Each lane pulls its own block's bytes from the
// stream (neighbouring lanes read neighbouring bytes, so the wave's loads stay within a few
// cache lines), parses them into a private LDS scratch (by column pairs, coef_byte() below: two 16-byte
// reads are a column pair, one row to a dword), then runs both transform passes entirely in registers —
// two values to a register where the block's values allow it (rtj_idct_pk.h).
//
// The kernel is bound by vector-instruction issue, so the parse loop is built to cost few
// instructions per stream byte:
//   * the slot table holds (dequantiser << 16 | scratch byte offset); byte select, sign extension
//     and field select ride on the multiply and the address add (SDWA);
//   * the slot counter is kept as the table's LDS address; "one slot, or the run length, and stop
//     at 64" is one add, one shift-add and one median; entries past slot 63 point at a write-only
//     dump with multiplier 0, so finished lanes need no predicate;
//   * a zero run writes a 0 at its first slot instead of being predicated off (the scratch is
//     zero already, and no slot is visited twice);
//   * DC and the bt8 raw bytes sit at fixed slots: one multiply and one store at a constant
//     offset each, per wave-uniform bt8 (0, 4, 8, 9 are the values the tables take);
//   * the "past the packet's end reads as zero" masking is skipped when the whole wave's loads lie
//     inside the packet (all but the last few blocks of a packet).
// When no block of a wave has a coefficient outside the low 4x4 (chroma at high quality, flat
// content), both passes run the four-input transform: four columns instead of eight.
//
// A wave works through several groups so that it can request the next group's block offset before
// parsing and the next group's stream bytes before transforming: only the first group pays the
// three dependent loads (descriptor -> block offset -> stream bytes).  Eleven groups per wave measured
// 5 % faster than three at 1080p (A/B over 3..32, tools/ab_iters.sh); the number of waves per part
// ("slots", decode_slots()) matters as well.
// ---------------------------------------------------------------------------------------
constexpr int kCoefWords = kDecThreads * kCoefStride / 2;
#ifndef MIRTJ_DEC_LDS_PAD
#define MIRTJ_DEC_LDS_PAD 0
#endif
constexpr int kDecLdsWords = kCoefWords + 2 * kSlotTabN + MIRTJ_DEC_LDS_PAD;  // scratch, luma slot table, chroma slot table



// ---------------------------------------------------------------------------------------
// What k_decode leaves to k_decode_list: (frame row of the launch, group | part << 28).  A wave of the batch
// instantiation that meets a block outside the packed passes' 16-bit budget (rtj_idct_pk.h: no legal picture has one),
// and a pooling chroma wave that meets a group its short forms do not cover, append the WHOLE part of the group here
// and store nothing of it; k_decode_list then decodes those parts with the one-value-per-register passes — whole
// parts, so whole row segments (partial-line writes are what made round 2's deferred blocks slow).  The capacity is
// every part of every group of the launch: the list cannot overflow.
// ---------------------------------------------------------------------------------------
// LDS traffic of ONE wave is ordered by the hardware (a wave's LDS instructions execute in order); what the lanes of a
// wave need between a write and another lane's read is that the compiler keeps the order: fences at wavefront scope.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct DecList {
  uint32_t* count;
  uint2* items;
  uint32_t cap;
};
// The plan's decode policy, on the device (two words: mode, launches left in it): batches start with k_decode_split; a
// launch that leaves more than 1 / kDecListShare of its group parts to the list — content whose chroma the pooling waves
// do not cover: noisy pictures — makes the next kDecClassicLaunches launches run k_decode<true, false> instead, then the
// split form is tried again.  k_decode_list, the last kernel of a launch, keeps the books.
enum : uint32_t { kDecModeSplit = 0u, kDecModeClassic = 1u };
constexpr uint32_t kDecListShare = 48u;       // of all group parts of the launch (three per group)
constexpr uint32_t kDecClassicLaunches = 64u;
__device__ __forceinline__ void declist_push(const DecList& L, uint32_t fidx, uint32_t grp, uint32_t part) {
  // called by the lanes of a (possibly divergent) branch with wave-uniform arguments: the first active lane appends
  const unsigned long long m = __ballot(1);
  if (((uint32_t)threadIdx.x & 63u) == (uint32_t)__builtin_ctzll(m)) {
    const uint32_t i = atomicAdd(L.count, 1u);
    if (i < L.cap) L.items[i] = make_uint2(fidx, grp | (part << 28));
  }
}

// a wave-uniform pointer, told to the compiler: the hand-issued loads take their bases from scalar registers, and a
// value loaded from memory the kernel also writes (the list's entries, a descriptor behind an atomic) is not known to
// be uniform otherwise
template <class T>
__device__ __forceinline__ T* uniform_ptr(T* p) {
  const uint64_t v = (uint64_t)(uintptr_t)p;
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return (T*)(uintptr_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ int half16(uint32_t w, int odd) { return odd ? (int)w >> 16 : (int)(int16_t)(w & 0xFFFFu); }

// The transform's forms for blocks with nothing outside the low 4x4 (three-input, packed or not; four-input): `my` is
// the lane's coefficient scratch, the eight rows are handed to `putp` (clamped and packed, row 0 first).  Called by the
// lanes that have a live block; which form runs is decided per wave (ballots over those lanes).
template <class Put>
__device__ __forceinline__ void transform_lo(const uint4* my, const IdctK& K, const IdctPK& KP, Put&& putp) {
  auto putr = [&](const int (&y)[8]) {
    uint2 o;
    // three shift-or instructions per four pixels, spelled out: the compiler's own choice for
    // a | b<<8 | c<<16 | d<<24 is two shifts, an or3 and a shift-or
    o.x = lshl_or(lshl_or(px(y[3]), 8, px(y[2])), 16, lshl_or(px(y[1]), 8, px(y[0])));
    o.y = lshl_or(lshl_or(px(y[7]), 8, px(y[6])), 16, lshl_or(px(y[5]), 8, px(y[4])));
    putp(o);
  };
  // rows 0-3 of the column pairs (0, 1) and (2, 3)
  const uint4 qa = my[0], qb = my[2];
  // anything in row 3 or column 3?
  const uint32_t t3 = qa.w | qb.w | ((qb.x | qb.y | qb.z) & 0xFFFF0000u);
  if (!__any(t3 != 0u)) {
    // ---- three-input transform: columns 0-2 in, rows of three in ----
    const bool fits = __all(pk_range_lo3(qa, qb, KP));
    if (fits) {
      // two columns, then two rows, to a register (rtj_idct_pk.h)
      uint32_t ya[8], yb[8];
      idct8_pk_lo3_col<true>(qa.x, qa.y, qa.z, ya, KP);   // columns 0, 1
      idct8_pk_lo3_col<false>(qb.x, qb.y, qb.z, yb, KP);  // columns 2, (3: zero)
#pragma unroll
      for (int r = 0; r < 8; r += 2) {
        uint2 o0, o1;
        idct8_pk_lo3_row_px(ya[r], ya[r + 1], yb[r], yb[r + 1], o0, o1, KP);
        putp(o0);
        putp(o1);
      }
    } else {
      int ws[8][3];
      {
        int y[8];
        idct8_lo3_col<true, false>(qa.x, qa.y, qa.z, y, K);
#pragma unroll
        for (int r = 0; r < 8; r++) ws[r][0] = y[r];
        idct8_lo3_col<false, true>(qa.x, qa.y, qa.z, y, K);
#pragma unroll
        for (int r = 0; r < 8; r++) ws[r][1] = y[r];
        idct8_lo3_col<false, false>(qb.x, qb.y, qb.z, y, K);
#pragma unroll
        for (int r = 0; r < 8; r++) ws[r][2] = y[r];
      }
#pragma unroll
      for (int r = 0; r < 8; r++) putp(idct8_lo3_row_px(ws[r][0], ws[r][1], ws[r][2], K));
    }
  } else {
    // ---- four-input transform: columns 0-3 in, rows of four in ----
    int ws[8][4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const uint4& q = c < 2 ? qa : qb;
      int x0 = half16(q.x, c & 1);
      const int x1 = half16(q.y, c & 1), x2 = half16(q.z, c & 1), x3 = half16(q.w, c & 1);
      if (c == 0) x0 += 4;  // DESCALE's rounding term, carried through both linear DC paths
      int y[8];
      idct8_lo(x0, x1, x2, x3, y);
#pragma unroll
      for (int r = 0; r < 8; r++) ws[r][c] = y[r];
    }
#pragma unroll
    for (int r = 0; r < 8; r++) {
      int y[8];
      idct8_lo(ws[r][0], ws[r][1], ws[r][2], ws[r][3], y);
      putr(y);
    }
  }
}

// The full 8x8 transform of a live block: `my` is the lane's coefficient scratch (lane `lane` of `s_lds`), the eight rows
// are handed to `put` (clamped and packed, row 0 first).  Called by the lanes that have a live block.  Where every such
// block of the wave is inside the packed passes' 16-bit budget (pk_range_full, rtj_idct_pk.h: every legal picture) the
// packed passes run and the result is true.  Otherwise the result is false, and
//   kOwnPasses: the one-value-per-register passes (rtj_idct_asm.h) ran instead;
//   else:       nothing was stored — the caller leaves the part to k_decode_list (DecList above).  Those passes size the
//               register file of every path of a kernel that holds them.
template <bool kOwnPasses, class Put>
__device__ __forceinline__ bool transform_full(const uint4* my, uint32_t* s_lds, int lane, const IdctK& K,
                                               const IdctPK& KP, Put&& put) {
  uint4 q[8];
#pragma unroll
  for (int i = 0; i < 8; i++) q[i] = my[i];
  const bool packed = __all(pk_range_full(q, KP));  // wave-uniform
  if (packed) {
    // ---- column pass on the four column pairs, as they lie in the scratch (rtj_idct_pk.h) ----
    uint32_t yy[4][8];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      uint32_t x[8] = {q[2 * j].x,     q[2 * j].y,     q[2 * j].z,     q[2 * j].w,
                       q[2 * j + 1].x, q[2 * j + 1].y, q[2 * j + 1].z, q[2 * j + 1].w};
      if (j == 0) idct8_pk_col<true>(x, KP);
      else idct8_pk_col<false>(x, KP);
#pragma unroll
      for (int r = 0; r < 8; r++) yy[j][r] = x[r];
    }
    // ---- row pass on the four row pairs + scatter ----
#pragma unroll
    for (int r = 0; r < 8; r += 2) {
      uint2 o0, o1;
      uint32_t ya[4] = {yy[0][r], yy[1][r], yy[2][r], yy[3][r]};
      uint32_t yb[4] = {yy[0][r + 1], yy[1][r + 1], yy[2][r + 1], yy[3][r + 1]};
      idct8_pk_row_px(ya, yb, o0, o1, KP);
      put(o0);
      put(o1);
    }
  }
  if (kOwnPasses && !packed) {
    // ---- column pass: column c is one half of the 16-byte pieces c & ~1 (rows 0-3) and (c & ~1) + 1 (rows 4-7) ----
    // Two rounds, rows 0-3 and rows 4-7, each with a column pass of its own: this path is the rare one (a block
    // outside the 16-bit budget), and 32 + 32 registers of column results are what the kernel's register count —
    // and with it the waves per SIMD of EVERY path — would be sized for.  (The scratch is read again, through
    // an address the compiler cannot tell from the one above, or the 32 registers of the range test stay alive
    // as well.)
    uint32_t again = (uint32_t)lane * (uint32_t)(kCoefStride * 2);
    asm volatile("" : "+v"(again));
    const uint4* mq = (const uint4*)((const uint8_t*)s_lds + again);
#pragma unroll
    for (int half = 0; half < 2; half++) {
      int ws[4][8];
      int y[8];
      idct8_col<true, false>(mq[0], mq[1], y, K);
#pragma unroll
      for (int r = 0; r < 4; r++) ws[r][0] = y[4 * half + r];
#pragma unroll
      for (int c = 1; c < 8; c++) {
        if (c & 1) idct8_col<false, true>(mq[c - 1], mq[c], y, K);
        else idct8_col<false, false>(mq[c], mq[c + 1], y, K);
#pragma unroll
        for (int r = 0; r < 4; r++) ws[r][c] = y[4 * half + r];
      }
#pragma unroll
      for (int r = 0; r < 4; r++)
        put(idct8_row_px(ws[r][0], ws[r][1], ws[r][2], ws[r][3], ws[r][4], ws[r][5], ws[r][6], ws[r][7], K));
      asm volatile("" : "+v"(again));  // (keeps the second round's column pass from being merged into the first)
      mq = (const uint4*)((const uint8_t*)s_lds + again);
    }
  }
  return packed;
}

// vector-memory stores every transform variant of decode_wave issues per live wave and iteration (eight rows of 8 bytes
// per lane); the counted wait behind them is written for exactly this number
constexpr int kRowStores = 8;
static_assert(kRowStores == 8, "the wait block of decode_wave spells vmcnt(8)");
// kRot: a wave takes kParts parts of its groups in turn, starting with part0 (kParts = 3: the batches of round 2 and 3;
// kParts = 2: the luma waves of a batch whose chroma parts go to pooling waves, rtj_decode_chroma.h) / one part (span 1).
// kPrev: sessions — unchanged (0xFF) blocks are copied from the previous packet's picture.  kList: a wave that meets a
// block outside the packed passes' 16-bit budget leaves its part of the group to k_decode_list (DecList above) instead
// of running the one-value-per-register passes itself: those passes size the register file of every path (108 vector
// registers with them, 4 waves per SIMD).  All compile-time: the instantiation a batch launch runs carries nothing of
// the other forms.  The wave is told what it works on (frame row `fidx`, `slot` of `slots`, first part `part0`) by its
// kernel.
// kSuper (the split form's luma waves): the wave's groups are given in SUPER GROUPS of three consecutive groups — `slot` is
// its first super group, `slots` the step to its next one — so that the luma waves and the pooling chroma wave that work
// on the same stretch of a packet can be placed on the same XCD (k_decode_split).
template <bool kRot, bool kPrev, int kParts, bool kList, bool kSuper = false>
__device__ __forceinline__ void decode_wave(uint32_t* __restrict__ s_lds, const FrameDev* __restrict__ frames,
                                            const uint32_t fidx, const uint32_t slot, const uint32_t slots,
                                            const uint32_t part0, const uint8_t* __restrict__ stream,
                                            const QTab* __restrict__ lut, const uint32_t* __restrict__ blkoff,
                                            uint8_t* __restrict__ outbuf, const uint8_t* __restrict__ prev,
                                            const DecList list) {
  uint32_t* s_tab = s_lds + kCoefWords;

  const FrameDev f = frames[fidx];
  // One part per wave (span 1): the three parts of a slot are dispatched one after the other and (workgroups are dealt
  // round-robin to the 8 XCDs) land on different XCDs — see decode_slots().  Several parts per wave: a group's stream
  // bytes and block offsets come over the fabric once.
  constexpr bool rot = kRot;
  const uint32_t ngroups = (f.nmb + (uint32_t)kMbPerGroup - 1u) / (uint32_t)kMbPerGroup;
  // the g-th group of this wave (wave-uniform): every `slots`-th group from `slot` on, or (kSuper) three in a row from
  // every `slots`-th super group
  auto group_of = [&](uint32_t g) -> uint32_t {
    if (!kSuper) return slot + g * slots;
    const uint32_t q = g / 3u;
    return 3u * (slot + q * slots) + (g - 3u * q);
  };
  if (group_of(0u) >= ngroups) return;
  const int lane = threadIdx.x & 63;
  const uint32_t* off = uniform_ptr(blkoff + f.blk_base);
  const QTab& qt = lut[f.qidx];
  {
    const int nat = c_zz[lane];
    const uint32_t where = (uint32_t)coef_byte(nat);
    s_tab[lane] = ((uint32_t)qt.liqt[nat] << 16) | where;  // dequantisers: 0 .. 13984
    s_tab[kSlotTabN + lane] = ((uint32_t)qt.ciqt[nat] << 16) | where;
    if (lane < kSlotTabN - 64) {  // finished: multiplier 0, scratch slot 64 (write-only)
      s_tab[64 + lane] = 128u;
      s_tab[kSlotTabN + 64 + lane] = 128u;
    }
  }
  wave_lds_sync();  // orders the table write before the lanes' reads (the table is the wave's own)
  const uint32_t my_a = lds_address(s_lds) + (uint32_t)lane * (uint32_t)(kCoefStride * 2);
  const int k63 = 63;
  const uint4* my = (const uint4*)((const uint8_t*)s_lds + (size_t)lane * (kCoefStride * 2));
  // what depends on the part in hand (wave-uniform; set at the top of every iteration)
  int chroma = part0 == 2u;
  const uint32_t bt8_y = (uint32_t)qt.lb8, bt8_c = (uint32_t)qt.cb8;
  uint32_t bt8 = chroma ? bt8_c : bt8_y;
  uint32_t tab_a = lds_address(s_tab) + (chroma ? 4u * (uint32_t)kSlotTabN : 0u);
  int ca_end = (int)tab_a + 4 * 64;  // slot counter (see below) of a finished block
  const uint8_t* data = uniform_ptr(stream + f.data_off);
  // iteration `it` of this wave: which group, which block of it, and is there one (per lane)
  struct Src {
    uint32_t grp, dmb, kblk, mb, part;  // part: wave-uniform
    bool valid;
  };
  auto source = [&](uint32_t it) -> Src {
    Src r;
    uint32_t g = it;
    r.part = part0;
    if (rot) {
      g = it / (uint32_t)kParts;
      r.part = part0 + it - (uint32_t)kParts * g;
    }
    r.grp = group_of(g);
    r.dmb = r.part == 2u ? (uint32_t)(lane & 31) : (uint32_t)(lane >> 1);
    r.kblk = r.part == 2u ? 4u + (uint32_t)(lane >> 5) : 2u * r.part + (uint32_t)(lane & 1);
    r.mb = r.grp * (uint32_t)kMbPerGroup + r.dmb;
    r.valid = (kSuper || g < (uint32_t)kDecIters) && r.grp < ngroups && r.mb < f.nmb;  // (kSuper: as many groups as the wave's share has)
    if constexpr (kSuper) {
      // the same, with the group's share of the test on the scalar side: the macroblocks the picture has left from the
      // group's first one on (a group below ngroups starts below nmb), against the lane's place in the group
      const uint32_t left = r.grp < ngroups ? f.nmb - r.grp * (uint32_t)kMbPerGroup : 0u;  // wave-uniform
      r.valid = r.dmb < left;
    }
    return r;
  };
  // index into `off` of the block of `s`: 6 * mb + kblk.  kSuper (luma parts only: kblk = 2 * part + (lane & 1),
  // dmb = lane >> 1): the group's and the part's share is wave-uniform and the lane's a constant, so that the sum costs
  // an addition per use where the product cost a 32-bit multiplication (a quarter-rate instruction) and three more
  auto index_of = [&](const Src& s) -> uint32_t {
    if constexpr (kSuper)
      return (s.grp * (uint32_t)(6 * kMbPerGroup) + 2u * s.part) + (6u * (uint32_t)(lane >> 1) + (uint32_t)(lane & 1));
    return 6u * s.mb + s.kblk;
  };
  auto more_after = [&](uint32_t it) -> bool {  // wave-uniform: is there an iteration it + 1
    const uint32_t g = rot ? (it + 1u) / (uint32_t)kParts : it + 1u;
    return (kSuper || g < (uint32_t)kDecIters) && group_of(g) < ngroups;
  };

  // the dword that holds stream byte `p` and the four after it, bytes at or past data_len read as 0;
  // `inside`: every lane's loads are known to lie inside the packet
  struct Bytes {
    uint32_t d[9];
  };
  auto fetch = [&](uint32_t p, bool inside, int n) -> Bytes {
    const uint8_t* g = data + p;
    const uint32_t sh = (uint32_t)((uintptr_t)g & 3u);
    const uint32_t* g4 = (const uint32_t*)(g - sh);
    Bytes b;
    if (inside) {
#pragma unroll
      for (int k = 0; k < 9; k++)
        if (k < n) b.d[k] = g4[k];
      return b;
    }
    const long long rel = (long long)p - (long long)sh;  // position of g4[0]'s first byte
#pragma unroll
    for (int k = 0; k < 9; k++) {
      if (k < n) {
        const long long rem = (long long)f.data_len - (rel + 4ll * k);
        uint32_t v = 0;
        if (rem > 0) {
          v = g4[k];
          if (rem < 4) v &= (1u << (8 * (int)rem)) - 1u;
        }
        b.d[k] = v;
      }
    }
    return b;
  };

  // Vector-memory operations of a wave complete in issue order, loads and stores alike (one counter, vmcnt), so a
  // load issued behind the eight row stores of a group is only known to be complete once those stores are.  The
  // loop is therefore ordered so that nothing it waits for is younger than a store: a group's stream bytes AND the
  // block offset of the group after it are requested before the group in hand is transformed, and waited for
  // right behind its row stores with a counted wait, "all but the 8 youngest" (arrived_behind_stores below) — by
  // then they have had the whole transform to arrive.  The compiler cannot be made to place that wait: wherever
  // control flow joins it assumes the path with the fewest operations in flight and emits vmcnt(0) or vmcnt(1),
  // i.e. a wait for the stores.  These loads are therefore issued from inline assembly (the compiler does not know
  // they are pending) and waited for by hand; `next_bytes` and `pos_nn` must not be read before that wait.
  // (Round 1 loaded the offset at the top of the next iteration and the compiler waited with vmcnt(0) at the loop
  // end: every wave sat out the latency of its row stores once per group.)
  // where a block's eight rows go: a wave-uniform plane base (scalar registers) plus a 32-bit offset per lane, so that
  // the step from row to row is one plain 32-bit add with the stride in a vector register — the kind of instruction
  // that does not slow the transform's cheap stretches down (a 64-bit pointer step does, rtj_idct_asm.h).  Offsets
  // stay below 2^32: the luma plane of the largest picture the header can describe has 65520^2 bytes.
  const size_t ysz = (size_t)f.w * f.h;
  size_t plane_off = f.out_off + (chroma ? ysz : (size_t)0);  // wave-uniform
  uint32_t stride = chroma ? f.w >> 1 : f.w;
  auto block_offset = [&](uint32_t grp, uint32_t dmb, uint32_t kblk, uint32_t mb) -> uint32_t {
    // macroblock coordinates without a per-lane division: one scalar division for the group's
    // first macroblock, then at most one row wrap per lane when rows are at least a group wide
    uint32_t mx, my_;
    const uint32_t mbw = f.mbw, mb0 = grp * (uint32_t)kMbPerGroup;
    const uint32_t gy = mb0 / mbw, gx = mb0 - gy * mbw;  // uniform in k_decode
    if constexpr (kSuper) {
      // luma parts only (kblk >> 1 is the part, wave-uniform).  Rows at least a group wide: what the group and the part
      // decide is added up on the scalar side, the lane's share is a constant, and a lane on the next macroblock row
      // (dmb >= mbw - gx) adds the step to it: one test and one selection per lane.  (Modulo 2^32 like every offset
      // here; the sum is the block's offset, below 2^32.)
      if (mbw >= (uint32_t)kMbPerGroup) {
        uint32_t st = stride;
        asm volatile("" : "+s"(st));  // (worked out where it is used: held across the loop it is one more spilled scalar)
        const uint32_t base = (16u * gy + 8u * (kblk >> 1)) * stride + 16u * gx;  // wave-uniform
        const uint32_t wrap_step = 16u * (st - mbw);                              // wave-uniform
        return base + (16u * dmb + 8u * (kblk & 1u)) + (dmb >= mbw - gx ? wrap_step : 0u);
      }
      my_ = mb / mbw;
      mx = mb - my_ * mbw;
      return (16u * my_ + 8u * (kblk >> 1)) * stride + 16u * mx + 8u * (kblk & 1u);
    }
    if (mbw >= (uint32_t)kMbPerGroup) {
      const bool wrap = gx + dmb >= mbw;
      mx = wrap ? gx + dmb - mbw : gx + dmb;
      my_ = wrap ? gy + 1u : gy;
    } else {
      my_ = mb / mbw;
      mx = mb - my_ * mbw;
    }
    return chroma ? (kblk == 5u ? (uint32_t)(ysz >> 2) : 0u) + 8u * my_ * stride + 8u * mx
                  : (16u * my_ + 8u * (kblk >> 1)) * stride + 16u * mx + 8u * (kblk & 1u);
  };

  // (which block a lane has in an iteration is worked out afresh where it is needed — a handful of instructions —
  // instead of being carried from iteration to iteration in vector registers: the register count decides how many
  // waves a SIMD holds)
  const Src s0 = source(0u), s1 = source(1u);
  uint32_t pos0 = off[s0.valid ? index_of(s0) : 0u];  // block start relative to the first data byte
  uint32_t pos_n = off[s1.valid ? index_of(s1) : 0u];  // the same for the wave's next iteration
  pos0 = s0.valid ? pos0 : 0u;
  bool inside = !kForceGenericPaths && __all(pos0 + kFetchSpan <= f.data_len);  // wave-uniform
  Bytes cur = fetch(pos0, inside, 9);  // 32 bytes (+ alignment): all of most blocks
  bool try_lo_y = true, try_lo_c = true;  // wave-uniform: test this wave's luma / chroma blocks for "low 4x4 only" until a test fails
  // the first group's loads are waited for here, not inside the loop: a wait at the top of the loop would be a
  // wait for everything in flight (it could not tell the first entry from the back edge), the row stores included
  asm volatile("" ::"v"(cur.d[0]), "v"(cur.d[1]), "v"(cur.d[2]), "v"(cur.d[3]), "v"(cur.d[4]), "v"(cur.d[5]),
               "v"(cur.d[6]), "v"(cur.d[7]), "v"(cur.d[8]), "v"(pos_n));


  uint32_t exit_grp = ~0u, exit_part = 0u;  // (kList) the last round's part goes to the list: appended behind the loop
  for (uint32_t it = 0;;) {
    const bool have_n = more_after(it);  // wave-uniform
    const Src s0 = source(it);
    const bool valid = s0.valid, valid_n = have_n && source(it + 1u).valid;
    const uint32_t grp = s0.grp, dmb = s0.dmb, kblk = s0.kblk, mb = s0.mb;
    pos_n = valid_n ? pos_n : 0u;
    if (rot) {  // the part in hand
      chroma = s0.part == 2u;
      bt8 = chroma ? bt8_c : bt8_y;
      tab_a = lds_address(s_tab) + (chroma ? 4u * (uint32_t)kSlotTabN : 0u);
      ca_end = (int)tab_a + 4 * 64;
      plane_off = f.out_off + (chroma ? ysz : (size_t)0);
      stride = chroma ? f.w >> 1 : f.w;
    }

    const uint32_t sh = (uint32_t)((uintptr_t)(data + pos0) & 3u);
    uint32_t d0 = cur.d[0], d1 = cur.d[1], d2 = cur.d[2], d3 = cur.d[3], d4 = cur.d[4];
    // unchanged block: previous pixels stay (lib/RTjpeg.c:2704)
    const uint32_t first4 = __builtin_amdgcn_alignbyte(d1, d0, sh);
    const bool live_any = valid && (first4 & 0xFFu) != 0xFFu;

    const bool live_blk = live_any;  // the lanes of this iteration's transform round
    bool rows_stored = true;         // (kList) false: the part was left to k_decode_list
    uint32_t nstored = 0;            // row stores this lane issued in this iteration (a constant on every path: the loops are unrolled)

    if (live_blk) {
      // ---- stream -> dequantised coefficients, int16, transposed (lib/RTjpeg.c:157-186) ----
      // The block's bytes are consumed 16 at a time from registers (aligned dwords + a byte funnel
      // shift), eight to a half round so that short blocks stop early.  The only loop-carried value
      // is the slot counter `ca` = LDS address of the next slot's table entry.
      {
        uint4* z = (uint4*)my;
#pragma unroll
        for (int i = 0; i < 8; i++) z[i] = make_uint4(0, 0, 0, 0);
      }
      uint32_t wd[4] = {__builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh),
                        __builtin_amdgcn_alignbyte(d3, d2, sh), __builtin_amdgcn_alignbyte(d4, d3, sh)};
      int ca = (int)tab_a + 4 * ((int)bt8 + 1);  // DC and the raw bytes have their slots fixed

      // Eight bytes t0..t0+7 of the current 16.  A token is one coefficient or (64..127) a run of
      // token-63 zero slots (lib/RTjpeg.c:171-182); DC (unsigned; 0xFF was handled above) and raw byte t,
      // 1 <= t <= bt8 (signed), sit at slot t.  The slot counter only depends on the bytes, so all
      // eight table reads are issued before the first product is needed.
      auto half_round = [&](int t0, auto b8c, bool first) {
        constexpr int B8 = decltype(b8c)::value;
        int svb[8];
        uint32_t e[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const int t = t0 + k;
          const uint32_t w = wd[t >> 2];
          const bool is_raw = first && (B8 >= 0 ? t <= B8 : t <= (int)bt8);
          if (is_raw) {
            e[k] = *(const lds_u32_t*)(uintptr_t)(tab_a + 4u * (uint32_t)t);
            svb[k] = 0;
          } else {
            svb[k] = sbyte_minus(w, t & 3, k63);  // token - 63: > 0 for a run, its length
            e[k] = *(const lds_u32_t*)(uintptr_t)(uint32_t)ca;
            ca = med3_i32(ca + 4, (svb[k] << 2) + ca, ca_end);  // == min(ca + 4 * max(1, svb), end) below the end
          }
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const int t = t0 + k;
          const uint32_t w = wd[t >> 2];
          const bool is_raw = first && (B8 >= 0 ? t <= B8 : t <= (int)bt8);
          if (is_raw) {
            *(lds_i16_t*)(uintptr_t)(my_a + (uint32_t)slot_byte(t)) = (int16_t)mul_byte_hi16(w, e[k], t & 3, t != 0);
          } else {
            int prod = mul_byte_hi16(w, e[k], t & 3, true);  // |byte| < 2^8, dequantiser < 2^14; stored as int16
            prod = svb[k] > 0 ? 0 : prod;
            *(lds_i16_t*)(uintptr_t)(my_a + (e[k] & 0xFFFFu)) = (int16_t)prod;
          }
        }
        ca = min(ca, ca_end);
        return (bool)__any(ca < ca_end);
      };
      // first 16 bytes; B8 >= 0: bt8 known at compile time
      bool more = true;
      auto first_round = [&](auto b8c) {
        more = half_round(0, b8c, true);
        if (more) more = half_round(8, b8c, true);
      };
      switch (kForceGenericPaths ? 99u : bt8) {
        case 9: first_round(std::integral_constant<int, 9>{}); break;
        case 8: first_round(std::integral_constant<int, 8>{}); break;
        case 4: first_round(std::integral_constant<int, 4>{}); break;
        case 0: first_round(std::integral_constant<int, 0>{}); break;
        default: first_round(std::integral_constant<int, -1>{}); break;
      }
      if (more) {
        // bytes 16..31 are in registers already
        wd[0] = __builtin_amdgcn_alignbyte(cur.d[5], d4, sh);
        wd[1] = __builtin_amdgcn_alignbyte(cur.d[6], cur.d[5], sh);
        wd[2] = __builtin_amdgcn_alignbyte(cur.d[7], cur.d[6], sh);
        wd[3] = __builtin_amdgcn_alignbyte(cur.d[8], cur.d[7], sh);
        more = half_round(0, std::integral_constant<int, -1>{}, false);
        if (more) more = half_round(8, std::integral_constant<int, -1>{}, false);
      }
      uint32_t pnext = pos0 + 16u;
      while (more) {  // blocks longer than 32 bytes: fetched on demand
        pnext += 16u;
        const Bytes nb = fetch(pnext, inside, 5);  // same alignment as pos0
        wd[0] = __builtin_amdgcn_alignbyte(nb.d[1], nb.d[0], sh);
        wd[1] = __builtin_amdgcn_alignbyte(nb.d[2], nb.d[1], sh);
        wd[2] = __builtin_amdgcn_alignbyte(nb.d[3], nb.d[2], sh);
        wd[3] = __builtin_amdgcn_alignbyte(nb.d[4], nb.d[3], sh);
        more = half_round(0, std::integral_constant<int, -1>{}, false);
        if (more) more = half_round(8, std::integral_constant<int, -1>{}, false);
      }
    }

    // ---- sessions with packets in flight give every packet a picture of its own: its unchanged (0xFF) blocks are
    // then fetched from the previous packet's picture (`prev`), which is what "left as it was" means there ----
    if (kPrev) {
      const bool keep = valid && !live_any;
      if (keep) {
        uint32_t o = block_offset(grp, dmb, kblk, mb);
        const uint8_t* src = prev + plane_off - f.out_off;  // the previous picture has the same layout, at its own base
        uint8_t* const dstp = outbuf + plane_off;
#pragma unroll
        for (int r = 0; r < 8; r++) {
          *(uint2*)(dstp + o) = *(const uint2*)(src + o);
          o += stride;
        }
      }
    }
    // ---- request the next group's stream bytes and the block offset of the group after it: they arrive while
    // this group is transformed ----
    typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
    u32x4_t nb0, nb1;
    uint32_t nb2, pos_nn;
    bool inside_n = false;
    if (have_n) {
      inside_n = !kForceGenericPaths && __all(pos_n + kFetchSpan <= f.data_len);
      const Src s2 = source(it + 2u);
      // addresses as a wave-uniform base (scalar registers) plus a 32-bit byte offset per lane: no 64-bit vector
      // arithmetic (a packet is shorter than 2^32 bytes; the index of a packet has fewer than 2^30 entries)
      const uint32_t offp = s2.valid ? 4u * index_of(s2) : 0u;
      const uint8_t* g4b = data - ((uintptr_t)data & 3u);  // uniform
      uint32_t g4o = (pos_n + (uint32_t)((uintptr_t)data & 3u)) & ~3u;
      // near the packet's end (rare) the bytes are fetched with masks, behind the wait at the end of this iteration —
      // fetched here they would occupy nine registers across the transform on every path; the hand-issued loads
      // below then read this packet's descriptor (64 valid bytes) instead
      if (!inside_n) {
        g4b = (const uint8_t*)uniform_ptr(frames + fidx);
        g4o = 0u;
      }
      // one block, issued on every path that has a next group: its results take part in no selection before the
      // wait (a selection could be a register copy, and a copy of a register that is still being filled is wrong)
      // (s_nop 4: a vector-memory instruction must not read a scalar register within five wait states of a vector
      // instruction writing it — v_readlane_b32 reloading a spilled base, say — and the compiler, which pads such
      // hazards in its own code, does not look inside an asm block.  The test build hit exactly that.)
      asm volatile(
          "s_nop 4\n\t"
          "global_load_dwordx4 %0, %4, %5\n\t"
          "global_load_dwordx4 %1, %4, %5 offset:16\n\t"
          "global_load_dword %2, %4, %5 offset:32\n\t"
          "global_load_dword %3, %6, %7 ; mirtj luma loads"
          : "=&v"(nb0), "=&v"(nb1), "=&v"(nb2), "=&v"(pos_nn)
          : "v"(g4o), "s"(g4b), "v"(offp), "s"(off)
          : "memory");
    }

    // ---- does any block of the wave reach outside the low 4x4?  (columns 4-7, rows 4-7) ----
    bool lo = false;
    const bool try_lo = chroma ? try_lo_c : try_lo_y;
    if (try_lo) {  // wave-uniform
      uint32_t hi = 0;
      if (live_blk) {
#pragma unroll
        for (int i = 0; i < 8; i++) {
          if (i == 0 || i == 2) continue;  // rows 0-3 of columns 0-3
          const uint4 q = my[i];
          hi |= q.x | q.y | q.z | q.w;
        }
      }
      lo = !__any(hi != 0u);
      if (chroma) try_lo_c = lo;
      else try_lo_y = lo;
    }

    if (live_blk) {
      const uint32_t off32 = block_offset(grp, dmb, kblk, mb);
      uint8_t* plane = outbuf + plane_off;  // wave-uniform; steps from row to row on the scalar side
      auto put_packed = [&](uint2 o) {  // one row of the block, already clamped and packed
        // nontemporal (global_store_dwordx2 ... nt): the picture is not read again by this kernel, and the
        // stores are what a short chroma round waits for (-3.5 % on the kernel, v21_nontemporal_stores_ab.txt)
        typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
        u32x2_t ov;
        ov.x = o.x;
        ov.y = o.y;
        __builtin_nontemporal_store(ov, (u32x2_t*)(plane + off32));
        plane += stride;
        nstored++;
      };
      const IdctK K{362, 473, -669, 277, 128, 235};
      const IdctPK KP = idct_pk_constants();

      if (lo) {
        transform_lo(my, K, KP, put_packed);
      } else {
        const bool packed = transform_full<!kList>(my, s_lds, lane, K, KP, put_packed);
        if (kList && !packed) rows_stored = false;  // not this kernel's business: the whole part goes to k_decode_list
      }
    }
    // (appended behind the counted wait, or on the way out: the append is an atomic and a store, and nothing but the row
    // stores may sit between the hand-issued loads and their wait)
    const bool to_list = kList && __ballot(live_blk && !rows_stored) != 0ull;  // wave-uniform
    if (!have_n) {
      if (to_list) {
        exit_grp = grp;
        exit_part = s0.part;
      }
      break;
    }
    // Every transform variant ends with kRowStores row stores, so behind the join "all but the kRowStores youngest
    // operations" is exactly "everything requested before the transform" — unless no lane had a live block: such a wave
    // stored nothing and waits for all there is.  (kRowStores sits next to the stores it counts: put_packed above.)
    {
      // (structural, VERDICT r3 item 8: the count of stores the lanes with a block really issued — folded to a constant on
      // every path — decides the arm; a variant that issued another number than kRowStores waits for everything, which is
      // slower and never wrong.  The compiled text is still checked by tools/check_async_loads.py on every build.)
      const uint32_t younger = __ballot(live_blk && rows_stored && nstored == (uint32_t)kRowStores) != 0ull &&
                                       __ballot(live_blk && rows_stored && nstored != (uint32_t)kRowStores) == 0ull
                                   ? (uint32_t)kRowStores : 0u;
      asm volatile(
          "s_cmp_eq_u32 %4, 8\n\t"
          "s_cbranch_scc1 .Lmirtj_w8_%=\n\t"
          "s_waitcnt vmcnt(0)\n\t"
          "s_branch .Lmirtj_arrived_%=\n"
          ".Lmirtj_w8_%=:\n\t"
          "s_waitcnt vmcnt(8) ; mirtj luma wait\n"
          ".Lmirtj_arrived_%=:"
          : "+v"(nb0), "+v"(nb1), "+v"(nb2), "+v"(pos_nn)
          : "s"(younger)
          : "scc", "memory");
    }
    if (to_list) declist_push(list, fidx, grp, s0.part);
    pos0 = pos_n;
    // a copy of our own, BEHIND the wait: left to the compiler, the loop-carried register of pos_n may be filled by a
    // copy it places in front of the wait block (tools/check_async_loads.py found exactly that)
    asm volatile("v_mov_b32 %0, %1" : "=v"(pos_n) : "v"(pos_nn));
    if (inside_n) {
      cur.d[0] = nb0.x; cur.d[1] = nb0.y; cur.d[2] = nb0.z; cur.d[3] = nb0.w;
      cur.d[4] = nb1.x; cur.d[5] = nb1.y; cur.d[6] = nb1.z; cur.d[7] = nb1.w;
      cur.d[8] = nb2;
    } else {
      cur = fetch(pos0, false, 9);
    }
    inside = inside_n;
    it++;
  }
  if (kList && exit_grp != ~0u) declist_push(list, fidx, exit_grp, exit_part);
}

// k_decode<kRot, kPrev>: see above.  kRot: grid (slots, frames), a wave takes all three parts of its groups; else grid
// (3 * slots, frames).  kPrev false: unchanged (0xFF) blocks keep what the output buffer holds; true: they are copied
// from the picture at `prev` (same layout as the output buffer: frame i of the plan at prev + its out_off).
template <bool kRot, bool kPrev>
__global__ __launch_bounds__(kDecThreads, MIRTJ_DEC_WAVES) void k_decode(const FrameDev* __restrict__ frames,
                                                         const uint8_t* __restrict__ stream,
                                                         const QTab* __restrict__ lut,
                                                         const uint32_t* __restrict__ blkoff,
                                                         uint8_t* __restrict__ outbuf,
                                                         const uint8_t* __restrict__ prev,
                                                         const uint32_t* __restrict__ only_in_mode) {
  // (batches: the plan's decode policy — rtj_decode_chroma.h, DecPolicy — says whether this form or k_decode_split runs)
  if (only_in_mode && *only_in_mode != kDecModeClassic) return;
  __shared__ __attribute__((aligned(16))) uint32_t s_lds[kDecLdsWords];
  const uint32_t slots = kRot ? gridDim.x : gridDim.x / 3u;
  const uint32_t slot = kRot ? blockIdx.x : blockIdx.x / 3u, part0 = kRot ? 0u : blockIdx.x - slot * 3u;
  decode_wave<kRot, kPrev, 3, false>(s_lds, frames, blockIdx.y, slot, slots, part0, stream, lut, blkoff, outbuf, prev,
                                     DecList{nullptr, nullptr, 0u});
}

}  // namespace mirtj
