// dv_hold_kernels.h — phase 2 of mi_dv_decode_batch_held: macroblocks a DV stream flags as errors keep the stream's
// last good pixels (gfx950).  DESIGN.md section 9.6.
//
// A run is a stretch of consecutive frames of a batch that are consecutive pictures of one stream.  Phase 1 is
// k_dv_decode<Sys> over the whole batch, unchanged: it writes every macroblock of every picture, flagged ones included.
// A macroblock is flagged when bit STA (the high nibble of byte 3 of its DIF block) is set in the caller's 16-bit mask.
// Macroblock m of picture k of a run then is macroblock m of the nearest earlier picture j < k of the run in which m is
// good; else of the run's picture of d_prev (the stream's picture before the run), where the caller gave one; else it
// stays what the decoder made of it.  The source is resolved with a segmented "last good" scan over chunks of kHoldChunk
// pictures, as rtj_runs_kernels.h does for unchanged RTjpeg blocks; kernel boundaries are the only ordering between the
// passes:
//
//   k_dv_hold_mask   per (chunk, macroblock), a wave each: 64-bit mask of the chunk's pictures in which the macroblock
//                    is good
//   k_dv_hold_carry  per (run, macroblock), serially over the run's chunks only: the source a chunk's first picture
//                    inherits (the last good picture of an earlier chunk, else -1: none in the run); zeroes the count
//   k_dv_hold_copy   per (kHoldSub pictures of a chunk, super block of 27 macroblocks): resolves every flagged
//                    macroblock from the mask and the carry and copies its three rectangles (Sys::rects, dv_common.h)
//
// Copies write flagged macroblocks only, and read good macroblocks or d_prev, which phase 1 has finished and phase 2
// never writes: one copy pass needs no ordering among its own workgroups.  Every loop is bounded by a count the host
// passes (pictures of a chunk <= 64, chunks of a run, work items).
#pragma once
#include <hip/hip_runtime.h>

#include "dv_common.h"

namespace midv {

constexpr int kHoldChunk = 64;                      // pictures per scan chunk (one bit each in a 64-bit mask)
constexpr int kHoldSub = 8;                         // pictures per copy workgroup
constexpr int kHoldSubs = kHoldChunk / kHoldSub;    // copy workgroups per chunk and super block
constexpr int kHoldCopyThreads = 192;               // one lane per 64-byte piece of a super block: three waves
constexpr int kHoldScanThreads = 256;
constexpr int kHoldMaskMbs = kHoldScanThreads / 64; // macroblocks per workgroup of k_dv_hold_mask: one wave each
constexpr uint32_t kHoldMaxGridY = 65535u;          // the kernels loop over their work items past this
// The count of copied macroblocks is kHoldCounters partial counts, each on a 128-byte line of its own: a wave adds to the
// one its number picks, so that the adds of a launch (up to one per wave, all at the memory side) do not queue behind
// each other at one address; the host sums them.
constexpr int kHoldCounters = 64, kHoldCounterStride = 16;  // (in counters: 128 bytes)

// One chunk of a run (device view).  Rows of the mask / carry arrays are [chunk][macroblocks of a frame].
struct HoldChunkDev {
  uint32_t frame0;  // batch index of the run's picture 0
  uint32_t rel0;    // run-relative index of the chunk's first picture
  uint32_t count;   // pictures in the chunk, 1..kHoldChunk
  uint32_t run;     // the run's number: its picture of d_prev
};
static_assert(sizeof(HoldChunkDev) == 16, "HoldChunkDev layout");

// One run that needs phase 2 (two or more pictures, or a picture of d_prev).
struct HoldRunDev {
  uint32_t chunk0;  // its first chunk in the chunk array
  uint32_t nchunks;
};
static_assert(sizeof(HoldRunDev) == 8, "HoldRunDev layout");

// byte 3 (STA | QNO) of macroblock mb = 5 (27 seq + slot) + m of a frame: DIF block 7 + v + v / 15 of its sequence
MIDV_HD uint32_t hold_sta_offset(uint32_t mb) {
  const uint32_t S = mb / 5u, m = mb - 5u * S, seq = S / 27u, slot = S - 27u * seq, v = 5u * slot + m;
  return (seq * 150u + 7u + v + v / 15u) * 80u + 3u;
}

// grid (ceil(nmb / kHoldMaskMbs), min(chunks, 65535)), 256 threads: one wave per macroblock of a chunk, one lane per picture (the
// chunk's pictures are the 64 bits of one ballot), one byte per DIF block.  The bytes of a macroblock lie a frame apart
// and those of neighbouring macroblocks a DIF block apart: every read is a cache line of its own whichever way the lanes
// lie, and this way all of a chunk's reads are in flight at once.
__global__ __launch_bounds__(kHoldScanThreads) void k_dv_hold_mask(const uint8_t* __restrict__ frames, uint32_t frame_bytes,
                                                                   uint32_t nmb, const HoldChunkDev* __restrict__ chunks,
                                                                   uint32_t nchunks, uint32_t sta_mask,
                                                                   uint64_t* __restrict__ mask) {
  const uint32_t lane = threadIdx.x & 63u, mb = blockIdx.x * (uint32_t)kHoldMaskMbs + (threadIdx.x >> 6);
  if (mb >= nmb) return;  // (the whole wave)
  const uint32_t at = hold_sta_offset(mb);
  for (uint32_t c = blockIdx.y; c < nchunks; c += gridDim.y) {
    const HoldChunkDev ch = chunks[c];
    bool good = false;
    if (lane < ch.count) {
      const uint32_t sta = frames[(size_t)(ch.frame0 + ch.rel0 + lane) * frame_bytes + at] >> 4;
      good = !((sta_mask >> sta) & 1u);
    }
    const unsigned long long m = __ballot(good);
    if (lane == 0u) mask[(size_t)c * nmb + mb] = m;
  }
}

// grid (ceil(nmb / 256), min(runs, 65535)), 256 threads: one lane per macroblock of a run walks the run's chunks.
__global__ __launch_bounds__(kHoldScanThreads) void k_dv_hold_carry(const HoldRunDev* __restrict__ runs, uint32_t nruns,
                                                                    const HoldChunkDev* __restrict__ chunks, uint32_t nmb,
                                                                    const uint64_t* __restrict__ mask,
                                                                    int32_t* __restrict__ carry,
                                                                    unsigned long long* __restrict__ held) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < (uint32_t)kHoldCounters)
    held[threadIdx.x * kHoldCounterStride] = 0ull;  // k_dv_hold_copy of this launch counts
  const uint32_t mb = blockIdx.x * kHoldScanThreads + threadIdx.x;
  if (mb >= nmb) return;
  for (uint32_t r = blockIdx.y; r < nruns; r += gridDim.y) {
    const HoldRunDev run = runs[r];
    int32_t src = -1;  // no good picture in the run so far
#pragma unroll 4
    for (uint32_t c = 0; c < run.nchunks; c++) {
      const size_t row = (size_t)(run.chunk0 + c) * nmb + mb;
      const uint64_t good = mask[row];
      carry[row] = src;
      if (good) src = (int32_t)(chunks[run.chunk0 + c].rel0 + 63u - (uint32_t)__builtin_clzll(good));
    }
  }
}

// Thread t of a copy workgroup -> the macroblock (its segment slot) of super block (seq, m) and the 64-byte piece of it
// the lane copies: 0..3 the 8 x 8 parts of the luma rectangle in row-major order, 4 the Cb rectangle, 5 the Cr one.  The
// 27 macroblocks of a super block lie together in the picture (dv_common.h: place), and the lanes follow the picture's
// rows: consecutive lanes hold horizontally adjacent 8-byte columns of adjacent macroblocks, so that a wave's accesses
// to one pixel row are whole stretches of it (4:2:0 and 4:2:2: 144 bytes of luma per row of a super block; 4:1:1: up to
// 160).  false: the lane has no piece (4:1:1 super blocks are 4 1/2 columns of six; the workgroup's last lanes).
template <class Sys>
MIDV_HD bool hold_lane(uint32_t t, uint32_t m, uint32_t& slot, uint32_t& piece) {
  if constexpr (Sys::k411) {
    // columns k6 = 0..4 of six 32 x 8 macroblocks, walked downwards in even columns; k = slot + 3 where the super block
    // begins in mid-column (m 1, 2).  Column 22 of the picture is k6 = 4 of m = 4: three 16 x 16 macroblocks
    uint32_t row, k6;
    if (t < 120u) {  // luma: 6 rows of 20 blocks
      row = t / 20u;
      const uint32_t bx = t - 20u * row;
      k6 = bx >> 2;
      piece = bx & 3u;
    } else if (t < 180u) {  // chroma: Cb then Cr, 6 rows of 5 blocks
      const uint32_t u = t - 120u, pl = u / 30u, v = u - 30u * pl;
      row = v / 5u;
      k6 = v - 5u * row;
      piece = 4u + pl;
    } else {
      return false;
    }
    const uint32_t k = 6u * k6 + (k6 & 1u ? 5u - row : row), lead = m == 1u || m == 2u ? 3u : 0u;
    if (k < lead || k - lead > 26u) return false;
    slot = k - lead;
    return true;
  } else {
    // 9 columns x 3 rows of macroblocks, walked downwards in even columns; a macroblock is two luma blocks wide and
    // kRows high
    constexpr uint32_t kRows = Sys::kChans == 2 ? 1u : 2u, kLuma = 27u * 2u * kRows;
    uint32_t r, c;
    if (t < kLuma) {
      const uint32_t brow = t / 18u, bx = t - 18u * brow;
      r = brow / kRows;
      c = bx >> 1;
      piece = 2u * (brow - kRows * r) + (bx & 1u);
    } else if (t < kLuma + 54u) {
      const uint32_t u = t - kLuma, pl = u / 27u, v = u - 27u * pl;
      r = v / 9u;
      c = v - 9u * r;
      piece = 4u + pl;
    } else {
      return false;
    }
    slot = 3u * c + (c & 1u ? 2u - r : r);
    return true;
  }
}

// What thread t of the copy workgroup of super block (seq, m) copies: the macroblock mb of the frame, and its piece as
// 64 / w rows of w bytes (w 8, or 4 for the split chroma halves of 4:1:1's column 22) `stride` apart, the first at byte
// `off` of the picture.  From Sys::rects alone; host and device, so that a host program can walk every lane of every
// workgroup and see the pieces tile the picture.  false: the lane is idle.
template <class Sys>
MIDV_HD bool hold_piece(uint32_t seq, uint32_t m, uint32_t t, uint32_t& mb, uint32_t& piece, uint32_t& off, uint32_t& stride,
                        uint32_t& w) {
  uint32_t slot = 0;
  if (seq >= (uint32_t)(Sys::kChans * Sys::kSeqs) || m >= 5u || !hold_lane<Sys>(t, m, slot, piece)) return false;
  mb = 5u * (27u * seq + slot) + m;
  Rect rc[3];
  Sys::rects(seq, slot, m, rc);
  if (piece < 4u) {
    const uint32_t nbx = rc[0].w >> 3, by = piece / nbx, bx = piece - nbx * by;
    stride = Sys::kW;
    off = (rc[0].y + 8u * by) * stride + rc[0].x + 8u * bx;
    w = 8u;
  } else {
    const Rect q = piece == 4u ? rc[1] : rc[2];
    stride = Sys::kCW;
    off = (uint32_t)(Sys::kW * Sys::kH) + (piece == 5u ? (uint32_t)(Sys::kCW * Sys::kCH) : 0u) + q.y * stride + q.x;
    w = q.w;
  }
  return true;
}

// grid (super blocks of a frame, min(chunks * kHoldSubs, 65535)), 192 threads.  prev: the runs' pictures before them,
// back to back, or nullptr.
template <class Sys>
__global__ __launch_bounds__(kHoldCopyThreads) void k_dv_hold_copy(const HoldChunkDev* __restrict__ chunks, uint32_t nitems,
                                                                   const uint64_t* __restrict__ mask,
                                                                   const int32_t* __restrict__ carry,
                                                                   uint8_t* __restrict__ pics, const uint8_t* __restrict__ prev,
                                                                   unsigned long long* __restrict__ held) {
  constexpr uint32_t kNmb = (uint32_t)Sys::kSegments * 5u;
  typedef uint32_t u32x2a __attribute__((ext_vector_type(2), aligned(4)));  // (a 180-byte chroma row is 4-byte aligned)
  const uint32_t t = threadIdx.x;
  const uint32_t seq = blockIdx.x / 5u, m = blockIdx.x - 5u * seq;
  uint32_t mb = 0, piece = 0, off = 0, stride = 0, w = 8;
  uint32_t done = 0;
  if (hold_piece<Sys>(seq, m, t, mb, piece, off, stride, w)) {
    for (uint32_t it = blockIdx.y; it < nitems; it += gridDim.y) {
      const uint32_t c = it / (uint32_t)kHoldSubs;
      const HoldChunkDev ch = chunks[c];
      const uint32_t j0 = (it - c * (uint32_t)kHoldSubs) * (uint32_t)kHoldSub;
      const uint32_t count = ch.count < (uint32_t)kHoldChunk ? ch.count : (uint32_t)kHoldChunk;
      if (j0 >= count) continue;
      const uint64_t good = mask[(size_t)c * kNmb + mb];
      const int32_t cin = carry[(size_t)c * kNmb + mb];
      const uint32_t jn = count < j0 + (uint32_t)kHoldSub ? count : j0 + (uint32_t)kHoldSub;
      for (uint32_t j = j0; j < jn; j++) {
        if ((good >> j) & 1ull) continue;  // phase 1 wrote it
        const uint64_t below = good & ((1ull << j) - 1ull);
        const int32_t src = below ? (int32_t)(ch.rel0 + 63u - (uint32_t)__builtin_clzll(below)) : cin;
        const uint8_t* s;
        if (src >= 0) s = pics + (size_t)(ch.frame0 + (uint32_t)src) * Sys::kPicBytes + off;
        else if (prev) s = prev + (size_t)ch.run * Sys::kPicBytes + off;
        else continue;  // no source: the macroblock keeps what the decoder made of it
        uint8_t* d = pics + (size_t)(ch.frame0 + ch.rel0 + j) * Sys::kPicBytes + off;
        if (!Sys::k411 || w == 8u) {
          u32x2a v[8];
#pragma unroll
          for (int r = 0; r < 8; r++) v[r] = *(const u32x2a*)(s + (uint32_t)r * stride);
#pragma unroll
          for (int r = 0; r < 8; r++) *(u32x2a*)(d + (uint32_t)r * stride) = v[r];
        } else {
          uint32_t v[16];
#pragma unroll
          for (int r = 0; r < 16; r++) v[r] = *(const uint32_t*)(s + (uint32_t)r * stride);
#pragma unroll
          for (int r = 0; r < 16; r++) *(uint32_t*)(d + (uint32_t)r * stride) = v[r];
        }
        done += piece == 0u;  // once per macroblock
      }
    }
  }
  // one atomic per wave
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) done += __shfl_xor(done, o);
  if ((t & 63u) == 0u && done)
    atomicAdd(held + ((3u * blockIdx.x + (t >> 6) + 7u * blockIdx.y) % (uint32_t)kHoldCounters) * kHoldCounterStride,
              (unsigned long long)done);
}

}  // namespace midv
