// rtj_runs_kernels.h — phase 2 of a plan with runs (mi_rtj_plan_set_runs): unchanged blocks of a stream (gfx950).
//
// A run is a stretch of consecutive packets of a plan that are consecutive pictures of one stream.  Phase 1 (the index
// kernels and the transform) writes every coded block of every picture and leaves unchanged (0xFF) blocks alone.  In
// the reference an unchanged block keeps what the stream's one frame holds (lib/RTjpeg.c:2704, lib/video_rtjpeg.c:81):
// block b of picture k > 0 of a run is block b of the nearest earlier picture j < k of the run in which b is coded, or
// of picture 0's slot if there is none (picture 0's slot holds the stream's previous picture, prefilled by the caller).
//
// Classification comes from the block-offset index of the launch, not from the packet bytes: a block of index length 1
// is the byte 0xFF, a coded block is at least 2 bytes (RTjpeg_s2b reads the DC byte and at least one more,
// lib/RTjpeg.c:157-186).  The source picture is resolved with a segmented "last coded" scan over chunks of kRunChunk
// pictures; kernel boundaries are the only ordering between its passes:
//
//   k_runs_mask    per (chunk, block): 64-bit mask of the chunk's pictures in which the block is coded
//   k_runs_carry   per (run, block), serially over the run's chunks only: the source a chunk's first picture inherits
//                  (the last picture of an earlier chunk that codes the block, else picture 0); zeroes the copy count
//   k_runs_copy    per (kRunSub pictures of a chunk, tile of 32 macroblocks): resolves every unchanged block from the
//                  mask and the carry and copies its 8 rows of 8 bytes from the source picture
//
// Copies write unchanged blocks of pictures k > 0 only, and read coded blocks or picture 0's slot, which phase 1 has
// finished and phase 2 never writes: one copy pass needs no ordering among its own workgroups.
//
// k_runs_mask_fmt / k_runs_carry_fmt / k_runs_copy_fmt<Fmt> at the end of the file are the same passes for 4:2:2 and
// greyscale plans (mi_rtj_plan_set_runs_fmt), with FmtShape<Fmt>'s geometry.
#pragma once
#include <hip/hip_runtime.h>

#include "rtj_common.h"

namespace mirtj {

constexpr int kRunChunk = 64;                      // pictures per scan chunk (one bit each in a 64-bit mask)
constexpr int kRunSub = 8;                         // pictures per copy workgroup
constexpr int kRunSubs = kRunChunk / kRunSub;      // copy workgroups per chunk and tile
constexpr int kRunTileMb = 32;                     // macroblocks per copy workgroup
constexpr int kRunCopyThreads = 6 * kRunTileMb;    // one lane per block of the tile: three waves
constexpr int kRunScanThreads = 256;
constexpr uint32_t kRunMaxGridY = 65535u;          // the kernels loop over their work items past this

// One chunk of a run (device view).  Rows of the mask / carry arrays are [chunk][blocks per macroblock * nmb]
// (4:2:0: 6; the other formats: FmtShape::kBlkPerMb, below).
struct RunChunkDev {
  uint32_t frame0;  // plan index of the run's picture 0
  uint32_t rel0;    // run-relative index of the chunk's first picture
  uint32_t count;   // pictures in the chunk, 1..kRunChunk
  uint32_t nmb;     // macroblocks per picture (the run's pictures share their coded size)
  uint64_t row;     // first entry of the chunk in the mask / carry arrays
  uint32_t pad[2];
};
static_assert(sizeof(RunChunkDev) == 32, "RunChunkDev layout");

// One run of two or more pictures (runs of one picture need no phase 2).
struct RunDev {
  uint32_t chunk0;   // its first chunk in the chunk array
  uint32_t nchunks;
  uint32_t nmb;
  uint32_t pad;
};
static_assert(sizeof(RunDev) == 16, "RunDev layout");

// grid (ceil(6 * max nmb / 256), min(chunks, 65535)), 256 threads: one lane per block of a chunk.  The reads of a
// picture's index entries are consecutive across the lanes; the picture's index base is uniform.
__global__ __launch_bounds__(kRunScanThreads) void k_runs_mask(const FrameDev* __restrict__ frames,
                                                               const RunChunkDev* __restrict__ chunks, uint32_t nchunks,
                                                               const uint32_t* __restrict__ blkoff,
                                                               uint64_t* __restrict__ mask) {
  const uint32_t b = blockIdx.x * kRunScanThreads + threadIdx.x;
  for (uint32_t c = blockIdx.y; c < nchunks; c += gridDim.y) {
    const RunChunkDev ch = chunks[c];
    if (b >= 6u * ch.nmb) continue;
    const FrameDev* const f = frames + ch.frame0 + ch.rel0;
    uint64_t m = 0;
    for (uint32_t j = 0; j < ch.count; j++) {
      const uint32_t* const ix = blkoff + f[j].blk_base + b;
      m |= (uint64_t)(ix[1] - ix[0] != 1u) << j;
    }
    mask[ch.row + b] = m;
  }
}

// grid (ceil(6 * max nmb / 256), min(runs, 65535)), 256 threads: one lane per block of a run walks the run's chunks.
__global__ __launch_bounds__(kRunScanThreads) void k_runs_carry(const RunDev* __restrict__ runs, uint32_t nruns,
                                                                const RunChunkDev* __restrict__ chunks,
                                                                const uint64_t* __restrict__ mask,
                                                                uint16_t* __restrict__ carry,
                                                                unsigned long long* __restrict__ copied) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *copied = 0ull;  // k_runs_copy of this launch counts
  const uint32_t b = blockIdx.x * kRunScanThreads + threadIdx.x;
  for (uint32_t r = blockIdx.y; r < nruns; r += gridDim.y) {
    const RunDev run = runs[r];
    if (b >= 6u * run.nmb) continue;
    uint32_t src = 0;  // picture 0 of the run
#pragma unroll 4
    for (uint32_t c = 0; c < run.nchunks; c++) {
      const RunChunkDev& ch = chunks[run.chunk0 + c];
      const uint64_t m = mask[ch.row + b];
      carry[ch.row + b] = (uint16_t)src;
      if (m) src = ch.rel0 + 63u - (uint32_t)__builtin_clzll(m);
    }
  }
}

// grid (ceil(max nmb / 32), min(chunks * kRunSubs, 65535)), 192 threads.  Lanes lie along block rows: wave 0 takes the
// top luma blocks of the tile's 32 macroblocks (Y0 Y1 of each: 256 consecutive bytes of a row when the tile lies in one
// macroblock row), wave 1 the bottom ones, wave 2 the U blocks then the V blocks, so that the 8-byte row stores of a
// wave coalesce.
__global__ __launch_bounds__(kRunCopyThreads) void k_runs_copy(const FrameDev* __restrict__ frames,
                                                               const RunChunkDev* __restrict__ chunks, uint32_t nitems,
                                                               const uint64_t* __restrict__ mask,
                                                               const uint16_t* __restrict__ carry,
                                                               uint8_t* __restrict__ out,
                                                               unsigned long long* __restrict__ copied) {
  const uint32_t t = threadIdx.x;
  const uint32_t mbl = t < 128u ? (t & 63u) >> 1 : (t - 128u) & 31u;
  const uint32_t k = t < 64u ? (t & 1u) : t < 128u ? 2u + (t & 1u) : 4u + ((t - 128u) >> 5);
  const uint32_t mb = blockIdx.x * kRunTileMb + mbl;
  uint32_t done = 0;
  for (uint32_t it = blockIdx.y; it < nitems; it += gridDim.y) {
    const RunChunkDev ch = chunks[it / kRunSubs];
    const uint32_t j0 = (it % kRunSubs) * kRunSub;
    if (j0 >= ch.count || mb >= ch.nmb) continue;
    const uint32_t b = 6u * mb + k;
    const uint64_t m = mask[ch.row + b];
    const uint32_t cin = carry[ch.row + b];
    const FrameDev* const run = frames + ch.frame0;
    const uint32_t w = run->w, h = run->h, mbw = run->mbw;
    const uint32_t mbx = mb % mbw, mby = mb / mbw;
    uint32_t stride;
    uint64_t off;  // the block's first byte relative to its picture's Y plane (Y, then U, then V, stride = width)
    if (k < 4u) {
      stride = w;
      off = (uint64_t)(mby * 16u + (k >> 1) * 8u) * w + mbx * 16u + (k & 1u) * 8u;
    } else {
      stride = w >> 1;
      off = (uint64_t)w * h + (k == 5u ? (uint64_t)w * h / 4u : 0ull) + (uint64_t)(mby * 8u) * stride + mbx * 8u;
    }
    const uint32_t jn = min(ch.count, j0 + (uint32_t)kRunSub);
    for (uint32_t j = j0; j < jn; j++) {
      const uint32_t rel = ch.rel0 + j;
      if (rel == 0u || ((m >> j) & 1ull)) continue;  // picture 0 keeps its slot; coded blocks were written by phase 1
      const uint64_t below = m & ((1ull << j) - 1ull);
      const uint32_t src = below ? ch.rel0 + 63u - (uint32_t)__builtin_clzll(below) : cin;
      const uint8_t* s = out + run[src].out_off + off;
      uint8_t* d = out + run[rel].out_off + off;
      uint2 v[8];
#pragma unroll
      for (int r = 0; r < 8; r++) v[r] = *(const uint2*)(s + (uint64_t)r * stride);
#pragma unroll
      for (int r = 0; r < 8; r++) *(uint2*)(d + (uint64_t)r * stride) = v[r];
      done++;
    }
  }
  // one atomic per wave
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) done += __shfl_xor(done, o);
  if ((t & 63u) == 0u && done) atomicAdd(copied, (unsigned long long)done);
}

// ---------------------------------------------------------------------------------------
// The same three passes for 4:2:2 and greyscale plans (mi_rtj_plan_set_runs_fmt).  The geometry is FmtShape<Fmt>'s
// (rtj_common.h): FmtShape::kBlkPerMb blocks per unit (a 16x8 macroblock: Y Y Cb Cr; greyscale: one block, raster
// order), rows of the mask / carry arrays are [chunk][kBlkPerMb * nmb].  The 4:2:0 kernels above stay as they are.
// ---------------------------------------------------------------------------------------

// The copy workgroup of a format: one lane per block of a tile of consecutive units, laid along block rows as
// k_decode_fmt lays its groups (rtj_format_kernels.h), so that a wave's 8-byte row loads and stores cover whole line
// segments.
//   4:2:2  32 macroblocks, 128 lanes: wave 0 the 64 luma blocks (lane l: block l & 1 of macroblock l >> 1, 512
//          consecutive bytes of a row where the tile lies in one macroblock row), wave 1 the 32 Cb then the 32 Cr blocks
//          (2 x 256 bytes; chroma stride w / 2, chroma plane height h)
//   grey   64 blocks in raster order, one wave: 512 bytes of a row
// A lane divides its unit number by the units per row, so a tile that wraps one or several picture rows, or the partial
// last tile, is no special case.
template <int Fmt>
struct RunTile {
  static constexpr uint32_t kUnits = FmtShape<Fmt>::kBlkPerMb == 1u ? 64u : (uint32_t)kRunTileMb;
  static constexpr uint32_t kThreads = kUnits * FmtShape<Fmt>::kBlkPerMb;
};
static_assert(RunTile<kFmtYUV422>::kThreads == 128u && RunTile<kFmtGrey>::kThreads == 64u, "whole waves");

// grid (ceil(kBlkPerMb * max nmb / 256), min(chunks, 65535)), 256 threads: k_runs_mask with the format's blocks per unit.
// (A body shared with k_runs_mask / k_runs_carry through an inlined template was tried: the 4:2:0 kernels then compile to
// other instruction text, so the scans are written out.)
template <int Fmt>
__global__ __launch_bounds__(kRunScanThreads) void k_runs_mask_fmt(const FrameDev* __restrict__ frames,
                                                                   const RunChunkDev* __restrict__ chunks,
                                                                   uint32_t nchunks, const uint32_t* __restrict__ blkoff,
                                                                   uint64_t* __restrict__ mask) {
  const uint32_t b = blockIdx.x * kRunScanThreads + threadIdx.x;
  for (uint32_t c = blockIdx.y; c < nchunks; c += gridDim.y) {
    const RunChunkDev ch = chunks[c];
    if (b >= FmtShape<Fmt>::kBlkPerMb * ch.nmb) continue;
    const FrameDev* const f = frames + ch.frame0 + ch.rel0;
    uint64_t m = 0;
    for (uint32_t j = 0; j < ch.count; j++) {
      const uint32_t* const ix = blkoff + f[j].blk_base + b;
      m |= (uint64_t)(ix[1] - ix[0] != 1u) << j;
    }
    mask[ch.row + b] = m;
  }
}

// grid (ceil(kBlkPerMb * max nmb / 256), min(runs, 65535)), 256 threads: k_runs_carry with the format's blocks per unit.
template <int Fmt>
__global__ __launch_bounds__(kRunScanThreads) void k_runs_carry_fmt(const RunDev* __restrict__ runs, uint32_t nruns,
                                                                    const RunChunkDev* __restrict__ chunks,
                                                                    const uint64_t* __restrict__ mask,
                                                                    uint16_t* __restrict__ carry,
                                                                    unsigned long long* __restrict__ copied) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *copied = 0ull;  // k_runs_copy_fmt of this launch counts
  const uint32_t b = blockIdx.x * kRunScanThreads + threadIdx.x;
  for (uint32_t r = blockIdx.y; r < nruns; r += gridDim.y) {
    const RunDev run = runs[r];
    if (b >= FmtShape<Fmt>::kBlkPerMb * run.nmb) continue;
    uint32_t src = 0;  // picture 0 of the run
#pragma unroll 4
    for (uint32_t c = 0; c < run.nchunks; c++) {
      const RunChunkDev& ch = chunks[run.chunk0 + c];
      const uint64_t m = mask[ch.row + b];
      carry[ch.row + b] = (uint16_t)src;
      if (m) src = ch.rel0 + 63u - (uint32_t)__builtin_clzll(m);
    }
  }
}

// grid (ceil(max nmb / RunTile::kUnits), min(chunks * kRunSubs, 65535)), RunTile::kThreads threads.
template <int Fmt>
__global__ __launch_bounds__(RunTile<Fmt>::kThreads) void k_runs_copy_fmt(const FrameDev* __restrict__ frames,
                                                                          const RunChunkDev* __restrict__ chunks,
                                                                          uint32_t nitems,
                                                                          const uint64_t* __restrict__ mask,
                                                                          const uint16_t* __restrict__ carry,
                                                                          uint8_t* __restrict__ out,
                                                                          unsigned long long* __restrict__ copied) {
  using S = FmtShape<Fmt>;
  const uint32_t t = threadIdx.x;
  uint32_t ul, k;  // the lane's unit of the tile and its block of the unit
  if (Fmt == kFmtYUV422) {
    ul = t < 64u ? t >> 1 : (t - 64u) & 31u;
    k = t < 64u ? (t & 1u) : 2u + ((t - 64u) >> 5);
  } else {
    ul = t;
    k = 0u;
  }
  const uint32_t unit = blockIdx.x * RunTile<Fmt>::kUnits + ul;
  uint32_t done = 0;
  for (uint32_t it = blockIdx.y; it < nitems; it += gridDim.y) {
    const RunChunkDev ch = chunks[it / kRunSubs];
    const uint32_t j0 = (it % kRunSubs) * kRunSub;
    if (j0 >= ch.count || unit >= ch.nmb) continue;
    const uint32_t b = S::kBlkPerMb * unit + k;
    const uint64_t m = mask[ch.row + b];
    const uint32_t cin = carry[ch.row + b];
    const FrameDev* const run = frames + ch.frame0;
    const uint32_t w = run->w, h = run->h, mbw = run->mbw;
    const uint32_t ux = unit % mbw, uy = unit / mbw;
    uint32_t stride;
    uint64_t off;  // the block's first byte relative to its picture's Y plane (Y, then Cb, then Cr)
    if (Fmt == kFmtYUV422 && k >= 2u) {
      stride = w >> 1;
      off = (uint64_t)w * h + (k == 3u ? (uint64_t)w * h / 2u : 0ull) + (uint64_t)(uy * 8u) * stride + ux * 8u;
    } else {
      stride = w;
      off = (uint64_t)(uy * 8u) * w + ux * S::kMbW + k * 8u;
    }
    const uint32_t jn = min(ch.count, j0 + (uint32_t)kRunSub);
    for (uint32_t j = j0; j < jn; j++) {
      const uint32_t rel = ch.rel0 + j;
      if (rel == 0u || ((m >> j) & 1ull)) continue;  // picture 0 keeps its slot; coded blocks were written by phase 1
      const uint64_t below = m & ((1ull << j) - 1ull);
      const uint32_t src = below ? ch.rel0 + 63u - (uint32_t)__builtin_clzll(below) : cin;
      const uint8_t* s = out + run[src].out_off + off;
      uint8_t* d = out + run[rel].out_off + off;
      uint2 v[8];
#pragma unroll
      for (int r = 0; r < 8; r++) v[r] = *(const uint2*)(s + (uint64_t)r * stride);
#pragma unroll
      for (int r = 0; r < 8; r++) *(uint2*)(d + (uint64_t)r * stride) = v[r];
      done++;
    }
  }
  // one atomic per wave
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) done += __shfl_xor(done, o);
  if ((t & 63u) == 0u && done) atomicAdd(copied, (unsigned long long)done);
}

}  // namespace mirtj
