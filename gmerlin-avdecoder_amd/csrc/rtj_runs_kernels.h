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
//   k_runs_copy    per (kRunSub pictures of a chunk, tile of RunTile<Fmt>::kUnits units): resolves every unchanged block from the
//                  mask and the carry and copies its 8 rows of 8 bytes from the source picture
//
// Copies write unchanged blocks of pictures k > 0 only, and read coded blocks or picture 0's slot, which phase 1 has
// finished and phase 2 never writes: one copy pass needs no ordering among its own workgroups.
//
// The three kernels are templates on the picture format (mi_rtj_plan_set_runs: 4:2:0; mi_rtj_plan_set_runs_fmt: all
// three) and read its geometry from FmtShape<Fmt> (rtj_common.h): kBlkPerMb blocks per unit (4:2:0: a 16x16 macroblock,
// Y Y Y Y Cb Cr; 4:2:2: a 16x8 macroblock, Y Y Cb Cr; greyscale: one block, raster order).
#pragma once
#include <hip/hip_runtime.h>

#include "rtj_common.h"

namespace mirtj {

constexpr int kRunChunk = 64;                      // pictures per scan chunk (one bit each in a 64-bit mask)
constexpr int kRunSub = 8;                         // pictures per copy workgroup
constexpr int kRunSubs = kRunChunk / kRunSub;      // copy workgroups per chunk and tile
constexpr int kRunScanThreads = 256;
constexpr uint32_t kRunMaxGridY = 65535u;          // the kernels loop over their work items past this

// One chunk of a run (device view).  Rows of the mask / carry arrays are [chunk][FmtShape::kBlkPerMb * nmb].
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

// The copy workgroup of a format: one lane per block of a tile of consecutive units, laid along block rows as the
// transform lays its groups, so that a wave's 8-byte row loads and stores cover whole line segments (the lane map is in
// k_runs_copy).  4:2:0 and 4:2:2: 32 macroblocks, 192 and 128 lanes; greyscale: 64 blocks, one wave.
template <int Fmt>
struct RunTile {
  static constexpr uint32_t kUnits = FmtShape<Fmt>::kBlkPerMb == 1u ? 64u : 32u;
  static constexpr uint32_t kThreads = kUnits * FmtShape<Fmt>::kBlkPerMb;
};
static_assert(RunTile<kFmtYUV420>::kThreads == 192u && RunTile<kFmtYUV422>::kThreads == 128u &&
                  RunTile<kFmtGrey>::kThreads == 64u,
              "whole waves");

// grid (ceil(kBlkPerMb * max nmb / 256), min(chunks, 65535)), 256 threads: one lane per block of a chunk.  The reads of
// a picture's index entries are consecutive across the lanes; the picture's index base is uniform.
// (One body for the three formats costs 4:2:0 nothing: k_runs_mask<kFmtYUV420> and k_runs_carry<kFmtYUV420> compile to
// the instructions the kernels written out for 4:2:0 had.  An earlier note here said otherwise; the hash it went by
// covered the kernel's mangled name.  DESIGN.md section 11.2.)
template <int Fmt>
__global__ __launch_bounds__(kRunScanThreads) void k_runs_mask(const FrameDev* __restrict__ frames,
                                                               const RunChunkDev* __restrict__ chunks, uint32_t nchunks,
                                                               const uint32_t* __restrict__ blkoff,
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

// grid (ceil(kBlkPerMb * max nmb / 256), min(runs, 65535)), 256 threads: one lane per block of a run walks the run's
// chunks.
template <int Fmt>
__global__ __launch_bounds__(kRunScanThreads) void k_runs_carry(const RunDev* __restrict__ runs, uint32_t nruns,
                                                                const RunChunkDev* __restrict__ chunks,
                                                                const uint64_t* __restrict__ mask,
                                                                uint16_t* __restrict__ carry,
                                                                unsigned long long* __restrict__ copied) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *copied = 0ull;  // k_runs_copy of this launch counts
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

// grid (ceil(max nmb / RunTile::kUnits), min(chunks * kRunSubs, 65535)), RunTile::kThreads threads.  The lane map from
// thread to (unit of the tile, block of the unit) is the only text per format; the block's place in the picture is
// block_origin's (rtj_common.h).  A lane divides its unit number by the units per row, so a tile that wraps one or
// several picture rows, or the partial last tile, is no special case.
template <int Fmt>
__global__ __launch_bounds__(RunTile<Fmt>::kThreads) void k_runs_copy(const FrameDev* __restrict__ frames,
                                                                      const RunChunkDev* __restrict__ chunks,
                                                                      uint32_t nitems, const uint64_t* __restrict__ mask,
                                                                      const uint16_t* __restrict__ carry,
                                                                      uint8_t* __restrict__ out,
                                                                      unsigned long long* __restrict__ copied) {
  using S = FmtShape<Fmt>;
  const uint32_t t = threadIdx.x;
  uint32_t ul, k;  // the lane's unit of the tile and its block of the unit
  if (Fmt == kFmtYUV420) {
    // wave 0 takes the top luma blocks of the tile's 32 macroblocks (Y0 Y1 of each: 256 consecutive bytes of a row when
    // the tile lies in one macroblock row), wave 1 the bottom ones, wave 2 the U blocks then the V blocks, so that the
    // 8-byte row stores of a wave coalesce
    ul = t < 128u ? (t & 63u) >> 1 : (t - 128u) & 31u;
    k = t < 64u ? (t & 1u) : t < 128u ? 2u + (t & 1u) : 4u + ((t - 128u) >> 5);
  } else if (Fmt == kFmtYUV422) {
    // wave 0 the 64 luma blocks (lane l: block l & 1 of macroblock l >> 1, 512 consecutive bytes of a row where the tile
    // lies in one macroblock row), wave 1 the 32 Cb then the 32 Cr blocks (2 x 256 bytes; chroma stride w / 2, chroma
    // plane height h)
    ul = t < 64u ? t >> 1 : (t - 64u) & 31u;
    k = t < 64u ? (t & 1u) : 2u + ((t - 64u) >> 5);
  } else {
    // 64 blocks in raster order, one wave: 512 bytes of a row
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
    const BlockOrigin at = block_origin<Fmt>(unit, k, run->w, run->h, run->mbw);
    const uint64_t off = at.off;
    const uint32_t stride = at.stride;
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
