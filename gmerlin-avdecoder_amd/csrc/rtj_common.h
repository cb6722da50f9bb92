// rtj_common.h — structures shared by the host side and the gfx950 kernels.
#pragma once
#include <stdint.h>

namespace mirtj {

// One quality's tables as the device sees them (built on the host, rtj_tables.cpp).
// Natural (row-major) order like RTjpeg_t's liqt/ciqt/lqt/cqt (include/RTjpeg.h:40-58).
struct QTab {
  int32_t liqt[64];
  int32_t ciqt[64];
  int32_t lqt[64];
  int32_t cqt[64];
  int32_t lb8;
  int32_t cb8;
  int32_t pad[2];
};
static_assert(sizeof(QTab) == 1040, "QTab layout");

// Index 0 = the all-zero tables of a decoder that never saw a non-zero quality
// (RTjpeg_init bzero's the struct, lib/RTjpeg.c:2495-2502); 1..255 = RTjpeg_set_quality(Q).
constexpr int kNumQTab = 256;

// One packet of a plan, device view.
struct FrameDev {
  uint64_t data_off;  // offset of the first data byte (packet offset + 12) in the stream buffer
  uint64_t out_off;   // offset of the Y plane in the output buffer; U and V follow
  uint32_t data_len;  // bytes after the header; reads at or past it return 0
  uint32_t w, h;      // positive multiples of 16
  uint32_t qidx;      // row of the QTab LUT
  uint32_t blk_base;  // first entry of this frame in the block-offset index (nblk+1 entries)
  uint32_t nmb;       // macroblocks = (w/16)*(h/16)
  uint32_t mbw;       // macroblocks per row
  uint32_t nchunks;   // stream chunks of kChunk bytes covering data_len (at least 1)
  uint32_t chunk_base;  // first entry of this frame in the per-chunk arrays (nchunks+1 entries)
  uint32_t sum_base;    // first chunk of this frame in the summary array (nchunks rows of kEntries)
  uint32_t pad[2];
};
static_assert(sizeof(FrameDev) == 64, "FrameDev layout");

// Parallel block-offset index: the stream of a packet is cut into chunks of kChunk bytes.  A
// macroblock is at most 6*64 bytes, so the first macroblock that starts inside a chunk starts at
// one of kEntries offsets; a chunk's summary maps each of them to (exit offset, macroblock count).
constexpr int kChunk = 3584;
constexpr int kEntries = 384;
constexpr int kTabN = kChunk + kEntries;  // positions that get block-length tables
constexpr int kStageN = 4096;             // bytes staged per chunk (kTabN + 64 rounded up)

constexpr int kMbPerGroup = 32;  // macroblocks per decode workgroup (3 waves: Ytop, Ybottom, chroma)

// The three arms of RTjpeg_compress / RTjpeg_decompress (lib/RTjpeg.c:3488-3524, 3580-3585), numbered as MI_RTJ_FMT_*.
// FmtShape is the one statement of a format's geometry: the kernels that are templates on the format read it, and the
// host's table of formats (mi_rtjpeg.hip) is generated from it.
//   4:2:0  macroblock 16x16: Y Y Y Y Cb Cr, chroma planes w/2 x h/2
//   4:2:2  macroblock 16x8:  Y Y Cb Cr,     chroma planes w/2 x h
//   grey   "macroblock" = one 8x8 block, raster order, one plane
// A group is what one workgroup (decode) or `kParts` workgroups (encode) cover; a part is 64 blocks, one per lane:
// a row of 64 luma blocks, or 32 Cb + 32 Cr blocks.
enum { kFmtYUV420 = 0, kFmtYUV422 = 1, kFmtGrey = 2 };

template <int Fmt>
struct FmtShape;
template <>
struct FmtShape<kFmtYUV420> {
  static constexpr uint32_t kMbW = 16, kMbH = 16;  // pixels
  static constexpr uint32_t kBlkPerMb = 6;
  static constexpr uint32_t kParts = 3;  // upper luma row | lower luma row | chroma
  static constexpr uint32_t kUnitsPerGroup = (uint32_t)kMbPerGroup;
  static constexpr uint32_t kChromaPlanes = 2, kChromaShiftX = 1, kChromaShiftY = 1;
};
template <>
struct FmtShape<kFmtYUV422> {
  static constexpr uint32_t kMbW = 16, kMbH = 8;
  static constexpr uint32_t kBlkPerMb = 4;
  static constexpr uint32_t kParts = 2;  // luma row | chroma
  static constexpr uint32_t kUnitsPerGroup = (uint32_t)kMbPerGroup;
  static constexpr uint32_t kChromaPlanes = 2, kChromaShiftX = 1, kChromaShiftY = 0;
};
template <>
struct FmtShape<kFmtGrey> {
  static constexpr uint32_t kMbW = 8, kMbH = 8;
  static constexpr uint32_t kBlkPerMb = 1;
  static constexpr uint32_t kParts = 1;
  static constexpr uint32_t kUnitsPerGroup = 64;
  static constexpr uint32_t kChromaPlanes = 0, kChromaShiftX = 0, kChromaShiftY = 0;
};

#if defined(__HIP__) || defined(__HIPCC__)
#define MIRTJ_HD __attribute__((host, device, always_inline)) inline
#else
#define MIRTJ_HD inline
#endif

// Where block `k` (stream order: the luma blocks row by row, then Cb, then Cr) of unit `unit` of a w x h picture with
// `upr` units per row lies: the byte offset of its first row relative to the Y plane (Y, then Cb, then Cr, each plane
// packed) and the stride of its rows.  The one statement of this arithmetic for the kernels that are templates on the
// format.
struct BlockOrigin {
  uint64_t off;
  uint32_t stride;
};
template <int Fmt>
MIRTJ_HD BlockOrigin block_origin(uint32_t unit, uint32_t k, uint32_t w, uint32_t h, uint32_t upr) {
  using S = FmtShape<Fmt>;
  constexpr uint32_t kLuma = S::kBlkPerMb - S::kChromaPlanes, kPerRow = S::kMbW / 8u;
  const uint32_t ux = unit % upr, uy = unit / upr;
  if (S::kChromaPlanes == 0u || k < kLuma) {
    const uint32_t row = S::kMbH == 8u ? 0u : k / kPerRow, col = k - row * kPerRow;
    return {(uint64_t)(uy * S::kMbH + row * 8u) * w + ux * S::kMbW + col * 8u, w};
  }
  const uint32_t stride = w >> S::kChromaShiftX;
  const uint64_t ysz = (uint64_t)w * h;
  return {ysz + (k == S::kBlkPerMb - 1u ? ysz >> (S::kChromaShiftX + S::kChromaShiftY) : 0ull) +
              (uint64_t)(uy * (S::kMbH >> S::kChromaShiftY)) * stride + ux * (S::kMbW >> S::kChromaShiftX),
          stride};
}

// zig-zag order of the bitstream, transposed relative to JPEG (lib/RTjpeg.c:59-74)
#define MIRTJ_ZZ_INIT                                                                        \
  {0,  8,  1,  2,  9,  16, 24, 17, 10, 3,  4,  11, 18, 25, 32, 40, 33, 26, 19, 12, 5,  6,   \
   13, 20, 27, 34, 41, 48, 56, 49, 42, 35, 28, 21, 14, 7,  15, 22, 29, 36, 43, 50, 57, 58,  \
   51, 44, 37, 30, 23, 31, 38, 45, 52, 59, 60, 53, 46, 39, 47, 54, 61, 62, 55, 63}

}  // namespace mirtj
