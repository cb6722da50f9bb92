// rtj_encode_fmt_kernels.h — gfx950 kernel of the two other arms of RTjpeg_compress (lib/RTjpeg.c:3488-3524):
//
//   RTjpeg_compressYUV422 / RTjpeg_mcompressYUV422 (lib/RTjpeg.c:2565-2608, 2924-2988)
//                           macroblock = 16x8 pixels: Y, Y (luma tables, lb8), Cb, Cr (chroma tables, cb8, stride w/2)
//   RTjpeg_compress8 / RTjpeg_mcompress8           (lib/RTjpeg.c:2610-2637, 2990-3018)
//                           8x8 luma blocks in raster order, one plane
//
//   k_encode_fmt<Fmt, kInter>   forward transform + quantiser + run-length pack, one lane per 8x8 block, one wave per part
//                               of a group: the lane arrangement of k_decode_fmt (rtj_format_kernels.h), the body of
//                               k_encode_wave (rtj_encode_kernels.h).  kInter adds RTjpeg_bcomp (lib/RTjpeg.c:2827-2838).
//
// Greyscale codes the picture it is given: block (row r, column c) is lines 8r .. 8r+7, pixels 8c .. 8c+7, line stride
// w — the picture RTjpeg_decompress8 puts back.  The reference's greyscale arms do not: they hand RTjpeg_dctY the width
// where the other arms hand it width / 8 (lib/RTjpeg.c:2626, 3004; RTjpeg_dctY advances by rskip << 3, :341), so a block is
// read with a line stride of 8 w, and the intra arm moves on by ONE line per block row (:2630).  Everything else of a
// greyscale block's coding is the 4:2:2 luma block's, which is held to the reference.
//
// k_encode_scan, k_encode_place and k_encode_pack (rtj_encode_kernels.h) only know a block count and serve every format.
// Nothing here is called by the 4:2:0 kernels and nothing of theirs is changed.
#pragma once
#include <hip/hip_runtime.h>

#include "rtj_common.h"
#include "rtj_encode_kernels.h"  // fdct8, kEncSlotStride
#include "rtj_format_kernels.h"  // FmtShape

namespace mirtj {

// Rows -> quantised coefficients in natural order (lib/RTjpeg.c:288-389 dctY, :245-252 quant): eight 8-byte row loads
// (aligned: a block starts at a multiple of 8 pixels of a line whose stride is a multiple of 8), both passes and the
// quantiser in registers, every index a compile-time constant.
__device__ __forceinline__ void encode_fmt_transform(const uint8_t* __restrict__ src, uint32_t stride,
                                                     const int32_t* __restrict__ q, int (&blk)[64]) {
  int ws[64];
#pragma unroll
  for (int row = 0; row < 8; row++) {
    const uint2 d = *(const uint2*)(src + (size_t)row * stride);
    int p[8] = {(int)(d.x & 255u), (int)((d.x >> 8) & 255u), (int)((d.x >> 16) & 255u), (int)(d.x >> 24),
                (int)(d.y & 255u), (int)((d.y >> 8) & 255u), (int)((d.y >> 16) & 255u), (int)(d.y >> 24)};
    int r[8];
    fdct8(p, r);
    r[0] <<= 8;
    r[4] <<= 8;
#pragma unroll
    for (int c = 0; c < 8; c++) ws[8 * row + c] = r[c];
  }
#pragma unroll
  for (int c = 0; c < 8; c++) {
    int p[8], r[8];
#pragma unroll
    for (int kk = 0; kk < 8; kk++) p[kk] = ws[8 * kk + c];
    fdct8(p, r);
#pragma unroll
    for (int kk = 0; kk < 8; kk++) {
      const int16_t d = (kk == 0 || kk == 4) ? (int16_t)((r[kk] + 128) >> 8) : (int16_t)((r[kk] + 32768) >> 16);
      blk[8 * kk + c] = (int)(int16_t)(((int)d * q[8 * kk + c] + 32767) >> 16);  // RTjpeg_quant
    }
  }
}

// RTjpeg_b2s (lib/RTjpeg.c:109-155) into the lane's LDS slot: DC clamped to 0..254, bt8 full-range bytes, then 7-bit
// values and zero runs (63 + run); the zig-zag order fully unrolled, so that the coefficient of a slot is a register.
// Returns the block's length, 2..64.
__device__ __forceinline__ int encode_fmt_pack(const int (&blk)[64], int bt8, uint8_t* out) {
  constexpr uint8_t zz[64] = MIRTJ_ZZ_INIT;
  int n = 0, run = 0;
  {
    const int v = blk[zz[0]];
    out[n++] = (uint8_t)(v > 254 ? 254 : (v < 0 ? 0 : v));
  }
#pragma unroll
  for (int z = 1; z < 64; z++) {
    const int v = blk[zz[z]];
    if (z <= kMaxRawBytes && z <= bt8) {  // (bt8 <= kMaxRawBytes: the host refuses other tables)
      out[n++] = (uint8_t)(int8_t)(v > 127 ? 127 : (v < -128 ? -128 : v));
    } else if (v != 0) {
      if (run) {
        out[n++] = (uint8_t)(63 + run);
        run = 0;
      }
      out[n++] = (uint8_t)(int8_t)(v > 63 ? 63 : (v < -64 ? -64 : v));
    } else {
      run++;
    }
  }
  if (run) out[n++] = (uint8_t)(63 + run);
  return n;
}

// grid (parts * groups, pictures), one wave per workgroup.
//   4:2:2  group = kMbPerGroup consecutive macroblocks.  part 0: their 64 luma blocks — lane l has block l & 1 of
//          macroblock l >> 1, so a row load of the wave covers 512 contiguous pixels (or two or more stretches where the
//          group wraps a picture row); part 1: lanes 0-31 the Cb blocks, lanes 32-63 the Cr blocks.
//   grey   group = 64 consecutive blocks in raster order.
// A lane divides its own macroblock (block) number by the count per picture row, so a group that wraps picture rows is
// no special case; lanes past the picture's last block return before their first load.  No barrier anywhere: a lane
// only touches its own LDS slot.
// Blocks are numbered in stream order across the pictures of the call: slot, length and (kInter) previous-block entry
// of block b of picture p are at p * nblk + b.
// kInter (one picture per launch, in stream order): `old` holds int16[64] per block, natural coefficient order.  A block
// whose 64 quantised coefficients all lie within the mask (lmask / cmask by block type) of its entry becomes the single
// byte 0xFF and leaves the entry alone; otherwise the entry takes the whole new block and the block is coded.
template <int Fmt, bool kInter>
__global__ __launch_bounds__(64) void k_encode_fmt(const uint8_t* __restrict__ frames, int w, int h,
                                                    const QTab* __restrict__ qt, uint8_t* __restrict__ slots,
                                                    uint8_t* __restrict__ lens, int16_t* __restrict__ old, int lmask,
                                                    int cmask) {
  using S = FmtShape<Fmt>;
  __shared__ __attribute__((aligned(16))) uint8_t s_slot[64 * kEncSlotStride];
  const uint32_t lane = threadIdx.x;
  const uint32_t mbw = Fmt == kFmtYUV422 ? (uint32_t)w / 16u : (uint32_t)w / 8u, nmb = mbw * ((uint32_t)h / 8u);
  const uint32_t grp = blockIdx.x / S::kParts, part = blockIdx.x - grp * S::kParts, fr = blockIdx.y;  // wave-uniform
  const bool chroma = Fmt == kFmtYUV422 && part == 1u;
  uint32_t unit, kblk;  // macroblock (grey: block) of the picture, block of the macroblock
  if (Fmt == kFmtYUV422) {
    unit = grp * S::kUnitsPerGroup + (chroma ? (lane & 31u) : (lane >> 1));
    kblk = chroma ? 2u + (lane >> 5) : (lane & 1u);
  } else {
    unit = grp * S::kUnitsPerGroup + lane;
    kblk = 0u;
  }
  if (unit >= nmb) return;
  const uint32_t uy = unit / mbw, ux = unit - uy * mbw;
  const size_t ysz = (size_t)w * h;
  const uint8_t* f = frames + (size_t)fr * (Fmt == kFmtYUV422 ? 2u * ysz : ysz);
  const uint8_t* src;
  uint32_t stride;
  if (Fmt == kFmtYUV422 && chroma) {
    stride = (uint32_t)w >> 1;
    src = f + ysz + (kblk == 3u ? ysz >> 1 : (size_t)0) + (size_t)(8u * uy) * stride + 8u * ux;
  } else if (Fmt == kFmtYUV422) {
    stride = (uint32_t)w;
    src = f + (size_t)(8u * uy) * stride + 16u * ux + 8u * kblk;
  } else {
    stride = (uint32_t)w;
    src = f + (size_t)(8u * uy) * stride + 8u * ux;
  }
  int blk[64];
  encode_fmt_transform(src, stride, chroma ? qt->cqt : qt->lqt, blk);
  const size_t gb = (size_t)fr * nmb * S::kBlkPerMb + S::kBlkPerMb * unit + kblk;
  if (kInter) {
    uint4* o4 = (uint4*)(old + gb * 64);  // 128 bytes per block: 16-byte aligned
    const int mask = chroma ? cmask : lmask;
    bool same = true;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint4 o = o4[i];
      const uint32_t wv[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int d0 = (int)(int16_t)(wv[j] & 0xFFFFu) - blk[8 * i + 2 * j];
        const int d1 = ((int)wv[j] >> 16) - blk[8 * i + 2 * j + 1];
        same = same && (d0 < 0 ? -d0 : d0) <= mask && (d1 < 0 ? -d1 : d1) <= mask;
      }
    }
    if (same) {
      slots[gb * 64] = 0xFF;
      lens[gb] = 1;
      return;
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
      auto pk = [&](int a) { return ((uint32_t)blk[a] & 0xFFFFu) | ((uint32_t)blk[a + 1] << 16); };
      o4[i] = make_uint4(pk(8 * i), pk(8 * i + 2), pk(8 * i + 4), pk(8 * i + 6));
    }
  }
  uint8_t* const out = s_slot + lane * kEncSlotStride;
  const int n = encode_fmt_pack(blk, chroma ? qt->cb8 : qt->lb8, out);  // (the tables are the same for all lanes of a part)
  lens[gb] = (uint8_t)n;
  const uint4* s4 = (const uint4*)out;
  uint4* g4 = (uint4*)(slots + gb * 64);
#pragma unroll
  for (int i = 0; i < 4; i++) g4[i] = s4[i];
}

}  // namespace mirtj
