// rtj_format_kernels.h — gfx950 kernels of the two other arms of RTjpeg_decompress (lib/RTjpeg.c:3580-3585):
//
//   RTjpeg_decompressYUV422 (lib/RTjpeg.c:2639-2686)  macroblock = 16x8 pixels: Y, Y, Cb, Cr; chroma planes w/2 x h
//   RTjpeg_decompress8      (lib/RTjpeg.c:2751-2772)  8x8 luma blocks in raster order, one plane
//
//   k_index_fmt<Fmt>    block-start index: walk_packet<Fmt> (rtj_walk_kernels.h), one wave per packet, packets side by
//                       side (grid-stride).
//   k_decode_fmt<Fmt>   dequantise + inverse transform + plane scatter, one lane per 8x8 block, one wave per part of a
//                       group.  The arithmetic is the 4:2:0 path's: the packed passes of rtj_idct_pk.h behind their
//                       per-block range test, the one-value-per-register passes of rtj_idct_asm.h as the fallback,
//                       transform_lo for waves whose blocks stay inside the low 4x4, px() for the clamp.
//
// The descriptors are the 4:2:0 path's (FrameDev), read per format:
//   4:2:2  mbw = w / 16, nmb = mbw * (h / 8), 4 blocks per macroblock
//   grey   mbw = w / 8,  nmb = mbw * (h / 8), 1 block per "macroblock"
// Nothing here is called by the 4:2:0 kernels and nothing of theirs is changed.
#pragma once
#include <hip/hip_runtime.h>

#include "rtj_common.h"
#include "rtj_decode_kernels.h"
#include "rtj_walk_kernels.h"

namespace mirtj {

// The packets of a plan, a wave each, side by side (grid-stride over the packets as in k_index_walk_todo).
template <int Fmt>
__global__ __launch_bounds__(64) void k_index_fmt(const FrameDev* __restrict__ frames, uint32_t nframes,
                                                   const uint8_t* __restrict__ stream, const QTab* __restrict__ lut,
                                                   uint32_t* __restrict__ blkoff) {
  for (uint32_t i = blockIdx.x; i < nframes; i += gridDim.x) {
    const FrameDev f = frames[i];
    walk_packet<Fmt>(f, stream, lut, blkoff + f.blk_base);
  }
}

// ---------------------------------------------------------------------------------------
// k_decode_fmt<Fmt>: grid (parts * groups, frames), one wave per workgroup and part of a group.
//   4:2:2  group = kMbPerGroup consecutive macroblocks.  part 0: their 64 luma blocks — lane l has block l & 1 of
//          macroblock l >> 1, so the wave's row stores cover 512 contiguous pixels of one 8-line row (or two or more
//          stretches where the group wraps a picture row); part 1: lanes 0-31 the Cb blocks, lanes 32-63 the Cr blocks:
//          2 x 256 contiguous bytes.
//   grey   group = 64 consecutive blocks in raster order: 512 contiguous pixels.
// Lanes past the picture's last block have nothing to do (the partial last group).
// A lane reads its block's bytes 16 at a time through a buffer descriptor that returns 0 at or past the packet's end
// (RTjpeg_s2b's length rule, lib/RTjpeg.c:157-186: at most 64 bytes, four rounds), dequantises into its LDS scratch in
// the column-pair layout of coef_byte(), and runs the transform in registers.  A block whose first byte is 0xFF leaves
// its 8x8 destination as it was (lib/RTjpeg.c:2654, 2764).
// ---------------------------------------------------------------------------------------
constexpr int kFmtLdsWords = kCoefWords + 64;  // the lanes' coefficient scratch, then the part's slot table

template <int Fmt>
__global__ __launch_bounds__(kDecThreads) void k_decode_fmt(const FrameDev* __restrict__ frames,
                                                            const uint8_t* __restrict__ stream,
                                                            const QTab* __restrict__ lut,
                                                            const uint32_t* __restrict__ blkoff,
                                                            uint8_t* __restrict__ outbuf) {
  using S = FmtShape<Fmt>;
  __shared__ __attribute__((aligned(16))) uint32_t s_lds[kFmtLdsWords];
  uint32_t* s_tab = s_lds + kCoefWords;
  const FrameDev f = frames[blockIdx.y];
  const uint32_t grp = blockIdx.x / S::kParts, part = blockIdx.x - grp * S::kParts;  // wave-uniform
  const uint32_t ngroups = (f.nmb + S::kUnitsPerGroup - 1u) / S::kUnitsPerGroup;
  if (grp >= ngroups) return;
  const uint32_t lane = threadIdx.x & 63u;
  const bool chroma = Fmt == kFmtYUV422 && part == 1u;
  const QTab& qt = lut[f.qidx];
  const uint32_t bt8 = (uint32_t)(chroma ? qt.cb8 : qt.lb8);
  {  // slot k of the zig-zag order: dequantiser << 16 | byte offset in the lane's scratch
    const int nat = c_zz[lane];
    s_tab[lane] = ((uint32_t)(chroma ? qt.ciqt[nat] : qt.liqt[nat]) << 16) | (uint32_t)coef_byte(nat);
  }
  wave_lds_sync();

  // ---- which block this lane has and where its eight rows go ----
  uint32_t unit, kblk;  // macroblock (grey: block) of the picture, block of the macroblock
  if (Fmt == kFmtYUV422) {
    unit = grp * S::kUnitsPerGroup + (chroma ? (lane & 31u) : (lane >> 1));
    kblk = chroma ? 2u + (lane >> 5) : (lane & 1u);
  } else {
    unit = grp * S::kUnitsPerGroup + lane;
    kblk = 0u;
  }
  const bool valid = unit < f.nmb;
  const uint32_t uy = unit / f.mbw, ux = unit - uy * f.mbw;
  const size_t ysz = (size_t)f.w * f.h;
  uint32_t stride;
  size_t dst_off;
  if (Fmt == kFmtYUV422 && chroma) {
    stride = f.w >> 1;
    dst_off = ysz + (kblk == 3u ? ysz >> 1 : (size_t)0) + (size_t)(8u * uy) * stride + 8u * ux;
  } else if (Fmt == kFmtYUV422) {
    stride = f.w;
    dst_off = (size_t)(8u * uy) * stride + 16u * ux + 8u * kblk;
  } else {
    stride = f.w;
    dst_off = (size_t)(8u * uy) * stride + 8u * ux;
  }
  uint8_t* dst = outbuf + f.out_off + dst_off;

  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)(stream + f.data_off), 0, (int)f.data_len, 0x00020000);
  const uint32_t pos = valid ? blkoff[f.blk_base + S::kBlkPerMb * unit + kblk] : 0u;
  auto byte_at = [&](uint32_t p) -> uint32_t { return (uint32_t)__builtin_amdgcn_raw_buffer_load_b8(rs, (int)p, 0, 0); };

  const uint32_t my_a = lds_address(s_lds) + lane * (uint32_t)(kCoefStride * 2);
  const uint4* my = (const uint4*)((const uint8_t*)s_lds + (size_t)lane * (kCoefStride * 2));
  const uint32_t tab_a = lds_address(s_tab);

  uint32_t bytes[16];
#pragma unroll
  for (int i = 0; i < 16; i++) bytes[i] = byte_at(pos + (uint32_t)i);
  const bool live = valid && bytes[0] != 0xFFu;

  if (live) {
    {
      uint4* z = (uint4*)my;
#pragma unroll
      for (int i = 0; i < 8; i++) z[i] = make_uint4(0, 0, 0, 0);
    }
    // ---- stream -> dequantised coefficients, int16 (lib/RTjpeg.c:157-186): slot 0 is the unsigned DC, slots 1..bt8
    // signed raw bytes, then tokens: 64..127 a run of token - 63 zero slots, anything else one coefficient ----
    uint32_t co = 0;
    for (int round = 0; round < 4; round++) {  // 64 bytes: the longest block
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const uint32_t ub = bytes[i];
        const int sb = (int)(int8_t)ub;
        if (co < 64u) {
          if (co <= bt8 || sb <= 63) {
            const uint32_t e = *(const lds_u32_t*)(uintptr_t)(tab_a + 4u * co);
            const int v = co == 0u ? (int)ub : sb;
            *(lds_i16_t*)(uintptr_t)(my_a + (e & 0xFFFFu)) = (int16_t)mul24(v, (int)(e >> 16));  // |v| < 2^8, dequantiser < 2^14
            co += 1u;
          } else {
            co += (uint32_t)(sb - 63);  // the scratch is zero already
          }
        }
      }
      if (co >= 64u || round == 3) break;
#pragma unroll
      for (int i = 0; i < 16; i++) bytes[i] = byte_at(pos + 16u * (uint32_t)(round + 1) + (uint32_t)i);
    }
  }

  wave_lds_sync();  // the coefficient stores (int16) before the reads of whole column pairs below

  // ---- does any block of the wave reach outside the low 4x4? ----
  uint32_t hi = 0;
  if (live) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      if (i == 0 || i == 2) continue;  // rows 0-3 of columns 0-3
      const uint4 q = my[i];
      hi |= q.x | q.y | q.z | q.w;
    }
  }
  const bool lo = !__any(hi != 0u);

  if (live) {
    auto put_packed = [&](uint2 o) {  // one row of the block, already clamped and packed
      typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
      u32x2_t ov;
      ov.x = o.x;
      ov.y = o.y;
      __builtin_nontemporal_store(ov, (u32x2_t*)dst);
      dst += stride;
    };
    const IdctK K{362, 473, -669, 277, 128, 235};
    const IdctPK KP = idct_pk_constants();
    if (lo) {
      transform_lo(my, K, KP, put_packed);
    } else {
      transform_full<true>(my, s_lds, (int)lane, K, KP, put_packed);
    }
  }
}

}  // namespace mirtj
