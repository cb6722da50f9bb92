// dv_encode_kernels.h — gfx950 kernel of the DV video encoder, all five systems (the statement: tests/dvenc.py, which this
// reproduces bit for bit; the rules: DESIGN.md section 9.7; nothing in the reference to follow).
//
//   k_dv_encode<Sys>  one instantiation per system (dv_common.h).  Mirrors k_dv_decode: one wave per two video segments
//                  (2 x 5 macroblocks = 60 blocks, one lane each; a workgroup is one wave), pixels gathered through the
//                  system's place() and the block arrangement of the decoder's store section; areas 1 and 3 of the 4:2:2
//                  systems are coded as flat 128.  In order: forward transform in registers; the products |c| m into LDS
//                  in scan order; bit counts per block for a candidate quantisation number and a sum per segment, in a
//                  wave-uniform loop downwards from 15 that ends when both segments fit; the overflow rule at 0; code
//                  words into a per-lane bit buffer in LDS; the three passes with prefix sums over free bits and demands,
//                  poured into the segment's five DIF blocks in LDS; row stores of whole 80-byte DIF blocks.
//                  Workgroups behind the video ones write the non-video DIF blocks of one sequence each (ids with the
//                  channel bit, DSF, APT, VAUX stype, zeros elsewhere), so that one launch makes complete frames.
//
// Integer only; every multiplication's operands stay within 17 bits and its product within 29 (measured on the edge
// pictures of tests/dvenc_edges.py, whose 0 / 255 sign patterns drive every coefficient as far as pixels can; the 24-bit
// multiplier needs them below 2^23 and 2^31, which tests/test_dv_encode_edges_cpu.py asserts), so the 24-bit multiplier is
// exact.  Lane masks are 64 bits wide, and every loop carries a bound no picture can reach.
#pragma once
#include <hip/hip_runtime.h>

#include "dv_common.h"
#include "dv_decode_kernels.h"  // dv_wave_sync, dv_peek, dv_or_bits: the decoder's LDS bit buffers, the other way round
#include "dv_encode_tables.h"

namespace midv {

constexpr int kEncLive = 60;        // lanes of a wave that hold a block
constexpr int kEncPStride = 65;     // dwords of a lane's products / levels: 64 in scan order, + 1 (odd: no bank conflicts)
constexpr int kEncBitStride = 61;   // dwords of a lane's code words: at most 63 x 29 + 4 = 1831 bits, + 2 to read past, odd
constexpr int kEncSegWords = 101;   // a segment's five DIF blocks, + 1
constexpr uint32_t kEncSegBits = 2680;
constexpr int kEncStats = 17;       // segments per chosen quantisation number, then the dropped levels
template <class Sys>
constexpr int kEncGridX = Sys::kPairs + Sys::kChans * Sys::kSeqs;  // the video waves, then one workgroup per DIF sequence
// what a system's header says beside DSF (tests/dvsys.py: Layout.apt, Layout.stype)
template <class Sys>
constexpr uint32_t kEncApt = (Sys::kId == Sys525::kId || Sys::kId == Sys625::kId) ? 0u : 1u;
template <class Sys>
constexpr uint32_t kEncStype = Sys::kChans == 2 ? 4u : 0u;

// (x c + 2048) >> 12
__device__ __forceinline__ int enc_mul(int x, int c) { return (__mul24(x, c) + 2048) >> 12; }
// the scaled 8-point forward butterfly and its even half (tests/dvenc.py: _fdct8, _fdct4)
__device__ __forceinline__ void enc_fdct8(const int (&x)[8], int (&o)[8]) {
  const int t0 = x[0] + x[7], t7 = x[0] - x[7], t1 = x[1] + x[6], t6 = x[1] - x[6];
  const int t2 = x[2] + x[5], t5 = x[2] - x[5], t3 = x[3] + x[4], t4 = x[3] - x[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  const int z1 = enc_mul(t12 + t13, 2896);
  o[0] = t10 + t11; o[4] = t10 - t11; o[2] = t13 + z1; o[6] = t13 - z1;
  const int u10 = t4 + t5, u11 = t5 + t6, u12 = t6 + t7;
  const int z5 = enc_mul(u10 - u12, 1567);
  const int z2 = enc_mul(u10, 2217) + z5, z4 = enc_mul(u12, 5352) + z5, z3 = enc_mul(u11, 2896);
  const int z11 = t7 + z3, z13 = t7 - z3;
  o[5] = z13 + z2; o[3] = z13 - z2; o[1] = z11 + z4; o[7] = z11 - z4;
}
__device__ __forceinline__ void enc_fdct4(int x0, int x1, int x2, int x3, int (&o)[4]) {
  const int t10 = x0 + x3, t13 = x0 - x3, t11 = x1 + x2, t12 = x1 - x2;
  const int z1 = enc_mul(t12 + t13, 2896);
  o[0] = t10 + t11; o[1] = t13 + z1; o[2] = t10 - t11; o[3] = t13 - z1;
}

// n bits (at most 128) from bit `from` of src to bit `to` of dst (both read or written one dword past their last bit)
__device__ __forceinline__ void enc_copy_bits(const uint32_t* src, uint32_t from, uint32_t* dst, uint32_t to, uint32_t n) {
  for (uint32_t done = 0; done < n && done < 128u; done += 32u) {
    const uint32_t cnt = n - done;
    uint32_t w = dv_peek(src, from + done);
    if (cnt < 32u) w &= ~(0xFFFFFFFFu >> cnt);
    dv_or_bits(dst, to + done, w);
  }
}

// sums and maxima over the two segments of a wave at once: lanes 0..29 and 30..59
__device__ __forceinline__ uint32_t enc_seg_sum(uint32_t v, uint32_t seg) {  // a segment's sum stays below 2^16
  uint32_t x = seg == 0u ? v : seg == 1u ? v << 16 : 0u;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x += (uint32_t)__shfl_xor((int)x, d, 64);
  return seg == 0u ? x & 0xFFFFu : x >> 16;
}
__device__ __forceinline__ uint32_t enc_seg_max(uint32_t v, uint32_t seg) {
  uint32_t a = seg == 0u ? v : 0u, b = seg == 1u ? v : 0u;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t oa = (uint32_t)__shfl_xor((int)a, d, 64), ob = (uint32_t)__shfl_xor((int)b, d, 64);
    a = oa > a ? oa : a;
    b = ob > b ? ob : b;
  }
  return seg == 0u ? a : b;
}
__device__ __forceinline__ uint32_t enc_scan(uint32_t v, int lane) {  // inclusive, over the wave
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
    if (lane >= d) incl += o;
  }
  return incl;
}

template <class Sys>
__global__ __launch_bounds__(64) void k_dv_encode(const uint8_t* __restrict__ pics, uint8_t* __restrict__ frames,
                                                  const EncTables* __restrict__ T, uint32_t flags,
                                                  unsigned long long* __restrict__ stats) {
  __shared__ uint32_t s_P[kEncLive * kEncPStride], s_bits[kEncLive * kEncBitStride], s_out[2][kEncSegWords];
  __shared__ uint32_t s_word[kEncRuns * kEncAmps], s_sh[22], s_a[64], s_l[64], s_p[64], s_x[64], s_y[64], s_q[2];
  const int lane = threadIdx.x;
  constexpr uint32_t kFrameSeqs = Sys::kChans * Sys::kSeqs;
  uint8_t* const frame = frames + (size_t)blockIdx.y * Sys::kFrameBytes;

  // ---- the non-video DIF blocks of one sequence: header, 2 subcode, 3 VAUX, 9 audio ----
  if (blockIdx.x >= (uint32_t)Sys::kPairs) {
    const uint32_t fs = blockIdx.x - (uint32_t)Sys::kPairs;
    if (fs >= kFrameSeqs) return;
    const uint32_t chan = fs / (uint32_t)Sys::kSeqs, sq = fs - chan * (uint32_t)Sys::kSeqs;
    for (uint32_t i = lane; i < 15u * 20u; i += 64u) {
      const uint32_t nb = i / 20u, w = i - 20u * nb;
      const uint32_t b = nb < 6u ? nb : 6u + 16u * (nb - 6u);
      uint32_t val = 0u;
      if (w == 0u) {
        const uint32_t sct = b == 0u ? 0u : b < 3u ? 1u : b < 6u ? 2u : 3u;
        const uint32_t num = b == 0u ? 0u : b < 3u ? b - 1u : b < 6u ? b - 3u : nb - 6u;
        val = ((sct << 5) | 0x1Fu) | ((sq << 4) | (chan << 3) | 7u) << 8 | num << 16;
        if (b == 0u) val |= (Sys::kSeqs == 12 ? 0xBFu : 0x3Fu) << 24;  // DSF
      }
      if (b == 0u && w == 1u) val = kEncApt<Sys> << 8;                                  // byte 5: APT
      if (b == 5u && w == 12u && (fs == 0u || kEncStype<Sys> != 0u)) val = kEncStype<Sys> << 24;  // byte 48 + 3: stype
      *(uint32_t*)(frame + (size_t)(fs * 150u + b) * 80u + 4u * w) = val;
    }
    return;
  }

  for (int i = lane; i < kEncRuns * kEncAmps; i += 64) s_word[i] = (&T->word[0][0])[i];
  if (lane < 22) s_sh[lane] = T->shift4[lane];
  const uint32_t eob = T->eob;
  for (int i = lane; i < 2 * kEncSegWords; i += 64) (&s_out[0][0])[i] = 0u;
  dv_wave_sync();

  // ---- which block this lane has ----
  const uint32_t pair = blockIdx.x;
  const bool live = lane < kEncLive;
  const uint32_t seg = (uint32_t)lane / 30u;  // 2: the idle lanes
  const uint32_t segc = seg < 2u ? seg : 1u;
  const uint32_t b30 = (uint32_t)lane - 30u * seg, mbi = live ? b30 / 6u : 0u, j = live ? b30 - 6u * mbi : 0u;
  const uint32_t mb10 = live ? (uint32_t)lane / 6u : 9u;
  const uint32_t S = 2u * pair + segc;  // video segment of the frame (below kSegments: kPairs waves, kSegments even)
  const uint32_t seq = S / 27u, slot = S - 27u * seq;
  constexpr bool k422 = Sys::kChans == 2;
  const bool shown = live && !(k422 && (j == 1u || j == 3u));

  // ---- the block's pixels: where the decoder stores them (dv_decode_kernels.h) ----
  uint32_t lo[8], hi[8];
  {
    uint32_t mx, my8;
    Sys::place(seq, slot, mbi, mx, my8);
    uint32_t stride, org;
    bool halves = false;
    if constexpr (Sys::k411) {
      constexpr uint32_t kW = Sys::kW, kH = Sys::kH, kCW = Sys::kCW;
      const bool edge = mx == 22u;
      if (j < 4u) {
        stride = kW;
        org = edge ? (8u * my8 + 8u * (j >> 1)) * kW + 32u * mx + 8u * (j & 1u) : 8u * my8 * kW + 32u * mx + 8u * j;
      } else {
        stride = kCW;
        org = kW * kH + (j == 4u ? kCW * kH : 0u) + 8u * my8 * kCW + 8u * mx;  // block 4 is Cr (third plane), block 5 Cb
      }
      halves = j >= 4u && edge;  // the right-edge chroma block: left half here, right half eight lines below
    } else if constexpr (k422) {
      constexpr uint32_t W = Sys::kW, H = Sys::kH, CW = Sys::kCW, CH = Sys::kCH;
      if (j < 4u) {
        stride = W;
        org = 8u * my8 * W + 16u * mx + 8u * (j >> 1);
      } else {
        stride = CW;
        org = W * H + (j == 4u ? CW * CH : 0u) + 8u * my8 * CW + 8u * mx;
      }
    } else {
      constexpr uint32_t W = Sys::kW, H = Sys::kH, CW = Sys::kCW, CH = Sys::kCH;
      if (j < 4u) {
        stride = W;
        org = (16u * my8 + 8u * (j >> 1)) * W + 16u * mx + 8u * (j & 1u);
      } else {
        stride = CW;
        org = W * H + (j == 4u ? CW * CH : 0u) + 8u * my8 * CW + 8u * mx;
      }
    }
    const uint8_t* pic = pics + (size_t)blockIdx.y * Sys::kPicBytes;
#pragma unroll
    for (int r = 0; r < 8; r++) {
      lo[r] = hi[r] = 0x80808080u;  // flat 128: the areas a system does not show, and the idle lanes
      if (shown) {
        const uint8_t* p = pic + org + (uint32_t)r * stride;
        lo[r] = *(const uint32_t*)p;
        hi[r] = halves ? *(const uint32_t*)(pic + org + (uint32_t)(r + 8) * stride) : *(const uint32_t*)(p + 4);
      }
    }
  }
  // ---- mode: 2-4-8 where neighbouring lines differ much more than lines two apart ----
  uint32_t mode;
  {
    uint32_t d1 = 0, d2 = 0;
#pragma unroll
    for (int r = 0; r < 6; r++) {
      d1 = __builtin_amdgcn_sad_u8(lo[r], lo[r + 1], d1);
      d1 = __builtin_amdgcn_sad_u8(hi[r], hi[r + 1], d1);
      d2 = __builtin_amdgcn_sad_u8(lo[r], lo[r + 2], d2);
      d2 = __builtin_amdgcn_sad_u8(hi[r], hi[r + 2], d2);
    }
    mode = (flags & 1u) && d1 > 2u * d2 + 64u ? 1u : 0u;
  }
  // ---- forward transform: along the lines, then down the columns ----
  int c[64];
#pragma unroll
  for (int r = 0; r < 8; r++) {
    int x[8], o[8];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      x[k] = ((int)((lo[r] >> (8 * k)) & 255u) - 128) * 8;
      x[4 + k] = ((int)((hi[r] >> (8 * k)) & 255u) - 128) * 8;
    }
    enc_fdct8(x, o);
#pragma unroll
    for (int h = 0; h < 8; h++) c[8 * r + h] = o[h];
  }
  if (mode == 0u) {
#pragma unroll
    for (int h = 0; h < 8; h++) {
      int x[8], o[8];
#pragma unroll
      for (int r = 0; r < 8; r++) x[r] = c[8 * r + h];
      enc_fdct8(x, o);
#pragma unroll
      for (int r = 0; r < 8; r++) c[8 * r + h] = o[r];
    }
  } else {  // 2-4-8: rows 2v / 2v + 1 hold frequency v of the line pairs' sums / differences
#pragma unroll
    for (int h = 0; h < 8; h++) {
      int a[4], b[4];
      enc_fdct4(c[h] + c[8 + h], c[16 + h] + c[24 + h], c[32 + h] + c[40 + h], c[48 + h] + c[56 + h], a);
      enc_fdct4(c[h] - c[8 + h], c[16 + h] - c[24 + h], c[32 + h] - c[40 + h], c[48 + h] - c[56 + h], b);
#pragma unroll
      for (int v = 0; v < 4; v++) {
        c[8 * (2 * v) + h] = a[v];
        c[8 * (2 * v + 1) + h] = b[v];
      }
    }
  }
  int dc = (c[0] + 128) >> 8;
  dc = dc < -256 ? -256 : dc > 255 ? 255 : dc;
  // ---- the products |c| m, in scan order, and the signs ----
  uint32_t* const myP = s_P + (live ? lane : 0) * kEncPStride;
  unsigned long long sgn = 0ull;
  uint32_t maxP = 0u;
#pragma unroll
  for (int i = 1; i < 64; i++) {
    const uint32_t m = mode ? kEncMult[1][i] : kEncMult[0][i], k = mode ? kEncPos[1][i] : kEncPos[0][i];
    const uint32_t a = (uint32_t)(c[i] < 0 ? -c[i] : c[i]);
    const uint32_t P = __umul24(a, m);
    if (live) myP[k] = P;
    if (c[i] < 0) sgn |= 1ull << k;
    maxP = P > maxP ? P : maxP;
  }
  uint32_t cls = 0u;
  if (flags & 2u) {
    const uint32_t big = maxP >> kEncFrac;
    cls = (big >= 12u ? 1u : 0u) + (big >= 36u ? 1u : 0u) + (big >= 144u ? 1u : 0u);
  }
  const uint32_t cls_off = cls == 0u ? 6u : cls == 1u ? 3u : cls == 2u ? 0u : 1u;
  dv_wave_sync();

  // bits of a pair's word or words, sign included / the word itself (at most 30 bits)
  auto pair_len = [&](uint32_t run, uint32_t amp) -> uint32_t {
    const uint32_t e = run < (uint32_t)kEncRuns && amp < (uint32_t)kEncAmps ? s_word[run * kEncAmps + amp] : 0u;
    if (e) return (e >> 16) + 1u;
    uint32_t n = amp < (uint32_t)kEncAmps ? (s_word[amp] >> 16) + 1u : 16u;
    if (run) n += run - 1u < 6u ? s_word[(run - 1u) * kEncAmps] >> 16 : 13u;
    return n;
  };
  auto pair_word = [&](uint32_t run, uint32_t amp, uint32_t neg, uint32_t& len) -> uint32_t {
    const uint32_t e = run < (uint32_t)kEncRuns && amp < (uint32_t)kEncAmps ? s_word[run * kEncAmps + amp] : 0u;
    if (e) {
      len = (e >> 16) + 1u;
      return (e & 0xFFFFu) << 1 | neg;
    }
    uint32_t v = 0u, n = 0u;
    if (run) {
      const uint32_t z = run - 1u < 6u ? s_word[(run - 1u) * kEncAmps] : ((0x7Eu << 6) | (run - 1u)) | 13u << 16;
      v = z & 0xFFFFu;
      n = z >> 16;
    }
    const uint32_t a = amp < (uint32_t)kEncAmps ? s_word[amp] : ((0x7Fu << 8) | amp) | 15u << 16;
    v = v << (a >> 16) | (a & 0xFFFFu);
    n += a >> 16;
    len = n + 1u;
    return v << 1 | neg;
  };
  // the level at scan position k under the four shifts sh4 (area 0 in the low nibble)
  auto level_at = [&](uint32_t k, uint32_t sh4) -> uint32_t {
    const uint32_t area = k < 6u ? 0u : k < 21u ? 1u : k < 43u ? 2u : 3u;
    const uint32_t n = (uint32_t)kEncFrac + ((sh4 >> (4u * area)) & 15u);
    const uint32_t lv = (myP[k] + (1u << (n - 1u))) >> n;
    return lv > 255u ? 255u : lv;
  };
  auto shifts_of = [&](uint32_t q) -> uint32_t { return s_sh[q + cls_off] + (cls == 3u ? 0x1111u : 0u); };

  // ---- rate control: downwards from 15 until both segments fit ----
  uint32_t qno = 0u, mybits = 0u;
  bool decided = !live;
  for (int q = 15; q >= 0; q--) {
    uint32_t bits = 0u;
    if (!decided) {
      const uint32_t sh4 = shifts_of((uint32_t)q);
      uint32_t run = 0u;
      bits = eob >> 16;
#pragma unroll 1
      for (uint32_t k = 1; k < 64u; k++) {
        const uint32_t lv = level_at(k, sh4);
        if (lv) {
          bits += pair_len(run, lv);
          run = 0u;
        } else {
          run++;
        }
      }
    }
    const uint32_t total = enc_seg_sum(bits, seg);
    if (!decided && (total <= kEncSegBits || q == 0)) {
      decided = true;
      qno = (uint32_t)q;
      mybits = bits;
    }
    if (__all(decided)) break;
  }
  // the levels stay where the products were
  uint32_t last = 0u;
  if (live) {
    const uint32_t sh4 = shifts_of(qno);
#pragma unroll 1
    for (uint32_t k = 1; k < 64u; k++) {
      const uint32_t lv = level_at(k, sh4);
      myP[k] = lv;
      if (lv) last = k;
    }
  }
  // ---- the overflow rule: the first block with the most bits loses its last level (a lane's bits change by the length
  // of its last word or words) ----
  uint32_t dropped = 0u;
  for (int step = 0; step < 30 * 63; step++) {
    const uint32_t total = enc_seg_sum(mybits, seg);
    const bool over = live && total > kEncSegBits;
    if (!__any(over)) break;
    const uint32_t key = over ? mybits << 5 | (31u - b30) : 0u;
    const uint32_t top = enc_seg_max(key, seg);
    if (over && key == top && last > 0u) {
      const uint32_t amp = myP[last];
      uint32_t k = last - 1u;
      for (int guard = 0; guard < 64 && k >= 1u && myP[k] == 0u; guard++) k--;
      mybits -= pair_len(last - k - 1u, amp);
      myP[last] = 0u;
      last = k;
      dropped++;
    }
  }
  {
    const uint32_t all_dropped = enc_seg_sum(dropped, seg);
    if (live && b30 == 0u) {
      s_q[seg] = qno;
      atomicAdd(&stats[qno], 1ull);
      if (all_dropped) atomicAdd(&stats[16], (unsigned long long)all_dropped);
    }
  }
  // ---- the block's code words ----
  uint32_t* const bb = s_bits + (live ? lane : 0) * kEncBitStride;
  uint32_t nbits = 0u;
  if (live) {
    unsigned long long acc = 0ull;
    uint32_t fill = 0u, w = 0u, run = 0u;
    auto append = [&](uint32_t v, uint32_t len) {  // len <= 30, fill < 32
      acc |= (unsigned long long)v << (64u - fill - len);
      fill += len;
      if (fill >= 32u) {
        bb[w++] = (uint32_t)(acc >> 32);
        acc <<= 32;
        fill -= 32u;
      }
    };
#pragma unroll 1
    for (uint32_t k = 1; k < 64u; k++) {
      const uint32_t lv = myP[k];
      if (!lv) {
        run++;
        continue;
      }
      uint32_t len;
      const uint32_t v = pair_word(run, lv, (uint32_t)(sgn >> k) & 1u, len);
      append(v, len);
      run = 0u;
    }
    append(eob & 0xFFFFu, eob >> 16);
    bb[w] = (uint32_t)(acc >> 32);
    bb[w + 1u] = 0u;
    nbits = 32u * w + fill;
  }
  // ---- pass 1: header and the block's own area ----
  const uint32_t ao = j < 4u ? 4u + 14u * j : 60u + 10u * (j - 4u);
  const uint32_t cap = j < 4u ? 100u : 68u;
  const uint32_t base = 640u * mbi + 8u * ao;  // the area's first bit in the segment's five DIF blocks
  uint32_t* const out = s_out[segc];
  const uint32_t n1 = nbits < cap ? nbits : cap;
  const uint32_t fre = live ? cap - n1 : 0u, dem = nbits - n1;
  if (live) {
    dv_or_bits(out, base, (((uint32_t)dc & 511u) << 3 | mode << 2 | cls) << 20);
    enc_copy_bits(bb, 0u, out, base + 12u, n1);
  }
  // a lane with demand takes its share [at, at + take) of the group's free stream, which is the supplies s_a / s_l / s_p
  // (stream offset, length, first bit in the segment) of `cnt` lanes from lane `first` on
  auto pour = [&](uint32_t first, uint32_t cnt, uint32_t at, uint32_t take, uint32_t from) {
    if (!take) return;
    for (uint32_t i = 0; i < cnt; i++) {
      const uint32_t a = s_a[first + i], l = s_l[first + i];
      const uint32_t b = at > a ? at : a, e = at + take < a + l ? at + take : a + l;
      if (b < e) enc_copy_bits(bb, from + (b - at), out, s_p[first + i] + (b - a), e - b);
    }
  };
  // ---- pass 2: the macroblock's free bits, in block order ----
  uint32_t take2, rest, rest_at;
  {
    const uint32_t xf = enc_scan(fre, lane) - fre, xd = enc_scan(dem, lane) - dem;
    s_x[lane] = xf;
    s_y[lane] = xd;
    dv_wave_sync();
    const uint32_t f0 = s_x[6u * mb10], d0 = s_y[6u * mb10];
    const uint32_t tot_f = s_x[6u * mb10 + 6u] - f0, tot_d = s_y[6u * mb10 + 6u] - d0;
    const uint32_t a = xf - f0, at = xd - d0;
    s_a[lane] = a;
    s_l[lane] = fre;
    s_p[lane] = base + 12u + n1;
    dv_wave_sync();
    take2 = at < tot_f ? (tot_f - at < dem ? tot_f - at : dem) : 0u;
    if (live) pour(6u * mb10, 6u, at, take2, n1);
    // what pass 2 left of this block's free bits is the segment's
    const uint32_t used = tot_d < tot_f ? tot_d : tot_f;
    rest = a + fre > used ? (a + fre - used < fre ? a + fre - used : fre) : 0u;
    rest_at = base + 12u + n1 + (fre - rest);
    dv_wave_sync();
  }
  // ---- pass 3: the segment's free bits, in macroblock then block order ----
  {
    const uint32_t dem3 = dem - take2;
    const uint32_t xf = enc_scan(rest, lane) - rest, xd = enc_scan(dem3, lane) - dem3;
    s_x[lane] = xf;
    s_y[lane] = xd;
    dv_wave_sync();
    const uint32_t f0 = s_x[30u * segc], d0 = s_y[30u * segc];
    const uint32_t tot_f = s_x[30u * segc + 30u] - f0;
    const uint32_t at = xd - d0;
    s_a[lane] = xf - f0;
    s_l[lane] = rest;
    s_p[lane] = rest_at;
    dv_wave_sync();
    const uint32_t take3 = at < tot_f ? (tot_f - at < dem3 ? tot_f - at : dem3) : 0u;
    if (live) pour(30u * segc, 30u, at, take3, n1 + take2);
    dv_wave_sync();
  }
  // ---- row stores of the ten DIF blocks ----
  for (uint32_t i = lane; i < 200u; i += 64u) {
    const uint32_t sg = i / 100u, wi = i - 100u * sg, m = wi / 20u, w = wi - 20u * m;
    const uint32_t S2 = 2u * pair + sg, fs = S2 / 27u, v = 5u * (S2 - 27u * fs) + m;
    const uint32_t chan = fs / (uint32_t)Sys::kSeqs, sq = fs - chan * (uint32_t)Sys::kSeqs;
    uint32_t val = __builtin_bswap32(s_out[sg][wi]);
    if (w == 0u) val = 0x9Fu | ((sq << 4) | (chan << 3) | 7u) << 8 | v << 16 | s_q[sg] << 24;  // ids; STA 0 | QNO
    *(uint32_t*)(frame + (size_t)(fs * 150u + 7u + v + v / 15u) * 80u + 4u * w) = val;
  }
}

}  // namespace midv
