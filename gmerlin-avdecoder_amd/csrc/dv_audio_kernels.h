// dv_audio_kernels.h — gfx950 kernels of the DV sound, all five systems (the statement: tests/dvaudio.py, which these
// reproduce byte for byte, and through it csrc/dvframe_host.c's mi_dv_extract_audio; the layout: DESIGN.md section 9.8).
//
//   k_dv_audio_extract<Sys>  resident frames -> PCM.  One workgroup per (stereo pair of the output, frame).  It reads the
//                  frame's AAUX source pack (every frame of a batch has its own sample count, rate and quantisation),
//                  zeroes an image of the pair's buffer in LDS, scatters the samples of its audio blocks into it (16-bit:
//                  the channel `pair`, two big-endian samples a dword; 12-bit: half the sequences of channel pair / 2,
//                  four byte triples = three dwords = eight samples an item, expanded to 16 bits), and stores the image in
//                  16-byte rows.  The workgroup of pair 0 writes the frame's row of d_info.
//   k_dv_audio_write<Sys>    PCM -> the audio DIF blocks of resident frames, 16-bit mode: the inverse.  One workgroup per
//                  (channel, frame): the channel's pair into LDS in 16-byte rows, then every dword of the channel's
//                  9 kSeqs audio blocks: ids as k_dv_encode writes them, the AAUX packs, two samples gathered from LDS.
//
// Integer only.  A slot is below 107 + 35 * 108 + 1 = 3888 < 4096 whatever the pack says, so the image holds every slot
// a block can name; the grid is exact (no guard on the frame index needed), and both kernels touch only their frame's
// audio blocks and their pair's kAudioPairBytes.
#pragma once
#include <hip/hip_runtime.h>

#include "dv_common.h"

namespace midv {

constexpr int kAudioPairs = 4;          // stereo pairs a frame can carry (MI_DV_AUDIO_PAIRS)
constexpr int kAudioPairBytes = 8192;   // a pair's buffer: 4096 slots (MI_DV_AUDIO_PAIR_BYTES)
constexpr int kAudioThreads = 256;
constexpr uint32_t kAudioPackAt = 80u * 6u + 80u * 16u * 3u + 3u;  // the AAUX source pack: audio block 3 of sequence 0
template <class Sys>
constexpr uint32_t kAudioLine = Sys::kSeqs == 12 ? 1u : 0u;  // the row of AudioTables
// audio block j of sequence q of channel c: DIF block 6 + 16 j of its sequence
template <class Sys>
__device__ __forceinline__ uint32_t audio_block_at(uint32_t c, uint32_t q, uint32_t j) {
  return ((c * (uint32_t)Sys::kSeqs + q) * 150u + 6u + 16u * j) * 80u;
}

// 12-bit non-linear code to 16 bits (csrc/dvframe_host.c: mi_dv_audio_12to16): magnitudes in eight segments of 256 codes,
// segment k >= 2 is 2^(k-1) times as wide; negative codes are the one's complement of the positive law
__device__ __forceinline__ uint32_t audio_expand_magnitude(uint32_t m) {
  const uint32_t k = m >> 8;
  return k < 2u ? m : (m - 256u * (k - 1u)) << (k - 1u);
}
__device__ __forceinline__ uint32_t audio_12to16(uint32_t s) {  // s: 0..0xfff; 0x800 is "no sample"
  if (s == 0x800u) return 0u;
  return (s & 0x800u ? ~audio_expand_magnitude(~s & 0x7FFu) : audio_expand_magnitude(s)) & 0xFFFFu;
}

template <class Sys>
__global__ __launch_bounds__(kAudioThreads) void k_dv_audio_extract(const uint8_t* __restrict__ frames, uint8_t* __restrict__ pcm,
                                                                    uint32_t pairs, int32_t* __restrict__ info,
                                                                    const AudioTables* __restrict__ T) {
  __shared__ uint4 s_img[kAudioPairBytes / 16];
  __shared__ uint16_t s_shuf[12 * 9];
  constexpr uint32_t kL = kAudioLine<Sys>, kSeqs = Sys::kSeqs, kHalf = kSeqs / 2u, kChans = Sys::kChans;
  const uint32_t t = threadIdx.x, pair = blockIdx.x, fr = blockIdx.y;
  const uint8_t* const frame = frames + (size_t)fr * Sys::kFrameBytes;
  uint16_t* const img = (uint16_t*)s_img;

  for (uint32_t i = t; i < (uint32_t)kAudioPairBytes / 16u; i += kAudioThreads) s_img[i] = uint4{0u, 0u, 0u, 0u};
  if (t < kSeqs * 9u) s_shuf[t] = (&T->shuffle[kL][0][0])[t];
  // ---- the source pack: what the host reader reads (mi_dv_extract_audio) ----
  const uint8_t* const as = frame + kAudioPackAt;
  const uint32_t b4 = as[4], extra = as[1] & 0x3Fu, freq = (b4 >> 3) & 7u, quant = b4 & 7u;
  int32_t samples = 0;
  if (as[0] == 0x50u) samples = quant > 1u || freq > 2u ? -1 : (int32_t)T->min_samples[kL][freq < 3u ? freq : 0u] + (int32_t)extra;
  const bool twelve = quant == 1u;
  if (pair == 0u && t == 0u) {
    const bool ok = samples > 0;
    info[4u * fr + 0u] = samples;
    info[4u * fr + 1u] = ok ? (freq == 0u ? 48000 : freq == 1u ? 44100 : 32000) : 0;
    info[4u * fr + 2u] = ok ? (int32_t)(twelve ? 2u * kChans : kChans) : 0;
    info[4u * fr + 3u] = ok ? (twelve ? 12 : 16) : 0;
  }
  __syncthreads();

  if (samples > 0) {
    const uint32_t limit = 2u * (uint32_t)samples, stride = T->stride[kL];
    if (!twelve) {
      if (pair < kChans) {
        for (uint32_t item = t; item < kSeqs * 9u * 18u; item += kAudioThreads) {
          const uint32_t blk = item / 18u, w = item - 18u * blk, q = blk / 9u, j = blk - 9u * q;
          const uint32_t d = *(const uint32_t*)(frame + audio_block_at<Sys>(pair, q, j) + 8u + 4u * w);
          const uint32_t v0 = (d & 0xFFu) << 8 | ((d >> 8) & 0xFFu), v1 = ((d >> 16) & 0xFFu) << 8 | d >> 24;
          const uint32_t s0 = (uint32_t)s_shuf[blk] + 2u * w * stride, s1 = s0 + stride;
          if (s0 < limit) img[s0] = (uint16_t)(v0 == 0x8000u ? 0u : v0);
          if (s1 < limit) img[s1] = (uint16_t)(v1 == 0x8000u ? 0u : v1);
        }
      }
    } else {
      const uint32_t c = pair >> 1, h = pair & 1u;
      if (c < kChans) {
        for (uint32_t item = t; item < kHalf * 9u * 6u; item += kAudioThreads) {
          const uint32_t blk = item / 6u, g = item - 6u * blk, qh = blk / 9u, j = blk - 9u * qh;
          const uint32_t* p = (const uint32_t*)(frame + audio_block_at<Sys>(c, h * kHalf + qh, j) + 8u + 12u * g);
          const uint32_t d[3] = {p[0], p[1], p[2]};
          const uint32_t base_l = s_shuf[blk], base_r = s_shuf[blk + 9u * kHalf];
#pragma unroll
          for (uint32_t i = 0; i < 4u; i++) {
            // the triple's bytes 3 i, 3 i + 1, 3 i + 2 of the twelve
            const uint32_t t0 = (d[(3u * i) >> 2] >> (8u * ((3u * i) & 3u))) & 0xFFu;
            const uint32_t t1 = (d[(3u * i + 1u) >> 2] >> (8u * ((3u * i + 1u) & 3u))) & 0xFFu;
            const uint32_t t2 = (d[(3u * i + 2u) >> 2] >> (8u * ((3u * i + 2u) & 3u))) & 0xFFu;
            const uint32_t n = 4u * g + i, sl = base_l + n * stride, sr = base_r + n * stride;
            if (sl >= limit) continue;  // (the left slot alone decides, as in the host reader)
            img[sl] = (uint16_t)audio_12to16(t0 << 4 | t2 >> 4);
            img[sr] = (uint16_t)audio_12to16(t1 << 4 | (t2 & 0xFu));
          }
        }
      }
    }
  }
  __syncthreads();
  uint4* const out = (uint4*)(pcm + ((size_t)fr * pairs + pair) * (size_t)kAudioPairBytes);
  for (uint32_t i = t; i < (uint32_t)kAudioPairBytes / 16u; i += kAudioThreads) out[i] = s_img[i];
}

// what a system's AAUX source pack says of it: the 50 Mbit/s systems are stype 2 (two pairs), the others 0
template <class Sys>
constexpr uint32_t kAudioStype = Sys::kChans == 2 ? 2u : 0u;

template <class Sys>
__global__ __launch_bounds__(kAudioThreads) void k_dv_audio_write(uint8_t* __restrict__ frames, const uint8_t* __restrict__ pcm,
                                                                  uint32_t pairs, uint32_t freq, const int32_t* __restrict__ samples,
                                                                  const AudioTables* __restrict__ T) {
  __shared__ uint4 s_img[kAudioPairBytes / 16];
  __shared__ uint16_t s_shuf[12 * 9];
  constexpr uint32_t kL = kAudioLine<Sys>, kSeqs = Sys::kSeqs, kHalf = kSeqs / 2u;
  const uint32_t t = threadIdx.x, chan = blockIdx.x, fr = blockIdx.y;
  uint8_t* const frame = frames + (size_t)fr * Sys::kFrameBytes;
  const uint16_t* const img = (const uint16_t*)s_img;

  const uint4* const in = (const uint4*)(pcm + ((size_t)fr * pairs + chan) * (size_t)kAudioPairBytes);
  for (uint32_t i = t; i < (uint32_t)kAudioPairBytes / 16u; i += kAudioThreads) s_img[i] = in[i];
  if (t < kSeqs * 9u) s_shuf[t] = (&T->shuffle[kL][0][0])[t];
  const uint32_t smp = (uint32_t)samples[fr], limit = 2u * smp, stride = T->stride[kL];
  const uint32_t extra = (smp - (uint32_t)T->min_samples[kL][freq]) & 0x3Fu;  // (the host layer has checked the window)
  __syncthreads();

  for (uint32_t item = t; item < kSeqs * 9u * 20u; item += kAudioThreads) {
    const uint32_t blk = item / 20u, w = item - 20u * blk, q = blk / 9u, j = blk - 9u * q;
    uint32_t val;
    if (w < 2u) {
      // the AAUX pack of this block: 0x50 .. 0x53 in blocks 3..6 of even sequences and 0..3 of odd ones, else none
      const uint32_t k = q & 1u ? j : j - 3u;  // (wraps past 3 for j < 3)
      uint32_t p0 = 0xFFu, p1234 = 0xFFFFFFFFu;
      if (k == 0u) {  // source: unlocked | samples beyond the minimum; the half; 1 1 DSF stype; 1 rate, 16-bit
        p0 = 0x50u;
        p1234 = (0xC0u | extra) | (q >= kHalf ? 1u : 0u) << 8 | (0xC0u | kL << 5 | kAudioStype<Sys>) << 16 | (0x80u | freq << 3) << 24;
      } else if (k == 1u) {  // source control
        p0 = 0x51u;
        p1234 = 0x3Fu | 0xCFu << 8 | 0xA0u << 16 | 0xFFu << 24;
      } else if (k < 4u) {  // rec date, rec time: no information
        p0 = 0x50u + k;
      }
      val = w == 0u ? (0x7Fu | ((q << 4) | (chan << 3) | 7u) << 8 | j << 16 | p0 << 24) : p1234;
    } else {
      const uint32_t s0 = (uint32_t)s_shuf[blk] + 2u * (w - 2u) * stride, s1 = s0 + stride;
      uint32_t v0 = s0 < limit ? img[s0] : 0u, v1 = s1 < limit ? img[s1] : 0u;
      v0 = v0 == 0x8000u ? 0x8001u : v0;  // (0x8000 is the format's "no sample")
      v1 = v1 == 0x8000u ? 0x8001u : v1;
      val = v0 >> 8 | (v0 & 0xFFu) << 8 | (v1 >> 8) << 16 | (v1 & 0xFFu) << 24;
    }
    *(uint32_t*)(frame + audio_block_at<Sys>(chan, q, j) + 4u * w) = val;
  }
}

}  // namespace midv
