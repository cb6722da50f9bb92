// dv_meta_kernels.h — gfx950 kernels of the DV timecode, recording date and time and the aspect flag, all five systems
// (the statement: tests/dvmeta.py, which these reproduce value for value and byte for byte; the layout: DESIGN.md section
// 9.9).  PARITY UNPINNED: the reader restates GetSSYBPack and its users (lib/dvframe.c:678-783, :460-471, through
// csrc/dvframe_host.c); the packs the writer makes are this repository's reading of IEC 61834-2/-4.
//
//   k_dv_meta_extract<Sys>  resident frames -> meta[n][kMetaInts].  One wave per frame, four in a workgroup.  The 12 kSeqs
//                  subcode packets of channel 0 (sequence i, block j, packet k: candidate c = 12 i + 6 j + k, the order the
//                  host reader scans them in) go to lane c % 64 in round c / 64; a lane reads its packet's five pack bytes
//                  as two aligned dwords (a pack lies at an even offset that is no multiple of 4).  Per pack id a ballot a
//                  round: the lowest lane of the first round with a hit is the reader's first hit, and its four bytes are
//                  broadcast.  Lanes 0..15 store the row as one 64-byte line.
//   k_dv_meta_write<Sys>    the two subcode and three VAUX blocks of every sequence of resident frames, whole.  One
//                  workgroup per frame: lane 0 makes the frame's timecode and civil date (the only divisions of 64-bit
//                  numbers, all by constants) and leaves the three packs in LDS; then every thread makes whole dwords of
//                  the kChans kSeqs 5 blocks from (sequence, block, word) and stores them.
//
// Integer only.  Lane masks are 64 bits wide in every expression; every loop has a bound known at compile time; the
// extract grid is rounded up and guarded by the frame index (a whole wave leaves), the write grid is exact.  Both kernels
// find their frame as a 64-bit wave-uniform pointer and add offsets below the frame's size; the writer's stores are aligned
// dwords inside DIF blocks 1..5 of a sequence and nothing else.
#pragma once
#include <hip/hip_runtime.h>

#include "dv_common.h"

namespace midv {

constexpr int kMetaInts = 16;          // a row of d_meta (MI_DV_META_INTS)
constexpr int kMetaExtractWaves = 4;   // frames a workgroup of k_dv_meta_extract reads
constexpr int kMetaWriteThreads = 256;
constexpr uint32_t kMetaPackTimecode = 0x13u, kMetaPackSource = 0x60u, kMetaPackControl = 0x61u, kMetaPackDate = 0x62u,
                   kMetaPackTime = 0x63u;
constexpr uint32_t kMetaControlAt = 80u * 5u + 48u + 5u;  // the VAUX source control pack the aspect is read from
// what a system's header says beside DSF, as k_dv_encode writes it (dv_encode_kernels.h: kEncApt, kEncStype)
template <class Sys>
constexpr uint32_t kMetaApt = (Sys::kId == Sys525::kId || Sys::kId == Sys625::kId) ? 0u : 1u;
template <class Sys>
constexpr uint32_t kMetaStype = Sys::kChans == 2 ? 4u : 0u;
constexpr long long kMetaDropPeriod = 2589408;            // frames of 24 hours of drop-frame timecode
constexpr long long kMetaLastSecond = 3155760000ll;       // 2070-01-01 00:00:00: recording times lie below it

// ---- a frame number as a timecode, seconds as a civil date: the host call and the writer's lane 0 share them ----
// base 25 or 30; drop 1 (base 30 only) is SMPTE drop-frame: labels ;00 and ;01 are skipped at every minute that is no
// multiple of ten.  Hours wrap at 24.  hmsf: hours, minutes, seconds, frames
MIDV_HD void meta_timecode(uint32_t base, uint32_t drop, unsigned long long frame, uint32_t hmsf[4]) {
  uint32_t n = drop ? (uint32_t)(frame % (unsigned long long)kMetaDropPeriod)
                    : base == 25u ? (uint32_t)(frame % (86400ull * 25ull)) : (uint32_t)(frame % (86400ull * 30ull));
  if (drop) {
    const uint32_t d = n / 17982u, m = n - 17982u * d;
    n += 18u * d + (m >= 2u ? 2u * ((m - 2u) / 1798u) : 0u);
  }
  const uint32_t secs = base == 25u ? n / 25u : n / 30u;
  hmsf[3] = n - secs * base;
  hmsf[2] = secs % 60u;
  hmsf[1] = secs / 60u % 60u;
  hmsf[0] = secs / 3600u % 24u;
}
// seconds from 1970-01-01 00:00:00 (below 2^32) in the proleptic Gregorian calendar, no time zone: ymdhms
MIDV_HD void meta_civil(uint32_t seconds, uint32_t ymdhms[6]) {
  const uint32_t days = seconds / 86400u, sod = seconds - 86400u * days;
  const uint32_t z = days + 719468u, era = z / 146097u, doe = z - era * 146097u;  // days from 0000-03-01
  const uint32_t yoe = (doe - doe / 1460u + doe / 36524u - doe / 146096u) / 365u;
  const uint32_t doy = doe - (365u * yoe + yoe / 4u - yoe / 100u), mp = (5u * doy + 2u) / 153u;
  const uint32_t month = mp < 10u ? mp + 3u : mp - 9u;
  ymdhms[0] = yoe + era * 400u + (month <= 2u ? 1u : 0u);
  ymdhms[1] = month;
  ymdhms[2] = doy - (153u * mp + 2u) / 5u + 1u;
  ymdhms[3] = sod / 3600u;
  ymdhms[4] = sod / 60u % 60u;
  ymdhms[5] = sod % 60u;
}
MIDV_HD uint32_t meta_bcd(uint32_t v) { return (v / 10u) << 4 | v % 10u; }                               // v below 100
MIDV_HD uint32_t meta_unbcd(uint32_t b, uint32_t tens_mask) { return (b & 0xFu) + 10u * ((b >> 4) & tens_mask); }

// ============================================================================ reading
// byte k (1..4) of a pack whose bytes 1..4 are the dword `pay`, little-endian
__device__ __forceinline__ uint32_t meta_pack_byte(uint32_t pay, uint32_t k) { return (pay >> (8u * (k - 1u))) & 0xFFu; }

// the first of the wave's candidates, in scan order, whose id is `id`: hit[r] says the lane's candidate of round r carries
// it.  Returns whether there is one; pay: its bytes 1..4
template <int Rounds>
__device__ __forceinline__ bool meta_first_hit(const bool (&hit)[Rounds], const uint32_t (&pays)[Rounds], uint32_t& pay) {
  bool found = false;
  pay = 0u;
#pragma unroll
  for (int r = 0; r < Rounds; r++) {
    const unsigned long long m = __ballot(hit[r]);  // (64 bits: lanes 32..63 hold candidates too)
    if (!found && m != 0ull) {                      // (wave-uniform)
      found = true;
      pay = (uint32_t)__shfl((int)pays[r], (int)__builtin_ctzll(m), 64);
    }
  }
  return found;
}

template <class Sys>
__global__ __launch_bounds__(64 * kMetaExtractWaves) void k_dv_meta_extract(const uint8_t* __restrict__ frames, uint32_t n,
                                                                           int32_t* __restrict__ meta) {
  constexpr uint32_t kCands = 12u * (uint32_t)Sys::kSeqs;  // 120 or 144: the subcode packets of channel 0
  constexpr int kRounds = (int)((kCands + 63u) / 64u);
  static_assert(kRounds <= 3, "at most three rounds");
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t fr = blockIdx.x * (uint32_t)kMetaExtractWaves + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (fr >= n) return;  // (the whole wave; there is no barrier below)
  const uint8_t* const frame = frames + (size_t)fr * Sys::kFrameBytes;

  bool is_tc[kRounds], is_date[kRounds], is_time[kRounds];
  uint32_t pays[kRounds];
#pragma unroll
  for (int r = 0; r < kRounds; r++) {
    const uint32_t c = 64u * (uint32_t)r + lane;
    uint32_t id = 0xFFu;
    pays[r] = 0u;
    if (c < kCands) {
      const uint32_t i = c / 12u, jk = c - 12u * i, j = jk / 6u, k = jk - 6u * j;
      // the pack's byte 0 is at i 12000 + 80 (1 + j) + 6 + 8 k: two bytes into an aligned dword
      const uint32_t* const p = (const uint32_t*)(frame + (i * 12000u + 80u * (1u + j) + 4u + 8u * k));
      const uint32_t a = p[0], b = p[1];
      id = (a >> 16) & 0xFFu;
      pays[r] = a >> 24 | b << 8;
    }
    is_tc[r] = id == kMetaPackTimecode;
    is_date[r] = id == kMetaPackDate;
    is_time[r] = id == kMetaPackTime;
  }
  uint32_t tc, date, rtime;
  const bool has_tc = meta_first_hit<kRounds>(is_tc, pays, tc);
  const bool has_date = meta_first_hit<kRounds>(is_date, pays, date);
  const bool has_time = meta_first_hit<kRounds>(is_time, pays, rtime);
  // the aspect: mi_dv_pixel_aspect's rule (its APT is byte 4 of the frame)
  const uint32_t vsc = *(const uint32_t*)(frame + (kMetaControlAt - 1u)), head = *(const uint32_t*)(frame + 4u);
  const bool has_vsc = ((vsc >> 8) & 0xFFu) == kMetaPackControl;
  const uint32_t disp = (vsc >> 24) & 7u, apt = head & 7u;
  const uint32_t wide = has_vsc && (disp == 2u || (apt == 0u && disp == 7u)) ? 1u : 0u;
  uint32_t year = meta_unbcd(meta_pack_byte(date, 4u), 0xFu);
  year += year < 25u ? 2000u : 1900u;

  uint32_t v = (has_tc ? 1u : 0u) | (has_date ? 2u : 0u) | (has_time ? 4u : 0u) | (has_vsc ? 8u : 0u);
  v = lane == 1u ? meta_unbcd(meta_pack_byte(tc, 4u), 0x3u) : v;
  v = lane == 2u ? meta_unbcd(meta_pack_byte(tc, 3u), 0x7u) : v;
  v = lane == 3u ? meta_unbcd(meta_pack_byte(tc, 2u), 0x7u) : v;
  v = lane == 4u ? meta_unbcd(meta_pack_byte(tc, 1u), 0x3u) : v;
  v = lane == 5u ? (tc >> 6) & 1u : v;
  v = lane == 6u ? (has_date ? year : 0u) : v;
  v = lane == 7u ? meta_unbcd(meta_pack_byte(date, 3u), 0x1u) : v;
  v = lane == 8u ? meta_unbcd(meta_pack_byte(date, 2u), 0x3u) : v;
  v = lane == 9u ? meta_unbcd(meta_pack_byte(rtime, 4u), 0x3u) : v;
  v = lane == 10u ? meta_unbcd(meta_pack_byte(rtime, 3u), 0x7u) : v;
  v = lane == 11u ? meta_unbcd(meta_pack_byte(rtime, 2u), 0x7u) : v;
  v = lane == 12u ? wide : v;
  v = lane == 13u ? tc : v;
  v = lane == 14u ? date : v;
  v = lane == 15u ? rtime : v;
  if (lane < (uint32_t)kMetaInts) meta[(size_t)fr * kMetaInts + lane] = (int32_t)v;
}

// ============================================================================ writing
// a frame's three subcode packs as the writer keeps them in LDS: [pack] = {id | bytes 1..3 << 8, byte 4}
struct MetaPacks {
  uint32_t lo[3], hi[3];  // 0: timecode, 1: recording date, 2: recording time
};
__device__ __forceinline__ uint32_t meta_packs_byte(const MetaPacks& p, uint32_t which, uint32_t k) {  // k: 0..4
  return k < 4u ? (p.lo[which] >> (8u * k)) & 0xFFu : p.hi[which];
}

// byte `at` (0..79) of block b (0, 1: the subcode blocks; 2..4: the VAUX blocks) of sequence sq of channel chan
template <class Sys>
__device__ __forceinline__ uint32_t meta_block_byte(const MetaPacks& p, uint32_t chan, uint32_t sq, uint32_t b, uint32_t at,
                                                    uint32_t wide) {
  constexpr uint32_t kDsf = Sys::kSeqs == 12 ? 1u : 0u;
  if (at < 3u)  // the id, as k_dv_encode writes it
    return at == 0u ? (b < 2u ? 0x3Fu : 0x5Fu) : at == 1u ? (sq << 4 | chan << 3 | 7u) : (b < 2u ? b : b - 2u);
  if (b < 2u) {
    if (at >= 51u) return 0xFFu;
    const uint32_t q = at - 3u, k = q >> 3, o = q & 7u, s = 6u * b + k;  // sync block s: packet k of block b
    if (o == 0u) {
      const uint32_t fr = sq < (uint32_t)Sys::kSeqs / 2u ? 1u : 0u;
      const uint32_t mid = s == 0u || s == 6u || s == 11u ? kMetaApt<Sys> : 7u;
      return fr << 7 | mid << 4 | 0xFu;
    }
    if (o == 1u) return 0xF0u | s;
    if (o == 2u) return 0xFFu;
    return meta_packs_byte(p, s % 3u, o - 3u);
  }
  if (at >= 78u) return 0xFFu;
  const uint32_t q = at - 3u, place = q / 5u, o = q - 5u * place;
  // 0x60 .. 0x63 at places 0..3 of the first VAUX block and 9..12 of the third
  const uint32_t which = b == 2u ? place : b == 4u ? place - 9u : 4u;  // (wraps past 3 for the other places)
  if (which == 0u) return o == 0u ? kMetaPackSource : o == 3u ? (0xC0u | kDsf << 5 | kMetaStype<Sys>) : 0xFFu;
  if (which == 1u) return o == 0u ? kMetaPackControl : o == 1u ? 0x3Fu : o == 2u ? (0xC8u | (wide ? 2u : 0u)) : o == 3u ? 0xFCu : 0xFFu;
  if (which < 4u) return meta_packs_byte(p, which - 1u, o);
  return 0xFFu;
}

// rec_seconds below 0: no date (the packs 0x62 and 0x63 are FF x 5)
template <class Sys>
__global__ __launch_bounds__(kMetaWriteThreads) void k_dv_meta_write(uint8_t* __restrict__ frames, unsigned long long first_frame,
                                                                     uint32_t drop, long long rec_seconds, uint32_t wide) {
  __shared__ MetaPacks s_packs;
  constexpr uint32_t kBase = Sys::kSeqs == 12 ? 25u : 30u, kRateNum = Sys::kSeqs == 12 ? 25u : 30000u,
                     kRateDen = Sys::kSeqs == 12 ? 1u : 1001u;
  constexpr uint32_t kFrameSeqs = (uint32_t)(Sys::kChans * Sys::kSeqs);
  const uint32_t t = threadIdx.x, fr = blockIdx.x;
  uint8_t* const frame = frames + (size_t)fr * Sys::kFrameBytes;

  if (t == 0u) {
    uint32_t hmsf[4];
    meta_timecode(kBase, drop, first_frame + fr, hmsf);
    s_packs.lo[0] = kMetaPackTimecode | (drop << 6 | meta_bcd(hmsf[3])) << 8 | (0x80u | meta_bcd(hmsf[2])) << 16 |
                    (0x80u | meta_bcd(hmsf[1])) << 24;
    s_packs.hi[0] = 0xC0u | meta_bcd(hmsf[0]);
    if (rec_seconds < 0) {
      s_packs.lo[1] = s_packs.lo[2] = 0xFFFFFFFFu;
      s_packs.hi[1] = s_packs.hi[2] = 0xFFu;
    } else {
      uint32_t c[6];  // (the sum stays below 2^32: kMetaLastSecond + 65535 frames)
      meta_civil((uint32_t)((unsigned long long)rec_seconds + fr * kRateDen / kRateNum), c);
      s_packs.lo[1] = kMetaPackDate | 0xFFu << 8 | (0xC0u | meta_bcd(c[2])) << 16 | (0xE0u | meta_bcd(c[1])) << 24;
      s_packs.hi[1] = meta_bcd(c[0] % 100u);
      s_packs.lo[2] = kMetaPackTime | 0xFFu << 8 | (0x80u | meta_bcd(c[5])) << 16 | (0x80u | meta_bcd(c[4])) << 24;
      s_packs.hi[2] = 0xC0u | meta_bcd(c[3]);
    }
  }
  __syncthreads();
  const MetaPacks& p = s_packs;  // (read where they lie: a copy indexed by the pack's number would be promoted to LDS per thread)

  for (uint32_t item = t; item < kFrameSeqs * 5u * 20u; item += kMetaWriteThreads) {
    const uint32_t blk = item / 20u, w = item - 20u * blk, fs = blk / 5u, b = blk - 5u * fs;
    const uint32_t chan = fs / (uint32_t)Sys::kSeqs, sq = fs - chan * (uint32_t)Sys::kSeqs;
    uint32_t val = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) val |= meta_block_byte<Sys>(p, chan, sq, b, 4u * w + k, wide) << (8u * k);
    *(uint32_t*)(frame + ((fs * 150u + 1u + b) * 80u + 4u * w)) = val;
  }
}

}  // namespace midv
