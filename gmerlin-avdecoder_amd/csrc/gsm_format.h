// gsm_format.h — GSM 06.10 full rate as lib/audio_gsm.c drives lib/GSM610/ (include/mi_gsm.h states the rules and cites
// upstream): the one unpacker of both framings, which mi_gsm_explode runs on the host and k_gsm_decode on the device, the
// integer operations, the two tables, and the chain of one frame over a history and a sample sink the caller supplies.
// Plain C++ that g++ compiles too: tests/harness/gsm_explode_san.cpp builds it with the sanitizers and runs the chain on
// the CPU against the recorded vectors.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MI_GSM_HD __host__ __device__
#else
#define MI_GSM_HD
#endif
#if defined(__clang__)
#define MI_GSM_UNROLL _Pragma("unroll")
#else
#define MI_GSM_UNROLL
#endif

namespace migsm {

constexpr int kFrameBytes = 33, kBlockBytes = 65, kParams = 76, kFrameSamples = 160, kStateWords = 144;
constexpr int kRing = 160;  // the history of 120 samples and the 40 of the subframe being made

// ---- the unpacker (G/gsm_decode.c:40-270 and 276-376) ----
// the width of field f of a frame: LARc[8], then four times Nc, bc, Mc, xmaxc, xMc[13]
MI_GSM_HD inline int width_of(int f) {
  if (f < 8) return 6 - (f >> 1);  // 6, 6, 5, 5, 4, 4, 3, 3
  const int g = (f - 8) % 17;
  return g == 0 ? 7 : g == 3 ? 6 : g < 3 ? 2 : 3;
}

// The 76 parameters of the frame whose first field starts `skip` bits into the 33 bytes get(0) .. get(32).  The plain
// framing is most significant bit first behind the nibble of the magic (skip 4).  The Microsoft framing is least
// significant bit first: a block's first frame starts at bit 0 of byte 0, its second at bit 4 of byte 32 (upstream's
// frame_chain), so both are 33 bytes, the first from the block's byte 0 and the second from its byte 32.  Reads no
// byte but the 33.
template <class Get, class Put>
MI_GSM_HD inline void unpack(Get get, bool msb_first, int skip, Put put) {
  int pos = skip;
  for (int f = 0; f < kParams; f++) {
    const int w = width_of(f), i = pos >> 3, b = pos & 7;
    const uint32_t first = get(i), second = b + w > 8 ? get(i + 1) : 0u;  // (b + w > 8 only where i + 1 <= 32)
    const uint32_t v = msb_first ? ((first << 8 | second) >> (16 - b - w)) : ((second << 8 | first) >> b);
    put(f, (uint8_t)(v & ((1u << w) - 1u)));
    pos += w;
  }
}

// ---- G/gsm610_priv.h:84-191 ----
MI_GSM_HD inline int32_t sat16(int32_t x) { return x > 32767 ? 32767 : x < -32768 ? -32768 : x; }  // what GSM_ADD and GSM_SUB do to a sum
MI_GSM_HD inline int32_t mul16(int32_t a, int32_t b) {  // both are words
#if defined(__HIP_DEVICE_COMPILE__)
  return __mul24(a, b);
#else
  return a * b;
#endif
}
MI_GSM_HD inline int32_t mult_r(int32_t a, int32_t b) { return (mul16(a, b) + 16384) >> 15; }  // GSM_MULT_R: no saturation
MI_GSM_HD inline int32_t narrow(int32_t x) { return (int16_t)(uint16_t)(uint32_t)x; }  // an assignment to `word`

// ---- the two tables ----
// xMp by (xmaxc, xMc): G/rpe.c:244-275 and 369-402 with gsm_sub, gsm_asl, gsm_asr of G/add.c
MI_GSM_HD constexpr int32_t xmp_of(int xmaxc, int xmc) {
  int expon = 0;
  if (xmaxc > 15) expon = (xmaxc >> 3) - 1;
  int mant = xmaxc - (expon << 3);
  if (mant == 0) {
    expon = -4, mant = 7;
  } else {
    while (mant <= 7) mant = mant << 1 | 1, expon--;
    mant -= 8;
  }
  const int32_t fac = 18431 + 2048 * mant;         // gsm_FAC (G/table.c:85)
  const int temp2 = 6 - expon;                     // 0 .. 10
  const int32_t temp3 = temp2 ? 1 << (temp2 - 1) : 0;  // gsm_asl(1, -1) is gsm_asr(1, 1)
  int32_t temp = ((xmc << 1) - 7) * 4096;
  temp = (fac * temp + 16384) >> 15;
  temp = temp + temp3;  // GSM_ADD: |temp| < 28672 and temp3 <= 512
  return temp >> temp2;
}
// LARpp by (i, LARc): G/short_term.c:44-93; 0 where LARc is beyond the field's width
MI_GSM_HD constexpr int32_t larpp_of(int i, int larc) {
  constexpr int32_t B[8] = {0, 0, 2048, -2560, 94, -1792, -341, -1144}, MIC[8] = {-32, -32, -16, -16, -8, -8, -4, -4},
                    INVA[8] = {13107, 13107, 13107, 13107, 19223, 17476, 31454, 29708};
  if (larc >= -2 * MIC[i]) return 0;
  int32_t t = (larc + MIC[i]) * 1024;
  t = t - B[i] * 2;
  t = t > 32767 ? 32767 : t < -32768 ? -32768 : t;
  t = (INVA[i] * t + 16384) >> 15;
  t = t + t;
  return t > 32767 ? 32767 : t < -32768 ? -32768 : t;
}
struct Tables {
  int16_t xmp[64 * 8], larpp[8 * 64];
};
constexpr Tables make_tables() {
  Tables t{};
  for (int x = 0; x < 64; x++)
    for (int c = 0; c < 8; c++) t.xmp[x * 8 + c] = (int16_t)xmp_of(x, c);
  for (int i = 0; i < 8; i++)
    for (int c = 0; c < 64; c++) t.larpp[i * 64 + c] = (int16_t)larpp_of(i, c);
  return t;
}
// (a function's static: usable in host and in device code alike)
MI_GSM_HD inline const Tables& tables() {
  static constexpr Tables t = make_tables();
  return t;
}

// ---- what survives a frame, beside the history; all of them words ----
struct Regs {
  int32_t v[9], msr, nrp, prev[8];
  int32_t pos;  // where in the ring the next subframe goes: a multiple of 40
};

// G/short_term.c:161-195 for one value.  The result is never -32768 (tests/test_gsmraw_cpu.py tries all 65,536), which
// is why the lattice below has no arm for -32768 times -32768.
MI_GSM_HD inline int32_t larp_to_rp(int32_t x) {
  const int32_t t = x < 0 ? (x == -32768 ? 32767 : -x) : x;
  const int32_t r = t < 11059 ? t << 1 : t < 20070 ? t + 11059 : sat16((t >> 2) + 26112);
  return x < 0 ? -r : r;
}

// The reflection coefficients of one of the four stretches of a frame (G/short_term.c:111-157): 0 is k = 0..12, 1 is
// 13..26, 2 is 27..39, 3 is 40..159.
MI_GSM_HD inline void make_rrp(int which, const int32_t* prev, const int32_t* cur, int32_t* rrp) {
  MI_GSM_UNROLL
  for (int i = 0; i < 8; i++) {
    const int32_t a = prev[i], b = cur[i];
    int32_t t;
    if (which == 0) t = sat16(sat16((a >> 2) + (b >> 2)) + (a >> 1));
    else if (which == 1) t = sat16((a >> 1) + (b >> 1));
    else if (which == 2) t = sat16(sat16((a >> 2) + (b >> 2)) + (b >> 1));
    else t = b;
    rrp[i] = narrow(larp_to_rp(t));
  }
}

// One good frame (G/decode.c:56-83): par are its 76 parameters, T the tables; ring.get(s) and ring.set(s, x) reach
// sample s of the ring of kRing words; out(at, s8) takes samples at .. at + 7 of the frame's 160.  Each subframe goes
// through the inverse quantiser and the long-term filter (G/long_term.c:924-967) into the ring and from there, sample by
// sample, through the lattice (G/short_term.c:280-318) and the de-emphasis (G/decode.c:40-54): the lattice and the
// de-emphasis look at nothing the later subframes change.
template <class Par, class Tab, class Ring, class Out>
MI_GSM_HD inline void decode_frame(Regs& r, Par par, Tab T, Ring ring, Out out) {
  int32_t cur[8], rrp[8];
  MI_GSM_UNROLL
  for (int i = 0; i < 8; i++) cur[i] = T.larpp(i * 64 + (int)par(i));
  MI_GSM_UNROLL
  for (int i = 0; i < 8; i++) rrp[i] = 0;
  for (int j = 0; j < 4; j++) {
    const int q = 8 + 17 * j;
    const int32_t Nc = par(q), bc = par(q + 1), Mc = par(q + 2), xmaxc = par(q + 3);
    const int32_t Nr = (Nc < 40 || Nc > 120) ? r.nrp : Nc;
    r.nrp = Nr;
    const int32_t brp = bc == 0 ? 3277 : bc == 1 ? 11469 : bc == 2 ? 21299 : 32767;  // gsm_QLB (G/table.c:67)
    const int32_t pos = r.pos;
    for (int k = 0; k < 40; k++) ring.set(pos + k, 0);  // G/rpe.c:406-441
    for (int i = 0; i < 13; i++) ring.set(pos + Mc + 3 * i, T.xmp(xmaxc * 8 + (int)par(q + 4 + i)));
    int32_t from = pos - Nr;
    if (from < 0) from += kRing;
    for (int k8 = 0; k8 < 5; k8++) {
      int32_t s8[8];
      MI_GSM_UNROLL
      for (int u = 0; u < 8; u++) {
        const int k = k8 * 8 + u;
        if (j == 0 ? (k == 0 || k == 13 || k == 27) : (j == 1 && k == 0))
          make_rrp(j ? 3 : k == 0 ? 0 : k == 13 ? 1 : 2, r.prev, cur, rrp);
        int32_t at = from + k;
        if (at >= kRing) at -= kRing;
        int32_t sri = sat16(ring.get(pos + k) + mult_r(brp, ring.get(at)));
        ring.set(pos + k, sri);
        MI_GSM_UNROLL
        for (int i = 7; i >= 0; i--) {
          sri = sat16(sri - mult_r(rrp[i], r.v[i]));
          r.v[i + 1] = sat16(r.v[i] + mult_r(rrp[i], sri));
        }
        r.v[0] = sri;
        r.msr = sat16(sri + mult_r(r.msr, 28180));
        s8[u] = narrow(sat16(r.msr + r.msr) & 0xFFF8);
      }
      out(j * 40 + k8 * 8, s8);
    }
    r.pos = pos + 40 == kRing ? 0 : pos + 40;
  }
  MI_GSM_UNROLL
  for (int i = 0; i < 8; i++) r.prev[i] = cur[i];
}

}  // namespace migsm
