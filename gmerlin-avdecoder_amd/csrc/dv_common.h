// dv_common.h — what the host side and the gfx950 kernels of the DV decoder share: the constant tables and the
// five systems' frame and picture layouts (25 Mbit/s: 525/60 4:1:1, 625/50 4:2:0, 625/50 4:1:1 "DVCPRO"; 50 Mbit/s: both
// line systems in 4:2:2).
#pragma once
#include <stdint.h>

namespace midv {

// A code word of the variable-length code as the kernels see it:
//   bits 0..4   total length in bits, sign bit included
//   bits 5..11  how far the scan position moves: run + 1; 64 for "end of block" (past the last coefficient)
//   bits 12..19 amplitude (the sign is the word's last bit)
constexpr uint32_t vlc_entry(uint32_t len, uint32_t adv, uint32_t amp) { return len | (adv << 5) | (amp << 12); }

// One reconstruction table entry per (transform mode, scan position):
//   bits 16..31 multiplier with 14 fractional bits (aan(h) aan(v) / (w(h) w(v)))
//   bits 8..9   area of the scan position (picks the quantiser shift)
//   bits 0..7   byte offset of the coefficient in a lane's scratch
struct Tables {
  uint32_t lut9[512];   // by the next 9 bits: words of up to 9 bits (+ sign)
  uint32_t lut2[64];    // words that begin 11111 and go on with 0: by the 6 bits behind that (lengths 10..12)
  uint32_t tab[2][64];  // [mode][scan position]
  uint32_t shift4[24];  // [quantisation number + class offset]: four 4-bit shifts (area 0 in the low nibble), the
                        // "+ 1" of the reconstruction included; class 3 adds one more
};

constexpr int kFrameBytes = 120000, kW = 720, kH = 480, kCW = 180, kPicBytes = kW * kH * 3 / 2;
constexpr int kSegments = 270;  // video segments per frame: 10 DIF sequences of 27

#if defined(__HIP__) || defined(__HIPCC__)
#define MIDV_HD __attribute__((host, device, always_inline)) inline
#else
#define MIDV_HD inline
#endif

// ---- the 25 Mbit/s systems (include/mi_dv.h: MI_DV_SYS_*; the third, Sys625_411, is below Sys625) ----
// A DIF sequence is 150 blocks of 80 bytes in both; video block v (0..134) of a sequence is block 7 + v + v / 15, and
// five consecutive video blocks are one video segment (27 per sequence).  What differs is the number of sequences, the
// macroblock shuffle and the picture: place() maps macroblock m (0..4) of segment `slot` (0..26) of sequence `seq` to
// its position, in the units the kernel's block placement uses.  The kernel and mi_dv_mb_place both call it.

// 525/60 4:1:1: 10 sequences; 720 x 480, Cb / Cr 180 x 480.  Macroblocks are 32 x 8 pixels (four 8 x 8 luma blocks side
// by side, one chroma block each) except in column 22, where they are 16 x 16 and their chroma blocks are split in
// halves.  x in 32-pixel columns (0..22), y in 8-line rows (0..59); the shuffle the checker states too (dvo_mb_place).
// The statement is also a macro: k_dv_decode<Sys525> expands it in place.  As a call it is inlined only after the callee
// was simplified on its own, and the 525/60 kernel then compiles to other (no faster) code than it did before 625/50
// existed; expanded, its code stays what it was, instruction for instruction.  MIDV_PLACE_411 is the statement with the
// number of DIF sequences as the modulus (10 here; 12 for Sys625_411), MIDV_PLACE_525 what the 525/60 kernel expands.
#define MIDV_PLACE_411(seqs, seq, slot, m, x32, y8)                                           \
  do {                                                                                        \
    const uint32_t off_ = (m) == 0u ? 2u : (m) == 1u ? 6u : (m) == 2u ? 8u : (m) == 3u ? 0u : 4u;       \
    const uint32_t start_ = (m) == 0u ? 9u : (m) == 1u ? 4u : (m) == 2u ? 13u : (m) == 3u ? 0u : 18u;   \
    const uint32_t i_ = ((seq) + off_) % (seqs);                                              \
    const uint32_t k_ = (slot) + ((m) == 1u || (m) == 2u ? 3u : 0u);                          \
    const uint32_t k6_ = k_ / 6u, km_ = k_ - 6u * k6_;                                        \
    const uint32_t serp_ = k6_ & 1u ? 5u - km_ : km_;                                         \
    (x32) = start_ + k6_;                                                                     \
    (y8) = (x32) > 21u ? 2u * serp_ + 6u * i_ : serp_ + 6u * i_;                              \
  } while (0)
#define MIDV_PLACE_525(seq, slot, m, x32, y8) MIDV_PLACE_411(10u, seq, slot, m, x32, y8)

// What a macroblock covers of a picture: one rectangle in each plane (Y, Cb, Cr), in that plane's own pixels.  rects()
// of a system, beside its place(), gives the three for macroblock m of segment `slot` of sequence `seq`; the numbers are
// those of k_dv_decode's store section (which does not call it: dv_decode_kernels.h).  The hold pass (dv_hold_kernels.h)
// and mi_dv_mb_rects both call it.
struct Rect {
  uint32_t x, y, w, h;
};
// 4:1:1 at (x32, y8): 32 x 8 with one 8 x 8 chroma block in each plane; in column 22 16 x 16, and the chroma block's two
// 4-wide halves lie one above the other
MIDV_HD void rects_411(uint32_t x32, uint32_t y8, Rect r[3]) {
  const bool edge = x32 == 22u;
  r[0] = edge ? Rect{704u, 8u * y8, 16u, 16u} : Rect{32u * x32, 8u * y8, 32u, 8u};
  r[1] = r[2] = edge ? Rect{176u, 8u * y8, 4u, 16u} : Rect{8u * x32, 8u * y8, 8u, 8u};
}
struct Sys525 {
  static constexpr int kId = 0, kChans = 1;
  static constexpr bool k411 = true;  // 32 x 8 macroblocks, 16 x 16 with split chroma blocks in column 22
  static constexpr int kFrameBytes = 120000, kSeqs = 10, kSegments = kSeqs * 27, kPairs = kSegments / 2;
  static constexpr int kW = 720, kH = 480, kCW = 180, kCH = 480, kPicBytes = kW * kH + 2 * kCW * kCH;
  static MIDV_HD void place(uint32_t seq, uint32_t slot, uint32_t m, uint32_t& x32, uint32_t& y8) {
    MIDV_PLACE_525(seq, slot, m, x32, y8);
  }
  static MIDV_HD void rects(uint32_t seq, uint32_t slot, uint32_t m, Rect r[3]) {
    uint32_t x32, y8;
    place(seq, slot, m, x32, y8);
    rects_411(x32, y8, r);
  }
};

// 625/50 IEC 4:2:0: 12 sequences; 720 x 576, Cb / Cr 360 x 288.  Every macroblock is 16 x 16 (Y0 Y1 / Y2 Y3, then one
// 8 x 8 block of each chroma plane).  The picture is 45 x 36 macroblocks: 5 columns x 12 rows of super blocks of 9 x 3;
// super block (row (seq + {2,6,8,0,4}[m]) mod 12, column {2,1,3,0,4}[m]), inside it column slot / 3 and row slot % 3,
// upwards in odd columns.  x, y in 16-pixel units (0..44, 0..35).
struct Sys625 {
  static constexpr int kId = 1, kChans = 1;
  static constexpr bool k411 = false;
  static constexpr int kFrameBytes = 144000, kSeqs = 12, kSegments = kSeqs * 27, kPairs = kSegments / 2;
  static constexpr int kW = 720, kH = 576, kCW = 360, kCH = 288, kPicBytes = kW * kH + 2 * kCW * kCH;
  static MIDV_HD void place(uint32_t seq, uint32_t slot, uint32_t m, uint32_t& x16, uint32_t& y16) {
    const uint32_t off = m == 0u ? 2u : m == 1u ? 6u : m == 2u ? 8u : m == 3u ? 0u : 4u;
    const uint32_t col = m == 0u ? 2u : m == 1u ? 1u : m == 2u ? 3u : m == 3u ? 0u : 4u;
    const uint32_t row = (seq + off) % 12u;
    const uint32_t c = slot / 3u, r = slot - 3u * c;
    x16 = 9u * col + c;
    y16 = 3u * row + (c & 1u ? 2u - r : r);
  }
  static MIDV_HD void rects(uint32_t seq, uint32_t slot, uint32_t m, Rect r[3]) {
    uint32_t x16, y16;
    place(seq, slot, m, x16, y16);
    r[0] = Rect{16u * x16, 16u * y16, 16u, 16u};
    r[1] = r[2] = Rect{8u * x16, 8u * y16, 8u, 8u};
  }
};

// 625/50 4:1:1 ("DVCPRO" 25 Mbit/s PAL: DSF 1, VAUX stype 0, APT != 0; lib/dvframe.c:149-169; SMPTE 314M as this
// repository reads it: parity unpinned): the 625/50 frame (12 sequences, 144,000 bytes) with the 525/60 picture layout
// carried on by two sequences: 720 x 576, Cb / Cr 180 x 576.  Macroblocks, the right-edge column and the shuffle are
// 525/60's with the sequence count as the modulus: x in 32-pixel columns (0..22), y in 8-line rows (0..71).
struct Sys625_411 {
  static constexpr int kId = 3, kChans = 1;
  static constexpr bool k411 = true;
  static constexpr int kFrameBytes = 144000, kSeqs = 12, kSegments = kSeqs * 27, kPairs = kSegments / 2;
  static constexpr int kW = 720, kH = 576, kCW = 180, kCH = 576, kPicBytes = kW * kH + 2 * kCW * kCH;
  static MIDV_HD void place(uint32_t seq, uint32_t slot, uint32_t m, uint32_t& x32, uint32_t& y8) {
    MIDV_PLACE_411(12u, seq, slot, m, x32, y8);
  }
  static MIDV_HD void rects(uint32_t seq, uint32_t slot, uint32_t m, Rect r[3]) {
    uint32_t x32, y8;
    place(seq, slot, m, x32, y8);
    rects_411(x32, y8, r);
  }
};

// ---- the two 50 Mbit/s systems ("DVCPRO50", VAUX stype 4; SMPTE 314M as this repository reads it: parity unpinned) ----
// Two DIF channels back to back, each of kSeqs sequences laid out as above; the compressed macroblock is the 25 Mbit/s
// one, but its areas 1 and 3 carry no pixels (they are parsed and lend their unused bits; their coefficients are thrown
// away): area 0 is the left 8 x 8 luma block, area 2 the right one, area 4 Cr, area 5 Cb.  A macroblock is 16 pixels wide
// and 8 lines high; the picture is 45 x (kH / 8) of them, Cb / Cr 360 x kH.  place() takes `seq` as the frame's sequence
// in byte order, 0 .. 2 kSeqs - 1 (channel seq / kSeqs), and is Sys625::place with the super-block row 2 row + channel
// and rows of 8 lines: x in 16-pixel columns (0..44), y in 8-line rows (0..59 / 0..71).
template <int Id, int Seqs>
struct Sys422 {
  static constexpr int kId = Id, kChans = 2;
  static constexpr bool k411 = false;
  static constexpr int kSeqs = Seqs, kFrameBytes = kChans * kSeqs * 150 * 80, kSegments = kChans * kSeqs * 27, kPairs = kSegments / 2;
  static constexpr int kW = 720, kH = 48 * kSeqs, kCW = 360, kCH = kH, kPicBytes = kW * kH + 2 * kCW * kCH;
  static MIDV_HD void place(uint32_t seq, uint32_t slot, uint32_t m, uint32_t& x16, uint32_t& y8) {
    const uint32_t off = m == 0u ? 2u : m == 1u ? 6u : m == 2u ? 8u : m == 3u ? 0u : 4u;
    const uint32_t col = m == 0u ? 2u : m == 1u ? 1u : m == 2u ? 3u : m == 3u ? 0u : 4u;
    const uint32_t chan = seq >= (uint32_t)kSeqs ? 1u : 0u;
    const uint32_t row = (seq - chan * (uint32_t)kSeqs + off) % (uint32_t)kSeqs;
    const uint32_t c = slot / 3u, r = slot - 3u * c;
    x16 = 9u * col + c;
    y8 = 3u * (2u * row + chan) + (c & 1u ? 2u - r : r);
  }
  static MIDV_HD void rects(uint32_t seq, uint32_t slot, uint32_t m, Rect r[3]) {  // (`seq` as place() takes it)
    uint32_t x16, y8;
    place(seq, slot, m, x16, y8);
    r[0] = Rect{16u * x16, 8u * y8, 16u, 8u};
    r[1] = r[2] = Rect{8u * x16, 8u * y8, 8u, 8u};
  }
};
using Sys525_422 = Sys422<4, 10>;  // 240,000-byte frames, 720 x 480
using Sys625_422 = Sys422<5, 12>;  // 288,000-byte frames, 720 x 576
static_assert(Sys525::kFrameBytes == Sys525::kSeqs * 150 * 80 && Sys625::kFrameBytes == Sys625::kSeqs * 150 * 80, "DIF frames");
static_assert(Sys525::kPicBytes == kPicBytes && Sys525::kFrameBytes == kFrameBytes && Sys525::kSegments == kSegments, "525/60");
static_assert(Sys625::kPicBytes == 622080 && Sys625::kPairs * 2 == Sys625::kSegments, "625/50");
static_assert(Sys625_411::kFrameBytes == Sys625_411::kSeqs * 150 * 80 && Sys625_411::kFrameBytes == Sys625::kFrameBytes &&
                  Sys625_411::kSegments == 324 && Sys625_411::kPairs == 162 && Sys625_411::kPairs * 2 == Sys625_411::kSegments &&
                  Sys625_411::kPicBytes == 622080 && Sys625_411::kCW * 4 == Sys625_411::kW && Sys625_411::kCH == Sys625_411::kH,
              "625/50 4:1:1");
static_assert(Sys525_422::kFrameBytes == 240000 && Sys525_422::kH == 480 && Sys525_422::kPicBytes == 691200 &&
                  Sys525_422::kSegments == 540 && Sys525_422::kPairs == 270, "525/60 4:2:2");
static_assert(Sys625_422::kFrameBytes == 288000 && Sys625_422::kH == 576 && Sys625_422::kPicBytes == 829440 &&
                  Sys625_422::kSegments == 648 && Sys625_422::kPairs == 324, "625/50 4:2:2");

// builds the tables (dv_tables.cpp); false if the code's lengths are not a complete prefix code
bool build_tables(Tables* t);

// ---- sound (dv_audio_kernels.h) ----
// Where the samples of a frame's audio DIF blocks go, per line system (0: 525/60, 1: 625/50; the 50 Mbit/s systems have
// their line system's layout in each channel).  A stereo pair's buffer is a row of 16-bit slots, left and right
// alternating; sample n of audio block j of DIF sequence q goes to slot shuffle[q][j] + n stride, and a frame carries
// min_samples[rate] + 0..63 samples a channel (rate 0: 48 kHz, 1: 44.1 kHz, 2: 32 kHz).  What include/mi_dvframe.h's
// profiles tabulate (lib/dvframe.c:76-104), made from the rule here; tests/test_dv_audio_cpu.py holds the two together.
struct AudioTables {
  uint16_t shuffle[2][12][9];  // (525/60 has 10 sequences: its rows 10 and 11 are zero)
  uint16_t stride[2];
  uint16_t min_samples[2][3];
};
void build_audio_tables(AudioTables* t);

}  // namespace midv
