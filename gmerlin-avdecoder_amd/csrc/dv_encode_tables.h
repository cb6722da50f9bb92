// dv_encode_tables.h — the constants of the DV encoder (k_dv_encode, dv_encode_kernels.h): what tests/dvenc.py states as
// MULT_NAT / POS_NAT, as compile-time literals (tools/dv_encode_tables.py prints both spellings), and the code-word table
// the host builds from the format's code (dv_tables.cpp).
#pragma once
#include <stdint.h>

namespace midv {

// by (mode, natural position 8 r + h): the quantiser's multiplier, round(2^20 W / ratio) — the closed-form weight over the
// forward butterfly's scale at that position
constexpr uint32_t kEncMult[2][64] = {
    {8192, 5793, 5793, 6270, 7168, 8867, 11585, 21407, 5793, 4096, 4096, 4433, 5069, 6270, 8192, 15137, 5793, 4096, 4096, 4433,
     5069, 6270, 8192, 15137, 6270, 4433, 4433, 4799, 5486, 6786, 8867, 16384, 7168, 5069, 5069, 5486, 6272, 7759, 10137, 18731,
     8867, 6270, 6270, 6786, 7759, 9598, 12540, 23170, 11585, 8192, 8192, 8867, 10137, 12540, 16384, 30274, 21407, 15137, 15137,
     16384, 18731, 23170, 30274, 55938},
    {8192, 5793, 5793, 6270, 7168, 8867, 11585, 21407, 8192, 5793, 5793, 6270, 7168, 8867, 11585, 21407, 5793, 4096, 4096, 4433,
     5069, 6270, 8192, 15137, 5793, 4096, 4096, 4433, 5069, 6270, 8192, 15137, 7168, 5069, 5069, 5486, 6272, 7759, 10137, 18731,
     7168, 5069, 5069, 5486, 6272, 7759, 10137, 18731, 11585, 8192, 8192, 8867, 10137, 12540, 16384, 30274, 11585, 8192, 8192,
     8867, 10137, 12540, 16384, 30274},
};
// by (mode, natural position): its scan position
constexpr uint32_t kEncPos[2][64] = {
    {0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53, 10, 19,
     23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63},
    {0, 2, 6, 18, 20, 34, 36, 50, 1, 3, 7, 19, 21, 35, 37, 51, 4, 8, 16, 22, 32, 38, 48, 52, 5, 9, 17, 23, 33, 39, 49, 53, 10, 14,
     24, 30, 40, 46, 54, 60, 11, 15, 25, 31, 41, 47, 55, 61, 12, 26, 28, 42, 44, 56, 58, 62, 13, 27, 29, 43, 45, 57, 59, 63},
};
constexpr int kEncFrac = 20;  // fractional bits of a multiplier

// What the encoder reads at run time.  word[run][amp]: the listed code word of the pair, code | length << 16 (without the
// sign bit), 0 where the code lists none; amp 0 is the bare run of run + 1 zeros (listed for runs 0..5).  The code lists no
// pair beyond run 14 or amplitude 22.  shift4[qno + class offset]: four 4-bit quantiser shifts, area 0 in the low nibble
// (class 3 adds one to each).  eob: the end of block, in word[]'s form.
constexpr int kEncRuns = 15, kEncAmps = 23;
struct EncTables {
  uint32_t word[kEncRuns][kEncAmps];
  uint32_t shift4[22];
  uint32_t eob;
};
// builds them (dv_tables.cpp); false if the code holds a pair outside word[][]
bool build_enc_tables(EncTables* t);

}  // namespace midv
