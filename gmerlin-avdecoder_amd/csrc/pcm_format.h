// pcm_format.h — the PCM family of lib/audio_pcm.c (include/mi_pcm.h states the rules and cites upstream): the codec
// table, the transform of one 16-byte piece of the output as integer operations on the bytes of the packet, the two G.711
// tables computed at compile time from their closed forms, the classifiers of the float readers on the raw bit patterns
// (no floating-point instruction anywhere), and codec_of, payload_of and layout_of.  Plain C++ that g++ compiles too: what
// k_pcm_decode runs on the device is what decode_host runs for tests/harness/pcm_format_san.cpp and the CPU tests.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define MI_PCM_HD __host__ __device__
#else
#define MI_PCM_HD
#endif

namespace mipcm {

// the order of include/mi_pcm.h's enum (mi_pcm.hip asserts it)
enum Codec : int {
  kCopy8 = 0, kCopy16, kSwap16, kS24le, kS24be, kLpcm24, kLpcm24Mono, kLpcm20, kLpcm20Mono, kCopy32, kSwap32,
  kF32le, kF32be, kF64le, kF64be, kUlaw, kAlaw, kCodecs
};
enum Label : int { kU8 = 0, kS8, kU16, kS16, kS32, kFloat, kDouble };  // upstream's sample_format
constexpr int kFrameSamples = 1024;                                    // FRAME_SAMPLES (P:32)
constexpr int kMaxChannels = 128;

// ---- the codec table ----
// A GROUP is what one turn of upstream's loop takes and gives; a PIECE is 16 bytes of the output, a whole number of groups
// for every codec, and piece_in bytes of the packet.
struct Group {
  const char* name;
  uint32_t in_bytes, out_bytes, samples;  // of a group
  uint32_t piece_in;                      // packet bytes behind 16 output bytes: in_bytes * 16 / out_bytes
  bool lpcm, mono;                        // counts frames and writes groups differently (P:195-326); takes one channel only
};
constexpr Group kGroups[kCodecs] = {
    {"COPY8", 1, 1, 1, 16, false, false},      {"COPY16", 2, 2, 1, 16, false, false},  {"SWAP16", 2, 2, 1, 16, false, false},
    {"S24LE", 3, 4, 1, 12, false, false},      {"S24BE", 3, 4, 1, 12, false, false},   {"LPCM24", 12, 16, 4, 12, true, false},
    {"LPCM24_MONO", 6, 8, 2, 12, true, true},  {"LPCM20", 10, 16, 4, 10, true, false}, {"LPCM20_MONO", 5, 8, 2, 10, true, true},
    {"COPY32", 4, 4, 1, 16, false, false},     {"SWAP32", 4, 4, 1, 16, false, false},  {"F32LE", 4, 4, 1, 16, false, false},
    {"F32BE", 4, 4, 1, 16, false, false},      {"F64LE", 8, 8, 1, 16, false, false},   {"F64BE", 8, 8, 1, 16, false, false},
    {"ULAW", 1, 2, 1, 8, false, false},        {"ALAW", 1, 2, 1, 8, false, false},
};
MI_PCM_HD constexpr uint32_t sample_bytes(int codec) { return kGroups[codec].out_bytes / kGroups[codec].samples; }
MI_PCM_HD constexpr bool is_float(int codec) { return codec >= kF32le && codec <= kF64be; }

// ---- G.711 (P:650-684, 721-754): the closed forms; the tables are made from them at compile time ----
MI_PCM_HD constexpr int32_t ulaw_of(uint32_t b) {
  const uint32_t u = ~b & 0xffu;
  const int32_t t = (int32_t)((((u & 15u) << 3) + 0x84u) << ((u >> 4) & 7u));
  return (u & 0x80u) ? 0x84 - t : t - 0x84;
}
MI_PCM_HD constexpr int32_t alaw_of(uint32_t b) {
  const uint32_t a = (b ^ 0x55u) & 0xffu, seg = (a >> 4) & 7u;
  int32_t t = (int32_t)((a & 15u) << 4);
  t = seg == 0 ? t + 8 : (t + 0x108) << (seg == 1 ? 0 : seg - 1);
  return (a & 0x80u) ? t : -t;
}
struct Table {
  int16_t v[256];
};
template <class F>
constexpr Table make_table(F f) {
  Table t{};
  for (uint32_t b = 0; b < 256; b++) t.v[b] = (int16_t)f(b);
  return t;
}
constexpr Table kUlawTable = make_table(ulaw_of), kAlawTable = make_table(alaw_of);
static_assert(kUlawTable.v[0] == -32124 && kUlawTable.v[0x7f] == 0 && kUlawTable.v[0x80] == 32124 && kUlawTable.v[0xff] == 0, "P:651, 666, 668, 683");
static_assert(kAlawTable.v[0] == -5504 && kAlawTable.v[0x55] == -8 && kAlawTable.v[0x80] == 5504 && kAlawTable.v[0xd5] == 8, "P:722, 732, 738, 748");

// ---- the float readers on bit patterns (P:399-520) ----
enum FloatClass : int { kZero = 0, kDenormal, kInside, kOutside };
// b is the sample as a native word.  Zero: both signs read as +0.0 (P:408-409).  Denormal: exponent field 0 is taken as
// exponent 0 (P:412) and the hidden bit is set anyway (P:411): +-(1 + m / 2^23).  Inside: 1 << |e| is defined, |e| <= 30,
// and every step is exact: the IEEE value.  Outside: the shift of P:419-422 is undefined.
MI_PCM_HD constexpr int classify32(uint32_t b) {
  const uint32_t e = (b >> 23) & 0xffu;
  if (e == 0) return (b & 0x7fffffu) ? kDenormal : kZero;
  return e >= 97u && e <= 157u ? kInside : kOutside;
}
MI_PCM_HD constexpr uint32_t read32(uint32_t b) {
  const uint32_t e = (b >> 23) & 0xffu, m = b & 0x7fffffu;
  return e ? b : m ? ((b & 0x80000000u) | 0x3f800000u | m) : 0u;
}
// the double readers have no arm for exponent field 0 (P:469-474): a denormal has e = -1023 and is outside
MI_PCM_HD constexpr int classify64(uint32_t hi, uint32_t lo) {
  const uint32_t e = (hi >> 20) & 0x7ffu;
  if (e == 0 && (hi & 0xfffffu) == 0 && lo == 0) return kZero;
  return e >= 993u && e <= 1053u ? kInside : kOutside;
}
MI_PCM_HD constexpr bool zero64(uint32_t hi, uint32_t lo) { return (hi & 0x7fffffffu) == 0 && lo == 0; }

// ---- the transform of one piece ----
// g(k) is byte k of the piece's piece_in packet bytes, o the 16 output bytes as four native (little-endian) words.
// Returns how many of the piece's samples lie outside the float domain.
template <int C, class Get>
MI_PCM_HD inline uint32_t piece(Get g, uint32_t o[4]) {
  uint32_t outside = 0;
  if constexpr (C == kCopy8 || C == kCopy16 || C == kCopy32) {  // P:51-69, 71-91, 329-347
    for (int i = 0; i < 4; i++) o[i] = g(4 * i) | g(4 * i + 1) << 8 | g(4 * i + 2) << 16 | g(4 * i + 3) << 24;
  } else if constexpr (C == kSwap16) {  // P:93-124
    for (int i = 0; i < 4; i++) o[i] = g(4 * i + 1) | g(4 * i) << 8 | g(4 * i + 3) << 16 | g(4 * i + 2) << 24;
  } else if constexpr (C == kSwap32) {  // P:351-383
    for (int i = 0; i < 4; i++) o[i] = g(4 * i + 3) | g(4 * i + 2) << 8 | g(4 * i + 1) << 16 | g(4 * i) << 24;
  } else if constexpr (C == kS24le) {  // P:126-159
    for (int i = 0; i < 4; i++) o[i] = g(3 * i) << 8 | g(3 * i + 1) << 16 | g(3 * i + 2) << 24;
  } else if constexpr (C == kS24be) {  // P:161-193
    for (int i = 0; i < 4; i++) o[i] = g(3 * i + 2) << 8 | g(3 * i + 1) << 16 | g(3 * i) << 24;
  } else if constexpr (C == kLpcm24) {  // P:195-227
    for (int k = 0; k < 4; k++) o[k] = g(2 * k) << 24 | g(2 * k + 1) << 16 | g(8 + k) << 8;
  } else if constexpr (C == kLpcm24Mono) {  // P:229-259, two groups
    for (int h = 0; h < 2; h++)
      for (int k = 0; k < 2; k++) o[2 * h + k] = g(6 * h + 2 * k) << 24 | g(6 * h + 2 * k + 1) << 16 | g(6 * h + 4 + k) << 8;
  } else if constexpr (C == kLpcm20) {  // P:261-294
    for (int k = 0; k < 4; k++) {
      const uint32_t x = g(8 + k / 2);
      o[k] = g(2 * k) << 24 | g(2 * k + 1) << 16 | ((k & 1) ? (x & 0x0fu) << 12 : (x & 0xf0u) << 8);
    }
  } else if constexpr (C == kLpcm20Mono) {  // P:296-326, two groups
    for (int h = 0; h < 2; h++) {
      const uint32_t x = g(5 * h + 4);
      o[2 * h] = g(5 * h) << 24 | g(5 * h + 1) << 16 | (x & 0xf0u) << 8;
      o[2 * h + 1] = g(5 * h + 2) << 24 | g(5 * h + 3) << 16 | (x & 0x0fu) << 12;
    }
  } else if constexpr (C == kF32le || C == kF32be) {  // P:399-454, 524-584
    for (int i = 0; i < 4; i++) {
      const uint32_t b = C == kF32le ? g(4 * i) | g(4 * i + 1) << 8 | g(4 * i + 2) << 16 | g(4 * i + 3) << 24
                                     : g(4 * i + 3) | g(4 * i + 2) << 8 | g(4 * i + 1) << 16 | g(4 * i) << 24;
      outside += classify32(b) == kOutside;
      o[i] = read32(b);
    }
  } else if constexpr (C == kF64le || C == kF64be) {  // P:456-520, 586-646
    for (int i = 0; i < 2; i++) {
      const int a = 8 * i;
      const uint32_t lo = C == kF64le ? g(a) | g(a + 1) << 8 | g(a + 2) << 16 | g(a + 3) << 24
                                      : g(a + 7) | g(a + 6) << 8 | g(a + 5) << 16 | g(a + 4) << 24;
      const uint32_t hi = C == kF64le ? g(a + 4) | g(a + 5) << 8 | g(a + 6) << 16 | g(a + 7) << 24
                                      : g(a + 3) | g(a + 2) << 8 | g(a + 1) << 16 | g(a) << 24;
      outside += classify64(hi, lo) == kOutside;
      const bool z = zero64(hi, lo);
      o[2 * i] = lo, o[2 * i + 1] = z ? 0u : hi;
    }
  } else if constexpr (C == kUlaw) {  // P:686-715
    for (int i = 0; i < 4; i++) o[i] = ((uint32_t)ulaw_of(g(2 * i)) & 0xffffu) | (uint32_t)ulaw_of(g(2 * i + 1)) << 16;
  } else {  // kAlaw, P:756-785
    static_assert(C == kAlaw, "a codec of the table");
    for (int i = 0; i < 4; i++) o[i] = ((uint32_t)alaw_of(g(2 * i)) & 0xffffu) | (uint32_t)alaw_of(g(2 * i + 1)) << 16;
  }
  return outside;
}

// f(std::integral_constant-like tag) for the codec; false for none of the table
template <int C>
struct CodecTag {
  static constexpr int value = C;
};
template <class F>
inline bool dispatch(int codec, F f) {
  switch (codec) {
    case kCopy8: f(CodecTag<kCopy8>()); return true;
    case kCopy16: f(CodecTag<kCopy16>()); return true;
    case kSwap16: f(CodecTag<kSwap16>()); return true;
    case kS24le: f(CodecTag<kS24le>()); return true;
    case kS24be: f(CodecTag<kS24be>()); return true;
    case kLpcm24: f(CodecTag<kLpcm24>()); return true;
    case kLpcm24Mono: f(CodecTag<kLpcm24Mono>()); return true;
    case kLpcm20: f(CodecTag<kLpcm20>()); return true;
    case kLpcm20Mono: f(CodecTag<kLpcm20Mono>()); return true;
    case kCopy32: f(CodecTag<kCopy32>()); return true;
    case kSwap32: f(CodecTag<kSwap32>()); return true;
    case kF32le: f(CodecTag<kF32le>()); return true;
    case kF32be: f(CodecTag<kF32be>()); return true;
    case kF64le: f(CodecTag<kF64le>()); return true;
    case kF64be: f(CodecTag<kF64be>()); return true;
    case kUlaw: f(CodecTag<kUlaw>()); return true;
    case kAlaw: f(CodecTag<kAlaw>()); return true;
    default: return false;
  }
}

// ---- get_packet's clamp (P:800-804) ----
MI_PCM_HD constexpr int64_t payload_of(int64_t len, int64_t duration, int64_t block_align) {
  return duration > 0 && duration * block_align < len ? duration * block_align : len;
}

// ---- what the chunk loop of decode_frame_pcm makes of len bytes, in closed form ----
// frames: the sample frames F upstream reports over all chunks.  written: the samples its loops write (whole groups only,
// P:213, 247, 280, 314).  consumed: the bytes it takes.  out_bytes: F * ch * size, what this library writes.  valid_in: the
// bytes its loops read, written / samples * in_bytes: the packet bytes behind the samples that are not zeros.
struct Layout {
  uint64_t frames, written, consumed, out_bytes, valid_in;
};
MI_PCM_HD constexpr Layout layout_of(int codec, uint32_t ch, uint64_t len) {
  const Group& g = kGroups[codec];
  Layout l{};
  if (!g.lpcm) {
    l.frames = len / ((uint64_t)g.in_bytes * ch);
    l.written = l.frames * ch;
    l.consumed = l.written * g.in_bytes;
  } else if (g.in_bytes == 12 || g.in_bytes == 6) {  // LPCM24: 3 bytes a sample (P:203, 237)
    l.frames = len / (3u * (uint64_t)ch);
    l.consumed = 3u * l.frames * ch;
    l.written = l.frames * ch / g.samples * g.samples;
  } else {  // LPCM20: 5 bytes two samples (P:270, 275, 304, 309)
    l.frames = 2u * len / (5u * (uint64_t)ch);
    l.consumed = 5u * l.frames * ch / 2u;
    l.written = l.frames * ch / g.samples * g.samples;
  }
  l.out_bytes = l.frames * ch * sample_bytes(codec);
  l.valid_in = l.written / g.samples * g.in_bytes;
  return l;
}

// ---- one piece of a packet from memory: bytes at and behind valid_in read as 0 and are never touched ----
template <int C>
MI_PCM_HD inline uint32_t piece_at(const uint8_t* in, uint64_t valid_in, uint64_t q, uint32_t o[4]) {
  constexpr uint32_t kIn = kGroups[C].piece_in;
  const uint64_t at = q * kIn;
  uint32_t v[4] = {0, 0, 0, 0};
  for (uint32_t k = 0; k < kIn; k++)
    if (at + k < valid_in) v[k >> 2] |= (uint32_t)in[at + k] << (8 * (k & 3));
  return piece<C>([&](int k) { return (v[k >> 2] >> (8 * (k & 3))) & 0xffu; }, o);
}

// the whole packet on the host, piece by piece: out takes layout_of().out_bytes, *outside the count
inline bool decode_host(int codec, uint32_t ch, const uint8_t* in, uint64_t len, uint8_t* out, uint32_t* outside) {
  if (codec < 0 || codec >= kCodecs || ch < 1 || ch > (uint32_t)kMaxChannels || (kGroups[codec].mono && ch != 1)) return false;
  const Layout l = layout_of(codec, ch, len);
  uint32_t count = 0;
  dispatch(codec, [&](auto tag) {
    for (uint64_t q = 0; 16 * q < l.out_bytes; q++) {
      uint32_t o[4];
      count += piece_at<decltype(tag)::value>(in, l.valid_in, q, o);
      const uint64_t left = l.out_bytes - 16 * q;
      memcpy(out + 16 * q, o, left < 16 ? (size_t)left : 16);
    }
  });
  if (outside) *outside = count;
  return true;
}

// ---- init_pcm (P:810-1236), arm by arm ----
struct Format {
  int codec, label, block_align, sample_bytes;
};
constexpr uint32_t fourcc(char a, char b, char c, char d) {  // BGAV_MK_FOURCC; a WAV id is its own fourcc
  return (uint32_t)(uint8_t)a << 24 | (uint32_t)(uint8_t)b << 16 | (uint32_t)(uint8_t)c << 8 | (uint32_t)(uint8_t)d;
}
constexpr int kEndianLittle = 2;  // BGAV_ENDIANESS_LITTLE; anything else takes the big-endian arm (P:992, 1005, 1052, 1065)

// false where upstream returns 0 and where it goes on with a NULL decode_func
inline bool codec_of(uint32_t fcc, int bits, int ch, int endianess, const uint8_t* header, int header_len, Format* out) {
  int codec = -1, label = kS32, align = 0;
  const bool little = endianess == kEndianLittle;
  switch (fcc) {
    case fourcc('t', 'w', 'o', 's'):
    case fourcc('a', 'i', 'f', 'f'):  // P:823-864
      if (bits <= 8) codec = kCopy8, label = kS8;
      else if (bits <= 16) codec = kSwap16, label = kS16;
      else if (bits <= 24) codec = kS24be;
      else if (bits <= 32) codec = kSwap32;
      else return false;  // P:857-863
      break;
    case 0x01:
    case fourcc('P', 'C', 'M', ' '):  // P:866-904
      if (bits <= 8) codec = kCopy8, label = kU8;
      else if (bits <= 16) codec = kCopy16, label = fcc == 0x01 ? kS16 : kU16;
      else if (bits <= 24) codec = kS24le;
      else if (bits <= 32) codec = kCopy32;
      else return false;  // no else arm upstream: decode_func stays NULL
      break;
    case fourcc('r', 'a', 'w', ' '):
    case fourcc('s', 'o', 'w', 't'):
    case fourcc('R', 'A', 'W', 'A'):  // P:905-947
      if (bits == 8) codec = kCopy8, label = fcc == fourcc('s', 'o', 'w', 't') ? kS8 : kU8;
      else if (bits == 16) codec = kCopy16, label = kS16;
      else if (bits == 24) codec = kS24le;
      else if (bits == 32) codec = kCopy32;
      else return false;  // P:941-945
      break;
    case fourcc('L', 'P', 'C', 'M'):  // P:948-989
      if (bits == 16) codec = kSwap16, label = kS16;
      else if (bits == 20) codec = ch == 1 ? kLpcm20Mono : kLpcm20;
      else if (bits == 24) codec = ch == 1 ? kLpcm24Mono : kLpcm24;
      else return false;  // P:981-985
      break;
    case fourcc('i', 'n', '2', '4'):  // P:991-1003
      codec = little ? kS24le : kS24be, align = 3 * ch;
      break;
    case fourcc('i', 'n', '3', '2'):  // P:1004-1027
      codec = little ? kCopy32 : kSwap32, align = 4 * ch;
      break;
    case 0x03:  // P:1029-1050
      if (bits == 32) codec = kF32le, label = kFloat;
      else if (bits == 64) codec = kF64le, label = kDouble;
      else return false;  // P:1046-1047
      break;
    case fourcc('f', 'l', '3', '2'):  // P:1051-1063
      codec = little ? kF32le : kF32be, label = kFloat, align = 4 * ch;
      break;
    case fourcc('f', 'l', '6', '4'):  // P:1064-1079
      codec = little ? kF64le : kF64be, label = kDouble, align = 8 * ch;
      break;
    case fourcc('u', 'l', 'a', 'w'):
    case fourcc('U', 'L', 'A', 'W'):
    case 0x07:  // P:1080-1088
      codec = kUlaw, label = kS16, align = ch;
      break;
    case fourcc('a', 'l', 'a', 'w'):
    case fourcc('A', 'L', 'A', 'W'):
    case 0x06:  // P:1089-1097
      codec = kAlaw, label = kS16, align = ch;
      break;
    case fourcc('l', 'p', 'c', 'm'): {  // P:1098-1217
      if (!header || header_len < 4) return false;  // P:1100-1106
      uint32_t flags;
      memcpy(&flags, header, 4);  // formatSpecificFlags in native byte order (P:1107)
      const bool big = flags & 2u;  // kAudioFormatFlagIsBigEndian
      if (flags & 1u) {             // kAudioFormatFlagIsFloat
        if (bits == 32) codec = big ? kF32be : kF32le, label = kFloat, align = 4 * ch;
        else if (bits == 64) codec = big ? kF64be : kF64le, label = kDouble, align = 8 * ch;
        else return false;  // the switch of P:1120-1153 lists no other depth: decode_func stays NULL
      } else {
        if (bits == 16) codec = big ? kSwap16 : kCopy16, label = kS16, align = 2 * ch;
        else if (bits == 24) codec = big ? kS24be : kS24le, align = 3 * ch;
        else if (bits == 32) codec = big ? kSwap32 : kCopy32, align = 4 * ch;
        else return false;  // P:1157-1215 likewise
      }
      break;
    }
    default: return false;  // P:1218-1221
  }
  if (!align) align = ch * ((bits + 7) / 8);  // P:1231-1233
  out->codec = codec, out->label = label, out->block_align = align, out->sample_bytes = (int)sample_bytes(codec);
  return true;
}

}  // namespace mipcm
