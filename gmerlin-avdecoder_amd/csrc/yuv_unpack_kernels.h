// yuv_unpack_kernels.h — the uncompressed QuickTime YUV family (lib/video_yuv.c) on gfx950: the format table, which host
// and device code share, the plane mover (2vuy, VYUY, yv12, YV12, YVU9) and k_yuv_unpack<Codec> (yuv2, yuv4, v308, v408,
// v410, v210).  include/mi_yuv.h states the formats with the upstream lines; DESIGN.md section 12 the kernel shapes.
//
// Addressing: a packet and a picture are found as a 64-bit wave-uniform base (blockIdx.y * stride) plus a 32-bit lane
// offset inside the frame; the host layer refuses packets and pictures of 2^31 bytes or more.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace miyuv {

enum Codec : int { kYuv2 = 0, k2vuy, kYv12Lower, kYv12Upper, kVyuy, kYvu9, kV308, kV408, kV410, kV210, kYuv4, kCodecs };

// ---- the format table ----
struct Format {
  const char* name;
  uint32_t fourcc;          // BGAV_MK_FOURCC
  uint32_t w_mult, h_mult;  // the sizes upstream's loops cover whole: multiples of these
  bool moves;               // the plane mover's (upstream hands the packet's planes on); else k_yuv_unpack<Codec>
};
constexpr uint32_t fourcc(char a, char b, char c, char d) {
  return (uint32_t)(uint8_t)a << 24 | (uint32_t)(uint8_t)b << 16 | (uint32_t)(uint8_t)c << 8 | (uint32_t)(uint8_t)d;
}
constexpr Format kFormats[kCodecs] = {
    {"yuv2", fourcc('y', 'u', 'v', '2'), 2, 1, false}, {"2vuy", fourcc('2', 'v', 'u', 'y'), 2, 1, true},
    {"yv12", fourcc('y', 'v', '1', '2'), 2, 2, true},  {"YV12", fourcc('Y', 'V', '1', '2'), 2, 2, true},
    {"VYUY", fourcc('V', 'Y', 'U', 'Y'), 2, 1, true},  {"YVU9", fourcc('Y', 'V', 'U', '9'), 4, 4, true},
    {"v308", fourcc('v', '3', '0', '8'), 1, 1, false}, {"v408", fourcc('v', '4', '0', '8'), 1, 1, false},
    {"v410", fourcc('v', '4', '1', '0'), 1, 1, false}, {"v210", fourcc('v', '2', '1', '0'), 2, 1, false},
    {"yuv4", fourcc('y', 'u', 'v', '4'), 2, 2, false},
};

constexpr uint64_t pad(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }  // PAD, lib/video_yuv.c:32

// what a codec makes of a size it accepts.  Picture plane p is w[p] x h[p] samples of bps[p] bytes, tightly packed behind
// plane p - 1; it comes from the packet's bytes at src_off[p], rows src_stride[p] apart (the unpacked codecs read one
// packed plane: src_off 0, src_stride[0])
struct Shape {
  uint64_t packet_bytes, picture_bytes;
  uint32_t planes;
  uint32_t w[3], h[3], bps[3];
  uint64_t src_off[3], src_stride[3], dst_off[3];
};
constexpr Shape shape_of(int codec, uint64_t w, uint64_t h) {
  Shape s{};
  auto planes = [&](uint32_t n, uint64_t cw, uint64_t ch, uint32_t bps) {
    s.planes = n;
    for (uint32_t p = 0; p < n; p++) {
      s.w[p] = (uint32_t)(p ? cw : w), s.h[p] = (uint32_t)(p ? ch : h), s.bps[p] = bps;
      s.dst_off[p] = s.picture_bytes;
      s.picture_bytes += (uint64_t)s.w[p] * s.h[p] * bps;
    }
  };
  switch (codec) {
    case kYuv2:  // :96 PAD(2w, 4) = 2w for even w
      planes(3, w / 2, h, 1), s.src_stride[0] = 2 * w, s.packet_bytes = 2 * w * h;
      break;
    case k2vuy:
    case kVyuy:  // :209, :239
      planes(1, 0, 0, 2), s.src_stride[0] = 2 * w, s.packet_bytes = 2 * w * h;
      break;
    case kYv12Lower:
    case kYv12Upper: {  // :253-255, :285-287: strides w, w/2; 'YV12' holds V before U
      planes(3, w / 2, h / 2, 1);
      const uint64_t c = (w / 2) * (h / 2), first = w * h, second = w * h + c;
      s.src_stride[0] = w, s.src_stride[1] = s.src_stride[2] = w / 2;
      s.src_off[1] = codec == kYv12Lower ? first : second, s.src_off[2] = codec == kYv12Lower ? second : first;
      s.packet_bytes = w * h + 2 * c;
      break;
    }
    case kYvu9: {  // :320-322, :336-338: strides PAD(w, 8) and a quarter of it; V before U
      planes(3, w / 4, h / 4, 1);
      const uint64_t st = pad(w, 8), c = (st / 4) * (h / 4);
      s.src_stride[0] = st, s.src_stride[1] = s.src_stride[2] = st / 4;
      s.src_off[2] = st * h, s.src_off[1] = st * h + c;
      s.packet_bytes = st * h + 2 * c;
      break;
    }
    case kV308:  // :392
      planes(3, w, h, 1), s.src_stride[0] = 3 * w, s.packet_bytes = 3 * w * h;
      break;
    case kV408:  // :178
      planes(1, 0, 0, 4), s.src_stride[0] = 4 * w, s.packet_bytes = 4 * w * h;
      break;
    case kV410:  // :446
      planes(3, w, h, 2), s.src_stride[0] = 4 * w, s.packet_bytes = 4 * w * h;
      break;
    case kV210:  // :536
      planes(3, w / 2, h, 2), s.src_stride[0] = pad(w, 48) * 8 / 3, s.packet_bytes = s.src_stride[0] * h;
      break;
    case kYuv4:  // :598, h/2 rows
      planes(3, w / 2, h / 2, 1), s.src_stride[0] = 3 * w, s.packet_bytes = 3 * w * (h / 2);
      break;
    default:
      break;
  }
  return s;
}

// v408's alpha (the table at :104-138 as a formula; include/mi_yuv.h)
__host__ __device__ constexpr uint32_t alpha_v408(uint32_t x) {
  const uint32_t v = x < 2 ? 0u : ((x - 2u) * 255u + 43u) / 219u;
  return v > 255u ? 255u : v;
}

// ---- 16 bytes of a frame at a 32-bit offset, by the widest access the offset's alignment allows (the frame's base is
// 16-byte aligned).  The alignment is the same in every lane of a wave wherever lanes step by multiples of 16 bytes ----
__device__ __forceinline__ uint4 get16(const uint8_t* __restrict__ p, uint32_t off) {
  if ((off & 15u) == 0) return *(const uint4*)(p + off);
  uint32_t v[4];
  if ((off & 3u) == 0) {
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = *(const uint32_t*)(p + off + 4 * i);
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++)
      v[i] = (uint32_t)p[off + 4 * i] | (uint32_t)p[off + 4 * i + 1] << 8 | (uint32_t)p[off + 4 * i + 2] << 16 |
             (uint32_t)p[off + 4 * i + 3] << 24;
  }
  return make_uint4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void put16(uint8_t* __restrict__ p, uint32_t off, const uint32_t* v) {
  if ((off & 15u) == 0) {
    *(uint4*)(p + off) = make_uint4(v[0], v[1], v[2], v[3]);
  } else if ((off & 3u) == 0) {
#pragma unroll
    for (int i = 0; i < 4; i++) *(uint32_t*)(p + off + 4 * i) = v[i];
  } else {
#pragma unroll
    for (int i = 0; i < 16; i++) p[off + i] = (uint8_t)(v[i >> 2] >> (8 * (i & 3)));
  }
}
__device__ __forceinline__ void load16s(uint32_t* v, const uint8_t* __restrict__ p, uint32_t off, int n16) {
#pragma unroll
  for (int i = 0; i < n16; i++) {
    const uint4 q = get16(p, off + 16u * i);
    v[4 * i] = q.x, v[4 * i + 1] = q.y, v[4 * i + 2] = q.z, v[4 * i + 3] = q.w;
  }
}
__device__ __forceinline__ uint32_t byte_at(const uint32_t* v, int i) { return (v[i >> 2] >> (8 * (i & 3))) & 0xffu; }
// four bytes of v, at i, i + step, ..., as one word
__device__ __forceinline__ uint32_t gather4(const uint32_t* v, int i, int step) {
  return byte_at(v, i) | byte_at(v, i + step) << 8 | byte_at(v, i + 2 * step) << 16 | byte_at(v, i + 3 * step) << 24;
}

// ---- the plane mover: strided planes of the packet -> tight planes of the picture, in the picture's order ----
// One item is one 16-byte aligned piece of the picture that holds bytes of a plane.  A piece that lies whole inside one row
// of its plane is one 16-byte store; the pieces at a plane's ends and across its rows' ends go byte by byte and write the
// plane's own bytes only.  (A plane whose rows lie back to back in the packet is one row to this kernel: the host says so.)
struct MovePlane {
  uint32_t src_off, src_stride, row_bytes, rows, dst_off;
  uint32_t first_piece, items_before;  // the plane's first piece (dst_off / 16); the items of the planes before it
};
struct MoveGeo {
  uint32_t items, planes;
  MovePlane p[3];
};
inline MoveGeo move_geo(const Shape& s) {
  MoveGeo g{};
  g.planes = s.planes;
  for (uint32_t p = 0; p < s.planes; p++) {
    MovePlane& m = g.p[p];
    const uint32_t row_bytes = s.w[p] * s.bps[p], bytes = row_bytes * s.h[p];
    const bool tight = s.src_stride[p] == row_bytes;
    m.src_off = (uint32_t)s.src_off[p], m.src_stride = (uint32_t)s.src_stride[p], m.dst_off = (uint32_t)s.dst_off[p];
    m.row_bytes = tight ? bytes : row_bytes, m.rows = tight ? 1u : s.h[p];
    m.first_piece = m.dst_off / 16u, m.items_before = g.items;
    g.items += (m.dst_off + bytes - 1u) / 16u - m.first_piece + 1u;
  }
  return g;
}

constexpr uint32_t kThreads = 256, kMaxGridX = 4096;

__global__ __launch_bounds__(256) void k_yuv_move(const uint8_t* __restrict__ packets, uint64_t packet_stride,
                                                  uint8_t* __restrict__ pics, uint64_t pic_stride, MoveGeo g) {
  const uint8_t* __restrict__ in = packets + (uint64_t)blockIdx.y * packet_stride;
  uint8_t* __restrict__ out = pics + (uint64_t)blockIdx.y * pic_stride;
  for (uint32_t item = blockIdx.x * kThreads + threadIdx.x; item < g.items; item += gridDim.x * kThreads) {
    const uint32_t pl = (g.planes > 1 && item >= g.p[1].items_before) + (g.planes > 2 && item >= g.p[2].items_before);
    const MovePlane m = pl == 0 ? g.p[0] : pl == 1 ? g.p[1] : g.p[2];
    const uint32_t d = (m.first_piece + (item - m.items_before)) * 16u, end = m.dst_off + m.rows * m.row_bytes;
    const uint32_t lo = d > m.dst_off ? d : m.dst_off, hi = d + 16u < end ? d + 16u : end;
    uint32_t row = m.rows == 1 ? 0u : (lo - m.dst_off) / m.row_bytes, col = (lo - m.dst_off) - row * m.row_bytes;
    if (hi - lo == 16u && col + 16u <= m.row_bytes) {
      *(uint4*)(out + d) = get16(in, m.src_off + row * m.src_stride + col);
    } else {
      for (uint32_t b = lo; b < hi; b++) {
        out[b] = in[m.src_off + row * m.src_stride + col];
        if (++col == m.row_bytes) col = 0, row++;
      }
    }
  }
}

// ---- k_yuv_unpack<Codec> ----
// A codec's MACROPIXEL is the least it codes on its own: one pixel (v308, v408, v410), two (yuv2), a 2 x 2 square (yuv4),
// a group of six in four words (v210).  A row of the work is a run of macropixels whose input and whose output samples
// are both consecutive: the whole frame for the codecs without row structure (with tight pictures pixel p of a frame is
// input byte 3p or 4p and output sample p), a pair of picture rows for yuv4, a row for v210.  A row is cut into WIDE
// items of kPerItem macropixels, as many as give every plane whole 16-byte pieces, and behind them tail items of one
// macropixel each.  A wide item loads 16 bytes at a time, shuffles in registers and stores 16 bytes at a time wherever the
// plane's offset in the picture (and the row's in the plane) is a multiple of 16, by words or bytes where it is not.
struct Geo {
  uint32_t items, items_per_row, full_per_row;
  uint32_t in_stride;  // bytes between the rows of the packet
  uint32_t w;          // the picture's width
  uint32_t off[3];     // the planes' offsets in the picture
};

struct V308 {  // :366-376: V Y U -> Y, U, V
  static constexpr bool kRows = false;
  static constexpr uint32_t kPerItem = 16;
  static uint32_t macropixels(uint32_t w, uint32_t h) { return w * h; }
  __device__ static void wide(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const Geo& g, uint32_t, uint32_t k) {
    uint32_t v[12], y[4], cb[4], cr[4];
    load16s(v, in, 48u * k, 3);
#pragma unroll
    for (int q = 0; q < 4; q++) cr[q] = gather4(v, 12 * q, 3), y[q] = gather4(v, 12 * q + 1, 3), cb[q] = gather4(v, 12 * q + 2, 3);
    put16(out, g.off[0] + 16u * k, y), put16(out, g.off[1] + 16u * k, cb), put16(out, g.off[2] + 16u * k, cr);
  }
  __device__ static void one(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const Geo& g, uint32_t, uint32_t p) {
    out[g.off[0] + p] = in[3u * p + 1u], out[g.off[1] + p] = in[3u * p + 2u], out[g.off[2] + p] = in[3u * p];
  }
};

struct V408 {  // :155-163: U Y V A -> Y U V alpha(A), packed
  static constexpr bool kRows = false;
  static constexpr uint32_t kPerItem = 4;
  static uint32_t macropixels(uint32_t w, uint32_t h) { return w * h; }
  __device__ static uint32_t pixel(uint32_t x) {
    return ((x >> 8) & 0xffu) | (x & 0xffu) << 8 | (x & 0xff0000u) | alpha_v408(x >> 24) << 24;
  }
  __device__ static void wide(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const Geo&, uint32_t, uint32_t k) {
    const uint4 x = *(const uint4*)(in + 16u * k);
    *(uint4*)(out + 16u * k) = make_uint4(pixel(x.x), pixel(x.y), pixel(x.z), pixel(x.w));
  }
  __device__ static void one(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const Geo&, uint32_t, uint32_t p) {
    *(uint32_t*)(out + 4u * p) = pixel(*(const uint32_t*)(in + 4u * p));
  }
};

struct V410 {  // :422-431: one word a pixel -> Y, U, V, 16 bits
  static constexpr bool kRows = false;
  static constexpr uint32_t kPerItem = 8;
  static uint32_t macropixels(uint32_t w, uint32_t h) { return w * h; }
  __device__ static uint32_t luma(uint32_t x) { return (x & 0x3ff000u) >> 6; }
  __device__ static uint32_t cb(uint32_t x) { return (x & 0xffcu) << 4; }
  __device__ static uint32_t cr(uint32_t x) { return (x & 0xffc00000u) >> 16; }
  __device__ static void wide(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const Geo& g, uint32_t, uint32_t k) {
    uint32_t v[8], y[4], u[4], r[4];
    load16s(v, in, 32u * k, 2);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      y[q] = luma(v[2 * q]) | luma(v[2 * q + 1]) << 16;
      u[q] = cb(v[2 * q]) | cb(v[2 * q + 1]) << 16;
      r[q] = cr(v[2 * q]) | cr(v[2 * q + 1]) << 16;
    }
    put16(out, g.off[0] + 16u * k, y), put16(out, g.off[1] + 16u * k, u), put16(out, g.off[2] + 16u * k, r);
  }
  __device__ static void one(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const Geo& g, uint32_t, uint32_t p) {
    const uint32_t x = *(const uint32_t*)(in + 4u * p);
    *(uint16_t*)(out + g.off[0] + 2u * p) = (uint16_t)luma(x);
    *(uint16_t*)(out + g.off[1] + 2u * p) = (uint16_t)cb(x);
    *(uint16_t*)(out + g.off[2] + 2u * p) = (uint16_t)cr(x);
  }
};

struct Yuv2 {  // :71-81: Y0 U Y1 V -> Y, U ^ 0x80, V ^ 0x80.  Rows of 2w bytes make rows of w and w/2: no row structure
  static constexpr bool kRows = false;
  static constexpr uint32_t kPerItem = 16;
  static uint32_t macropixels(uint32_t w, uint32_t h) { return w / 2 * h; }
  __device__ static void wide(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const Geo& g, uint32_t, uint32_t k) {
    uint32_t v[16], y[8], u[4], r[4];
    load16s(v, in, 64u * k, 4);
#pragma unroll
    for (int q = 0; q < 8; q++) y[q] = gather4(v, 8 * q, 2);
#pragma unroll
    for (int q = 0; q < 4; q++) u[q] = gather4(v, 16 * q + 1, 4) ^ 0x80808080u, r[q] = gather4(v, 16 * q + 3, 4) ^ 0x80808080u;
    put16(out, g.off[0] + 32u * k, y), put16(out, g.off[0] + 32u * k + 16u, y + 4);
    put16(out, g.off[1] + 16u * k, u), put16(out, g.off[2] + 16u * k, r);
  }
  __device__ static void one(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const Geo& g, uint32_t, uint32_t m) {
    const uint32_t x = *(const uint32_t*)(in + 4u * m);
    *(uint16_t*)(out + g.off[0] + 2u * m) = (uint16_t)((x & 0xffu) | ((x >> 16) & 0xffu) << 8);
    out[g.off[1] + m] = (uint8_t)((x >> 8) ^ 0x80u), out[g.off[2] + m] = (uint8_t)((x >> 24) ^ 0x80u);
  }
};

struct Yuv4 {  // :560-582: row i of the packet, macropixels U V Y00 Y01 Y10 Y11 -> rows 2i, 2i + 1 of Y, row i of U and V
  static constexpr bool kRows = true;
  static constexpr uint32_t kPerItem = 16;
  static uint32_t rows(uint32_t, uint32_t h) { return h / 2; }
  static uint32_t per_row(uint32_t w) { return w / 2; }
  __device__ static void wide(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const Geo& g, uint32_t row, uint32_t k) {
    uint32_t v[24], top[8], bottom[8], u[4], r[4];
    load16s(v, in, row * g.in_stride + 96u * k, 6);
#pragma unroll
    for (int q = 0; q < 8; q++) {  // two macropixels a word
      top[q] = byte_at(v, 12 * q + 2) | byte_at(v, 12 * q + 3) << 8 | byte_at(v, 12 * q + 8) << 16 | byte_at(v, 12 * q + 9) << 24;
      bottom[q] = byte_at(v, 12 * q + 4) | byte_at(v, 12 * q + 5) << 8 | byte_at(v, 12 * q + 10) << 16 | byte_at(v, 12 * q + 11) << 24;
    }
#pragma unroll
    for (int q = 0; q < 4; q++) u[q] = gather4(v, 24 * q, 6) ^ 0x80808080u, r[q] = gather4(v, 24 * q + 1, 6) ^ 0x80808080u;
    const uint32_t y0 = g.off[0] + 2u * row * g.w + 32u * k, c = row * (g.w / 2u) + 16u * k;
    put16(out, y0, top), put16(out, y0 + 16u, top + 4), put16(out, y0 + g.w, bottom), put16(out, y0 + g.w + 16u, bottom + 4);
    put16(out, g.off[1] + c, u), put16(out, g.off[2] + c, r);
  }
  __device__ static void one(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const Geo& g, uint32_t row, uint32_t m) {
    const uint8_t* s = in + row * g.in_stride + 6u * m;
    const uint32_t y0 = g.off[0] + 2u * row * g.w + 2u * m, c = row * (g.w / 2u) + m;
    out[g.off[1] + c] = s[0] ^ 0x80, out[g.off[2] + c] = s[1] ^ 0x80;
    out[y0] = s[2], out[y0 + 1u] = s[3], out[y0 + g.w] = s[4], out[y0 + g.w + 1u] = s[5];
  }
};

struct V210 {  // :476-521: four words a group of six pixels; a wide item is eight groups, 128 bytes in, 96 + 48 + 48 out
  static constexpr bool kRows = true;
  static constexpr uint32_t kPerItem = 8;
  static uint32_t rows(uint32_t, uint32_t h) { return h; }
  static uint32_t per_row(uint32_t w) { return (w + 5u) / 6u; }  // the last group of a row may code 2 or 4 pixels
  // field k of a word (Cb0 Y0 Cr0 | Y1 Cb1 Y2 | Cr1 Y3 Cb2 | Y4 Cr2 Y5), << 6
  __device__ static uint32_t field(uint32_t x, int k) { return ((x >> (10 * k)) & 0x3ffu) << 6; }
  __device__ static void wide(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const Geo& g, uint32_t row, uint32_t k) {
    uint32_t v[32], y[24], u[12], r[12];
    load16s(v, in, row * g.in_stride + 128u * k, 8);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint32_t a = v[4 * j], b = v[4 * j + 1], c = v[4 * j + 2], d = v[4 * j + 3];
      y[3 * j] = field(a, 1) | field(b, 0) << 16, y[3 * j + 1] = field(b, 2) | field(c, 1) << 16;
      y[3 * j + 2] = field(d, 0) | field(d, 2) << 16;
      const uint32_t cb[3] = {field(a, 0), field(b, 1), field(c, 2)}, cr[3] = {field(a, 2), field(c, 0), field(d, 1)};
#pragma unroll
      for (int t = 0; t < 3; t++) {
        const int s = 3 * j + t;
        if (s & 1) u[s >> 1] |= cb[t] << 16, r[s >> 1] |= cr[t] << 16;
        else u[s >> 1] = cb[t], r[s >> 1] = cr[t];
      }
    }
    const uint32_t y0 = g.off[0] + row * 2u * g.w + 96u * k, c0 = row * g.w + 48u * k;
#pragma unroll
    for (int q = 0; q < 6; q++) put16(out, y0 + 16u * q, y + 4 * q);
#pragma unroll
    for (int q = 0; q < 3; q++) put16(out, g.off[1] + c0 + 16u * q, u + 4 * q), put16(out, g.off[2] + c0 + 16u * q, r + 4 * q);
  }
  // one group, whole (it lies inside the row: the stride is a multiple of a group) or its first 2 or 4 pixels (:501-521)
  __device__ static void one(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const Geo& g, uint32_t row, uint32_t m) {
    const uint4 x = *(const uint4*)(in + row * g.in_stride + 16u * m);
    const uint32_t px = 6u * m, left = g.w - px, n = left < 6u ? left : 6u;
    uint16_t* y = (uint16_t*)(out + g.off[0] + row * 2u * g.w + 2u * px);
    uint16_t* u = (uint16_t*)(out + g.off[1] + row * g.w + px);
    uint16_t* r = (uint16_t*)(out + g.off[2] + row * g.w + px);
    u[0] = (uint16_t)field(x.x, 0), y[0] = (uint16_t)field(x.x, 1), r[0] = (uint16_t)field(x.x, 2), y[1] = (uint16_t)field(x.y, 0);
    if (n >= 4u) u[1] = (uint16_t)field(x.y, 1), y[2] = (uint16_t)field(x.y, 2), r[1] = (uint16_t)field(x.z, 0), y[3] = (uint16_t)field(x.z, 1);
    if (n >= 6u) u[2] = (uint16_t)field(x.z, 2), y[4] = (uint16_t)field(x.w, 0), r[2] = (uint16_t)field(x.w, 1), y[5] = (uint16_t)field(x.w, 2);
  }
};

template <class C>
inline Geo unpack_geo(const Shape& s) {
  Geo g{};
  const uint32_t w = s.w[0], h = s.h[0];
  uint32_t rows = 1, per_row;
  if constexpr (C::kRows) rows = C::rows(w, h), per_row = C::per_row(w);
  else per_row = C::macropixels(w, h);
  // v210's wide items hold whole groups of six only: the group that codes a row's last 2 or 4 pixels is a tail item
  const uint32_t whole = std::is_same<C, V210>::value ? w / 6u : per_row;
  g.full_per_row = whole / C::kPerItem;
  g.items_per_row = g.full_per_row + (per_row - g.full_per_row * C::kPerItem);
  g.items = rows * g.items_per_row;
  g.in_stride = (uint32_t)s.src_stride[0], g.w = w;
  for (uint32_t p = 0; p < s.planes; p++) g.off[p] = (uint32_t)s.dst_off[p];
  return g;
}

template <class C>
__global__ __launch_bounds__(256) void k_yuv_unpack(const uint8_t* __restrict__ packets, uint64_t packet_stride,
                                                    uint8_t* __restrict__ pics, uint64_t pic_stride, Geo g) {
  const uint8_t* __restrict__ in = packets + (uint64_t)blockIdx.y * packet_stride;
  uint8_t* __restrict__ out = pics + (uint64_t)blockIdx.y * pic_stride;
  for (uint32_t item = blockIdx.x * kThreads + threadIdx.x; item < g.items; item += gridDim.x * kThreads) {
    uint32_t row = 0, k = item;
    if constexpr (C::kRows) row = item / g.items_per_row, k = item - row * g.items_per_row;
    if (k < g.full_per_row) C::wide(in, out, g, row, k);
    else C::one(in, out, g, row, g.full_per_row * C::kPerItem + (k - g.full_per_row));
  }
}

}  // namespace miyuv
