// The strip layout of the 8-bit twin that the samplers gather from ("Input images"; section 4, "Sampling from
// the 8-bit twin").  A gather costs the memory pipeline per cache line that its lanes touch (tools/ubench/gather.hip), and a
// 128-byte line of a row-major 8-bit image is 128 pixels of ONE row, of which a description window uses a third.  Here a line is a
// 2-D block: the image is cut into strips of 15 columns, a strip stores 16 bytes per image row - its 15 columns and the first
// column of the next strip - with the rows consecutive, so that a line is 8 whole rows of a strip.
//   strip s holds the pixels 15 s ... 15 s + 15 of every row;  a pair (x, x + 1) with x <= w - 2 lies in ONE 16-byte row
//   (x = 15 s + 14 -> bytes 14 and 15 of strip s), and the pair of row y + 1 is the same address + 16: no case analysis at seams.
//   offset(x, y) = s * strip_pitch + 16 y + (x - 15 s),  s = x / 15,  strip_pitch = 16 * (h rounded up to 8)
//   image pitch  = n_strips * strip_pitch,  n_strips = ceil((w - 1) / 15)   (the last column is only ever the second of a pair)
// Padding bytes (rows h ... of a strip, columns w ... of the last strip) are written as zero and never read.
// Host and device: the producer (pair.hip), the consumers (device_util.hpp) and the tests (mods_u8_strips_layout) share this file.
#pragma once
#include <cstddef>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MODS_STRIP_HD __host__ __device__
#else
#define MODS_STRIP_HD
#endif
// 24-bit multiplies on the device (full rate; a 32-bit v_mul_lo is a quarter-rate instruction): every operand here is below 2^24
#if defined(__HIP_DEVICE_COMPILE__)
#define MODS_MUL24(a, b) __umul24((a), (b))
#else
#define MODS_MUL24(a, b) ((a) * (b))
#endif

namespace mods {

constexpr int kStripCols = 15, kStripRowBytes = 16;
constexpr unsigned kStripMaxW = 74909;      // x / 15 == (x * 0x8889) >> 19 for every x below this (tests/test_cpu_u8_strips.py runs them all)

MODS_STRIP_HD inline unsigned strip_of(unsigned x) { return MODS_MUL24(x, 0x8889u) >> 19; }
MODS_STRIP_HD inline unsigned strip_pitch(int h) { return (unsigned)kStripRowBytes * (((unsigned)h + 7u) & ~7u); }
MODS_STRIP_HD inline unsigned strip_count(int w) { return w > 1 ? ((unsigned)w - 1u + (kStripCols - 1)) / kStripCols : 1u; }
MODS_STRIP_HD inline size_t strip_image_bytes(int w, int h) { return (size_t)strip_count(w) * strip_pitch(h); }
// sizes the layout's arithmetic covers: strip_of is exact below kStripMaxW, strip_offset multiplies 24-bit operands into 32 bits
MODS_STRIP_HD inline bool strip_layout_ok(int w, int h) {
  return w >= 2 && h >= 2 && (unsigned)w < kStripMaxW && (unsigned)h < (1u << 19) && strip_image_bytes(w, h) < ((size_t)1 << 32);
}
// byte offset of pixel (x, y) in its own strip (x <= w - 2; the pixel x + 1 is the next byte).  pitch = strip_pitch(h)
MODS_STRIP_HD inline unsigned strip_offset(unsigned x, unsigned y, unsigned pitch) {
  const unsigned s = strip_of(x);
  return MODS_MUL24(s, pitch - kStripCols) + kStripRowBytes * y + x;      // = s * pitch + 16 y + (x - 15 s)
}

}  // namespace mods
