// ldt_idct_scaled.hpp — libjpeg's reduced-size inverse DCTs, the arithmetic of
// a drafted decode (ldt_set_draft): jidctred.c jpeg_idct_4x4 and jpeg_idct_2x2
// and jidctint.c jpeg_idct_1x1 restated for one 8x8 block of dequantised
// coefficients. Host and device: k_idct_scaled (ldt_kernels.hip) calls them per
// lane, tests/test_idct_scaled_ops.py compiles them for the CPU and holds them
// against Pillow's draft() byte for byte.
//
// A block at scale 1/2, 1/4, 1/8 becomes 4x4, 2x2, 1x1 samples. The 4x4
// transform never reads row 4 or column 4 of the block, the 2x2 one reads rows
// and columns 0, 1, 3, 5, 7 only, the 1x1 one the DC term alone.
//
// The rounding rule, on record: CONST_BITS 13, PASS1_BITS 2, and every descale
// is DESCALE(x, n) = (x + (1 << (n - 1))) >> n with an arithmetic shift.
//   4x4  pass 1 (columns)  n = CONST_BITS - PASS1_BITS + 1 = 12
//        pass 2 (rows)     n = CONST_BITS + PASS1_BITS + 3 + 1 = 19
//   2x2  pass 1            n = CONST_BITS - PASS1_BITS + 2 = 13
//        pass 2            n = CONST_BITS + PASS1_BITS + 3 + 2 = 20
//   1x1                    n = 3 on dc * q0
// The sample is range_limit[v & 1023] = clamp(sext10(v) + 128, 0, 255). The
// value between the passes is held to 16 bits with signed saturation, as
// libjpeg-turbo's SSE2 routines (the code Pillow runs on x86-64) pack it; for
// valid data that is the identity. libjpeg's shortcuts for columns and rows
// whose AC terms are zero give exactly what the full formula gives (dc << 14
// descaled by 12 is dc << 2), so they are not restated.
//
// All sums are formed in uint32 and wrap: a hostile file can push them past 32
// bits, the low bits the range limit keeps (bits n .. n + 9) are the same as
// in libjpeg's wider sums, and no signed overflow is ever evaluated.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LDT_IDCT_HD __host__ __device__ __forceinline__
#else
#define LDT_IDCT_HD inline
#endif

namespace ldt {

// jidctred.c's constants, FIX(x) = round(x * 2^13)
constexpr int32_t kRedFix_0_211164243 = 1730;
constexpr int32_t kRedFix_0_509795579 = 4176;
constexpr int32_t kRedFix_0_601344887 = 4926;
constexpr int32_t kRedFix_0_720959822 = 5906;
constexpr int32_t kRedFix_0_765366865 = 6270;
constexpr int32_t kRedFix_0_850430095 = 6967;
constexpr int32_t kRedFix_0_899976223 = 7373;
constexpr int32_t kRedFix_1_061594337 = 8697;
constexpr int32_t kRedFix_1_272758580 = 10426;
constexpr int32_t kRedFix_1_451774981 = 11893;
constexpr int32_t kRedFix_1_847759065 = 15137;
constexpr int32_t kRedFix_2_172734803 = 17799;
constexpr int32_t kRedFix_2_562915447 = 20995;
constexpr int32_t kRedFix_3_624509785 = 29692;

// a * c mod 2^32 (c: one of the constants above, possibly negated)
LDT_IDCT_HD uint32_t red_mul(int32_t a, int32_t c) { return (uint32_t)a * (uint32_t)c; }
// DESCALE of a wrapped sum: round, then an arithmetic shift of its int32 reading
LDT_IDCT_HD int32_t red_descale(uint32_t x, int n) { return (int32_t)(x + (1u << (n - 1))) >> n; }
LDT_IDCT_HD int32_t red_sat16(int32_t v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }
// jdmaster.c prepare_range_limit_table past the IDCT, indexed by v & 1023
LDT_IDCT_HD uint8_t red_limit(int32_t v) {
  const int32_t s = (int32_t)((uint32_t)v << 22) >> 22; // sign-extend the low 10 bits
  const int32_t r = s + 128;
  return (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
}

// One 1-D pass of jpeg_idct_4x4 on x[0..7] (x[4] is not read): the four sums
// before the descale, in output order.
LDT_IDCT_HD void red4_1d(const int32_t *x, uint32_t o[4]) {
  const uint32_t t0 = (uint32_t)x[0] << 14; // CONST_BITS + 1
  const uint32_t t2 = red_mul(x[2], kRedFix_1_847759065) + red_mul(x[6], -kRedFix_0_765366865);
  const uint32_t t10 = t0 + t2, t12 = t0 - t2;
  const int32_t z1 = x[7], z2 = x[5], z3 = x[3], z4 = x[1];
  const uint32_t a = red_mul(z1, -kRedFix_0_211164243) + red_mul(z2, kRedFix_1_451774981) +
                     red_mul(z3, -kRedFix_2_172734803) + red_mul(z4, kRedFix_1_061594337);
  const uint32_t b = red_mul(z1, -kRedFix_0_509795579) + red_mul(z2, -kRedFix_0_601344887) +
                     red_mul(z3, kRedFix_0_899976223) + red_mul(z4, kRedFix_2_562915447);
  o[0] = t10 + b;
  o[3] = t10 - b;
  o[1] = t12 + a;
  o[2] = t12 - a;
}

// jpeg_idct_4x4. blk: the dequantised block, row-major (natural order);
// out[4 * r + c]: the sample of row r, column c.
LDT_IDCT_HD void idct_4x4(const int32_t *blk, uint8_t *out) {
  int32_t ws[4][8]; // [output row][column]; column 4 stays unset and unread
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    if (c == 4) continue;
    int32_t x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = blk[8 * j + c];
    uint32_t o[4];
    red4_1d(x, o);
#pragma unroll
    for (int r = 0; r < 4; ++r) ws[r][c] = red_sat16(red_descale(o[r], 12));
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    int32_t x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = j == 4 ? 0 : ws[r][j];
    uint32_t o[4];
    red4_1d(x, o);
#pragma unroll
    for (int c = 0; c < 4; ++c) out[4 * r + c] = red_limit(red_descale(o[c], 19));
  }
}

// One 1-D pass of jpeg_idct_2x2 on x[0..7] (reads 0, 1, 3, 5, 7).
LDT_IDCT_HD void red2_1d(const int32_t *x, uint32_t o[2]) {
  const uint32_t t10 = (uint32_t)x[0] << 15; // CONST_BITS + 2
  const uint32_t t0 = red_mul(x[7], -kRedFix_0_720959822) + red_mul(x[5], kRedFix_0_850430095) +
                      red_mul(x[3], -kRedFix_1_272758580) + red_mul(x[1], kRedFix_3_624509785);
  o[0] = t10 + t0;
  o[1] = t10 - t0;
}

// jpeg_idct_2x2: out[2 * r + c].
LDT_IDCT_HD void idct_2x2(const int32_t *blk, uint8_t *out) {
  int32_t ws[2][8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    if (c == 2 || c == 4 || c == 6) continue;
    int32_t x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = blk[8 * j + c];
    uint32_t o[2];
    red2_1d(x, o);
    ws[0][c] = red_sat16(red_descale(o[0], 13));
    ws[1][c] = red_sat16(red_descale(o[1], 13));
  }
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    int32_t x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = (j == 2 || j == 4 || j == 6) ? 0 : ws[r][j];
    uint32_t o[2];
    red2_1d(x, o);
    out[2 * r] = red_limit(red_descale(o[0], 20));
    out[2 * r + 1] = red_limit(red_descale(o[1], 20));
  }
}

// jpeg_idct_1x1 on the dequantised DC term.
LDT_IDCT_HD uint8_t idct_1x1(int32_t dc) { return red_limit(red_descale((uint32_t)dc, 3)); }

} // namespace ldt
