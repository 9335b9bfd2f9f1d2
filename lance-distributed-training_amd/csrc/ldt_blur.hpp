// ldt_blur.hpp — the blur's arithmetic: Pillow's ImageFilter.GaussianBlur(radius)
// on a uint8 image, restated so that every byte is Pillow's. One source for the
// kernel (k_color_blur in ldt_color.hip), for ldt_blur_weights (ldt_abi.cpp) and
// for the CPU check against Pillow itself (tools/checks/blur_host.cpp,
// tests/test_blur_ops.py), so it is plain arithmetic with no HIP call.
//
// What is restated (Pillow 12, libImaging BoxBlur.c): a Gaussian blur is three
// "extended box" blurs along the rows, then three along the columns, each on
// the bytes the pass before it rounded. An extended box of (real) radius fr has
// 2 * r + 1 taps of weight ww, r = (int)fr, and one tap of weight fw beyond each
// end; the weights are 24-bit fixed point and sum to 2^24 at most, so a pass is
// exact in uint32. Lines are extended by their edge pixel.
//
// The way from Pillow's radius to (r, ww) is float32 arithmetic, except for one
// sqrt and one floor whose arguments are double, and ends in a float32 division
// whose quotient is truncated. Every step is an IEEE basic operation and no
// multiply-add may be contracted: build with -ffp-contract=off (this header
// says so again).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LDT_BLUR_HD __host__ __device__ __forceinline__
#else
#define LDT_BLUR_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ldt {

// The largest Pillow radius taken, and the box radius r it gives, which the
// kernel's halo is sized for.
constexpr float kBlurMaxRadius = 8.0f;
constexpr int kBlurMaxR = 7;

// Pillow's radius -> the box radius r and the tap weight ww of each of the
// three passes per axis. False when the radius is not in [0, kBlurMaxRadius]
// (NaN included). Radius 0 gives (0, 2^24): the identity.
inline bool blur_weights(float radius, int32_t &r, uint32_t &ww) {
  r = 0;
  ww = 0;
  if (!(radius >= 0.0f && radius <= kBlurMaxRadius)) return false; // NaN fails both
  const float sigma2 = radius * radius / 3.0f;
  const float L = (float)sqrt(12.0 * (double)sigma2 + 1.0);
  const float l = (float)floor(((double)L - 1.0) / 2.0);
  float a = (2.0f * l + 1.0f) * (l * (l + 1.0f) - 3.0f * sigma2);
  a /= 6.0f * (sigma2 - (l + 1.0f) * (l + 1.0f));
  const float fr = l + a;
  if (!(fr >= 0.0f) || fr >= (float)(kBlurMaxR + 1)) return false;
  // a float32 division: its rounded quotient is what Pillow truncates (in
  // double the quotient of radius 1.0 would truncate to one less)
  const float q = (float)(1 << 24) / (fr * 2.0f + 1.0f);
  r = (int32_t)fr;
  ww = (uint32_t)q;
  return true;
}

// The edge taps' weight.
LDT_BLUR_HD uint32_t blur_fw(int r, uint32_t ww) { return ((1u << 24) - (uint32_t)(2 * r + 1) * ww) / 2u; }

// True when (r, ww) is a pair a pass can run without wrapping and that
// blur_weights can return: 0 <= r <= kBlurMaxR and 2^24 / (2r + 3) <= ww <=
// 2^24 / (2r + 1).
LDT_BLUR_HD bool blur_pair_ok(int r, uint32_t ww) {
  if (r < 0 || r > kBlurMaxR) return false;
  const uint64_t lo = (uint64_t)(2 * r + 1) * ww, hi = (uint64_t)(2 * r + 3) * ww;
  return lo <= (1u << 24) && hi >= (1u << 24);
}

// One output byte from the sum of its 2r + 1 box taps and of its two edge taps:
// at most 2^24 * 255 + 2^23, so uint32 does not wrap.
LDT_BLUR_HD uint32_t blur_tap(uint32_t sum, uint32_t edge, uint32_t ww, uint32_t fw) {
  return (ww * sum + fw * edge + (1u << 23)) >> 24;
}

// One pass at position x of a line of `len` bytes whose elements are `stride`
// apart: out = (ww * sum(k = -r..r) in[x + k] + fw * (in[x - r - 1] + in[x + r
// + 1]) + 2^23) >> 24, indices clamped to the line.
LDT_BLUR_HD int blur_pass_at(const uint8_t *in, int stride, int len, int x, int r, uint32_t ww, uint32_t fw) {
  const int last = len - 1;
  uint32_t acc = 0;
  for (int k = -r; k <= r; ++k) {
    int i = x + k;
    i = i < 0 ? 0 : i > last ? last : i;
    acc += in[i * stride];
  }
  int lo = x - r - 1, hi = x + r + 1;
  lo = lo < 0 ? 0 : lo > last ? last : lo;
  hi = hi < 0 ? 0 : hi > last ? last : hi;
  const uint32_t edge = (uint32_t)in[lo * stride] + (uint32_t)in[hi * stride];
  return (int)blur_tap(acc, edge, ww, fw);
}

} // namespace ldt
