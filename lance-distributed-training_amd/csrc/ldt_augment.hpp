// ldt_augment.hpp — the arithmetic of the auto-augment stage (ldt_set_augments):
// the op set of torchvision's TrivialAugmentWide / RandAugment / AutoAugment as
// it acts on a uint8 PIL image, restated so that every result is Pillow's bit
// for bit. One source for the kernels (ldt_augment.hip) and for the CPU check
// against Pillow itself (tools/checks/augment_host.cpp,
// tests/test_augment_ops.py), so it is plain arithmetic with no HIP call. The
// blend, L and the contrast mean are ldt_color.hpp's.
//
// What is restated (Pillow 12, libImaging):
//   affine        Geometry.c affine_fixed, the 16.16 fixed-point walk that
//                 Image.transform(AFFINE, NEAREST) takes: the host rounds the
//                 six coefficients (aug_affine_fix) and the device walks them
//   SMOOTH        Filter.c ImagingFilter3x3 with ImageFilter.SMOOTH's kernel
//                 (1,1,1,1,5,1,1,1,1) / 13 in float32: the sum starts at 0.5,
//                 takes the row below first, then the pixel's row, then the
//                 row above, each as a*k0 + b*k1 + c*k2, and is truncated; the
//                 one-pixel border is copied. ImageEnhance.Sharpness blends it
//                 with the image
//   posterize     ImageOps.posterize: v & ~(2^(8 - bits) - 1)
//   invert        255 - v
//   autocontrast  ImageOps.autocontrast(cutoff=0): per channel the lowest and
//                 highest value present, a table in double arithmetic
//   equalize      ImageOps.equalize: per channel a table from the histogram
// Every floating-point step is an IEEE basic operation, so the device gives
// what the host gives as long as no multiply-add is contracted.
#pragma once
#include <math.h>
#include <stdint.h>

#include "ldt_color.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ldt {

// ldt_aug's op codes.
constexpr int kAugIdentity = 0, kAugAffine = 1, kAugBrightness = 2, kAugColor = 3, kAugContrast = 4,
              kAugSharpness = 5, kAugPosterize = 6, kAugSolarize = 7, kAugAutoContrast = 8, kAugEqualize = 9,
              kAugInvert = 10, kAugOpCodes = 11;

// True when the op needs the image's statistics before it runs (k_aug_stats).
LDT_COLOR_HD bool aug_needs_stats(int code) {
  return code == kAugContrast || code == kAugAutoContrast || code == kAugEqualize;
}

// Host side of the affine op: Pillow's FIX() of the six coefficients of the
// output -> input matrix, the half-pixel term folded into the two offsets.
// False when a coefficient's magnitude is >= 32768 (Pillow leaves the
// fixed-point path there) or is not finite.
inline bool aug_affine_fix(const double m[6], int32_t a[6]) {
  for (int k = 0; k < 6; ++k)
    if (!(fabs(m[k]) < 32768.0)) return false;
  const double v[6] = {m[0], m[1], m[2] + m[0] * 0.5 + m[1] * 0.5, m[3], m[4], m[5] + m[3] * 0.5 + m[4] * 0.5};
  for (int k = 0; k < 6; ++k) {
    const double f = floor(v[k] * 65536.0 + 0.5);
    if (!(f >= -2147483648.0 && f <= 2147483647.0)) return false;
    a[k] = (int32_t)f;
  }
  return true;
}

// True when the walk of `a` over an output of w x h stays inside int32 (Pillow
// walks in int and this restates it in 64 bits, so they agree exactly then).
inline bool aug_affine_walk_ok(const int32_t a[6], int w, int h) {
  for (int o = 0; o < 2; ++o) {
    const int64_t c0 = a[3 * o], c1 = a[3 * o + 1], c2 = a[3 * o + 2];
    for (int cy = 0; cy < 2; ++cy)
      for (int cx = 0; cx < 2; ++cx) {
        // one step past the last pixel: Pillow adds before it tests the loop's end
        const int64_t v = c2 + c0 * (cx ? w : 0) + c1 * (cy ? h : 0);
        if (v < -2147483648LL || v > 2147483647LL) return false;
      }
  }
  return true;
}

// The source pixel of output pixel (x, y) of a w x h image under the fixed
// coefficients `a`; false when it lies outside (the output keeps the fill).
LDT_COLOR_HD bool aug_affine_src(const int32_t a[6], int x, int y, int w, int h, int &xin, int &yin) {
  const int64_t xx = (int64_t)a[2] + (int64_t)a[0] * x + (int64_t)a[1] * y;
  const int64_t yy = (int64_t)a[5] + (int64_t)a[3] * x + (int64_t)a[4] * y;
  xin = (int)(xx >> 16);
  yin = (int)(yy >> 16);
  return xin >= 0 && xin < w && yin >= 0 && yin < h;
}

// ImageFilter.SMOOTH of the pixel whose 3 x 3 neighbourhood is up[3] (the row
// above), mid[3], down[3] (the row below). The border rule is the caller's:
// aug_smooth_is_border.
LDT_COLOR_HD int aug_smooth3x3(const int up[3], const int mid[3], const int down[3]) {
  const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
  float ss = 0.5f;
  ss += ((float)down[0] * k1 + (float)down[1] * k1) + (float)down[2] * k1;
  ss += ((float)mid[0] * k1 + (float)mid[1] * k5) + (float)mid[2] * k1;
  ss += ((float)up[0] * k1 + (float)up[1] * k1) + (float)up[2] * k1;
  return ss <= 0.0f ? 0 : ss >= 255.0f ? 255 : (int)ss;
}

// True when SMOOTH copies pixel (x, y) of a w x h image: the first and last
// row and column, and every pixel of an image with a side below 3.
LDT_COLOR_HD bool aug_smooth_is_border(int x, int y, int w, int h) {
  return x == 0 || y == 0 || x == w - 1 || y == h - 1; // a side below 3 has no other pixel
}

LDT_COLOR_HD int aug_posterize(int v, int bits) { return v & ~((1 << (8 - bits)) - 1) & 255; }
LDT_COLOR_HD int aug_invert(int v) { return 255 - v; }
LDT_COLOR_HD int aug_solarize(int v, int threshold) { return v < threshold ? v : 255 - v; }

// One entry of ImageOps.autocontrast's table for a channel whose lowest and
// highest present values are lo and hi (hi < lo: an empty histogram).
LDT_COLOR_HD int aug_autocontrast_entry(int i, int lo, int hi) {
  if (hi <= lo) return i;
  const double scale = 255.0 / (double)(hi - lo);
  const double offset = (double)(-lo) * scale;
  const double prod = (double)i * scale;
  const int ix = (int)(prod + offset);
  return ix < 0 ? 0 : ix > 255 ? 255 : ix;
}

// ImageOps.autocontrast's table of one channel from its 256-bin histogram.
LDT_COLOR_HD void aug_autocontrast_lut(const uint32_t *h, uint8_t *lut) {
  int lo = 256, hi = -1;
  for (int i = 0; i < 256; ++i)
    if (h[i]) {
      if (lo == 256) lo = i;
      hi = i;
    }
  for (int i = 0; i < 256; ++i) lut[i] = (uint8_t)aug_autocontrast_entry(i, lo, hi);
}

// ImageOps.equalize's step of one channel: 0 means the identity table (at most
// one bin present, or fewer than 255 pixels outside the last present bin).
LDT_COLOR_HD uint32_t aug_equalize_step(const uint32_t *h) {
  uint32_t sum = 0, last = 0;
  int present = 0;
  for (int i = 0; i < 256; ++i)
    if (h[i]) {
      sum += h[i];
      last = h[i];
      ++present;
    }
  return present <= 1 ? 0u : (sum - last) / 255u;
}

// ImageOps.equalize's table of one channel from its 256-bin histogram (the
// pixel count is at most 2^20, so every sum fits 32 bits).
LDT_COLOR_HD void aug_equalize_lut(const uint32_t *h, uint8_t *lut) {
  const uint32_t step = aug_equalize_step(h);
  if (step == 0) {
    for (int i = 0; i < 256; ++i) lut[i] = (uint8_t)i;
    return;
  }
  uint32_t n = step / 2;
  for (int i = 0; i < 256; ++i) {
    const uint32_t q = n / step;
    lut[i] = (uint8_t)(q > 255u ? 255u : q);
    n += h[i];
  }
}

// The pointwise ops of one pixel: everything but affine, sharpness and the two
// table ops. `mean` is the image's rounded L mean (contrast only).
LDT_COLOR_HD void aug_pointwise(int code, float factor, int param, int mean, int &r, int &g, int &b) {
  if (code == kAugBrightness) {
    r = color_blend(0, r, factor);
    g = color_blend(0, g, factor);
    b = color_blend(0, b, factor);
  } else if (code == kAugColor) {
    const int l = color_l(r, g, b);
    r = color_blend(l, r, factor);
    g = color_blend(l, g, factor);
    b = color_blend(l, b, factor);
  } else if (code == kAugContrast) {
    r = color_blend(mean, r, factor);
    g = color_blend(mean, g, factor);
    b = color_blend(mean, b, factor);
  } else if (code == kAugPosterize) {
    r = aug_posterize(r, param);
    g = aug_posterize(g, param);
    b = aug_posterize(b, param);
  } else if (code == kAugSolarize) {
    r = aug_solarize(r, param);
    g = aug_solarize(g, param);
    b = aug_solarize(b, param);
  } else if (code == kAugInvert) {
    r = aug_invert(r);
    g = aug_invert(g);
    b = aug_invert(b);
  }
}

} // namespace ldt
