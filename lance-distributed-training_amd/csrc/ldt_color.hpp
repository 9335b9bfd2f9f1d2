// ldt_color.hpp — the photometric stage's arithmetic (ldt_set_colors):
// torchvision's ColorJitter, RandomGrayscale and RandomSolarize as they act on
// a uint8 PIL image, restated per pixel so that every result is Pillow's bit
// for bit. One source for the kernels (ldt_color.hip) and for the CPU check
// against Pillow itself (tools/checks/color_host.cpp, tests/test_color_ops.py),
// so it is plain arithmetic with no HIP call.
//
// What is restated (Pillow 12, libImaging):
//   L            Convert.c L(rgb): (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16
//   blend        Blend.c ImagingBlend, which ImageEnhance.Brightness / Contrast /
//                Color call as Image.blend(degenerate, image, factor): one
//                float32 multiply and one float32 add per channel (never fused),
//                truncated for 0 <= alpha <= 1, clipped otherwise
//   RGB <-> HSV  Convert.c rgb2hsv_row / hsv2rgb, which torchvision's adjust_hue
//                runs around a uint8 wrap-add on H; the mixed float32 / double
//                steps are kept exactly as the C source has them
//   solarize     ImageOps.solarize's table: v < threshold ? v : 255 - v
// ImageFilter.GaussianBlur, which sits between grayscale and solarize, is
// restated in ldt_blur.hpp.
// Every floating-point step is an IEEE basic operation (add, multiply, divide,
// floor, conversion), so the device gives what the host gives as long as no
// multiply-add is contracted: the build has -ffp-contract=off and this header
// says so again.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/ldt.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LDT_COLOR_HD __host__ __device__ __forceinline__
#else
#define LDT_COLOR_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ldt {

// The jitter ops' codes: torchvision's fn_idx.
constexpr int kColorBrightness = 0, kColorContrast = 1, kColorSaturation = 2, kColorHue = 3;

LDT_COLOR_HD int color_clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

LDT_COLOR_HD int color_l(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// Image.blend(degenerate, image, a) for one channel.
LDT_COLOR_HD int color_blend(int deg, int px, float a) {
  const float prod = a * (float)(px - deg);
  const float t = (float)deg + prod;
  if (a >= 0.0f && a <= 1.0f) return (int)(uint8_t)(int)t;
  return t <= 0.0f ? 0 : t >= 255.0f ? 255 : (int)t;
}

// int(mean + 0.5) of `sum` over `count` values (ImageStat's mean of L, as
// ImageEnhance.Contrast rounds it). A non-zero distance of sum / count from a
// half is at least 1 / (2 * count), far above a double's rounding for count <=
// 1024 * 1024, so the integer quotient equals Python's int(sum / count + 0.5).
LDT_COLOR_HD int color_mean_round(uint32_t sum, uint32_t count) {
  return (int)((2u * sum + count) / (2u * count));
}

LDT_COLOR_HD void color_rgb2hsv(int r, int g, int b, int &H, int &S, int &V) {
  const int maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
  const int minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
  V = maxc;
  if (minc == maxc) {
    H = 0;
    S = 0;
    return;
  }
  const float cr = (float)(maxc - minc);
  const float s = cr / (float)maxc;
  const float rc = (float)(maxc - r) / cr;
  const float gc = (float)(maxc - g) / cr;
  const float bc = (float)(maxc - b) / cr;
  float h;
  if (r == maxc) h = bc - gc;
  else if (g == maxc) h = (float)((2.0 + (double)rc) - (double)bc);
  else h = (float)((4.0 + (double)gc) - (double)rc);
  // fmod(h / 6.0 + 1.0, 1.0): the argument is in [5 / 6, 11 / 6], where
  // x - floor(x) is exact and is fmod's value
  const double x = (double)h / 6.0 + 1.0;
  h = (float)(x - floor(x));
  H = color_clip8((int)((double)h * 255.0));
  S = color_clip8((int)((double)s * 255.0));
}

// round() of a value that is never negative here: half away from zero is
// floor(x + 0.5), exact in double for a float32 x below 2^24.
LDT_COLOR_HD int color_round8(float x) { return color_clip8((int)floor((double)x + 0.5)); }

LDT_COLOR_HD void color_hsv2rgb(int H, int S, int V, int &r, int &g, int &b) {
  if (S == 0) {
    r = g = b = V;
    return;
  }
  const double hf = (double)H * 6.0 / 255.0;
  const int i = (int)floor(hf);
  const float f = (float)(hf - (double)i);
  const float fs = (float)((double)S / 255.0);
  const double v = (double)V;
  const int p = color_round8((float)(v * (1.0 - (double)fs)));
  const int q = color_round8((float)(v * (1.0 - (double)fs * (double)f)));
  const int t = color_round8((float)(v * (1.0 - (double)fs * (1.0 - (double)f))));
  switch (i % 6) {
    case 0: r = V; g = t; b = p; break;
    case 1: r = q; g = V; b = p; break;
    case 2: r = p; g = V; b = t; break;
    case 3: r = p; g = q; b = V; break;
    case 4: r = t; g = p; b = V; break;
    default: r = V; g = p; b = q; break;
  }
}

// One jitter op of entry `c` on one pixel; `mean` is the image's rounded L
// mean in the state it has when contrast's turn comes (read by contrast only).
LDT_COLOR_HD void color_op(const ldt_color &c, int op, int mean, int &r, int &g, int &b) {
  if (!((c.mask >> op) & 1)) return;
  if (op == kColorBrightness) {
    r = color_blend(0, r, c.brightness);
    g = color_blend(0, g, c.brightness);
    b = color_blend(0, b, c.brightness);
  } else if (op == kColorContrast) {
    r = color_blend(mean, r, c.contrast);
    g = color_blend(mean, g, c.contrast);
    b = color_blend(mean, b, c.contrast);
  } else if (op == kColorSaturation) {
    const int l = color_l(r, g, b);
    r = color_blend(l, r, c.saturation);
    g = color_blend(l, g, c.saturation);
    b = color_blend(l, b, c.saturation);
  } else {
    int H, S, V;
    color_rgb2hsv(r, g, b, H, S, V);
    color_hsv2rgb((H + c.hue_shift) & 255, S, V, r, g, b);
  }
}

// True when entry `c` applies contrast, whose mean needs a pass of its own.
LDT_COLOR_HD bool color_has_contrast(const ldt_color &c) { return (c.mask >> kColorContrast) & 1; }
// True when the entry changes nothing: a plain table store.
LDT_COLOR_HD bool color_is_identity(const ldt_color &c) { return (c.mask & 15) == 0 && !c.gray && c.solarize < 0; }

// The ops that precede contrast in the entry's order: the state of the image
// whose L the contrast mean is taken of.
LDT_COLOR_HD void color_before_contrast(const ldt_color &c, int &r, int &g, int &b) {
  bool done = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int op = c.order[k];
    if (op == kColorContrast) done = true;
    if (!done) color_op(c, op, 0, r, g, b);
  }
}

// The chain of one output pixel up to the blur's place: the jitter ops in the
// entry's order, then grayscale.
LDT_COLOR_HD void color_chain_head(const ldt_color &c, int mean, int &r, int &g, int &b) {
#pragma unroll
  for (int k = 0; k < 4; ++k) color_op(c, c.order[k], mean, r, g, b);
  if (c.gray) r = g = b = color_l(r, g, b);
}

// What follows the blur's place: solarize.
LDT_COLOR_HD void color_chain_tail(const ldt_color &c, int &r, int &g, int &b) {
  if (c.solarize >= 0) {
    const int th = c.solarize;
    r = r < th ? r : 255 - r;
    g = g < th ? g : 255 - g;
    b = b < th ? b : 255 - b;
  }
}

// The whole chain of one output pixel of an entry without blur: the jitter ops
// in the entry's order, then grayscale, then solarize. An entry with blur
// (blur_ww != 0) runs the head, the blur over the image (ldt_blur.hpp), then
// the tail.
LDT_COLOR_HD void color_chain(const ldt_color &c, int mean, int &r, int &g, int &b) {
  color_chain_head(c, mean, r, g, b);
  color_chain_tail(c, r, g, b);
}

} // namespace ldt
