// color_host.cpp — csrc/ldt_color.hpp compiled for the host, for
// tests/test_color_ops.py: the photometric stage's arithmetic as the kernels
// run it, callable through ctypes on numpy arrays and compared there with
// Pillow itself (zero mismatches allowed).
//
//   g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC color_host.cpp -o libcolor_host.so
//
// With -DCOLOR_HOST_MAIN it is a stand-alone program instead (build it with
// -fsanitize=address,undefined): a sweep of the same functions over all 2^24
// RGB and HSV values, every factor class of the blend and every order, which
// checks that every result is a byte and that the chain equals its ops applied
// one by one; it prints "color ok".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../lance-distributed-training_amd/csrc/ldt_color.hpp"

using namespace ldt;

extern "C" {

// rgb: n pixels, interleaved. out: n bytes.
void color_host_l(const uint8_t *rgb, int64_t n, uint8_t *out) {
  for (int64_t i = 0; i < n; ++i) out[i] = (uint8_t)color_l(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
}

void color_host_rgb2hsv(const uint8_t *rgb, int64_t n, uint8_t *hsv) {
  for (int64_t i = 0; i < n; ++i) {
    int H, S, V;
    color_rgb2hsv(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], H, S, V);
    hsv[3 * i] = (uint8_t)H;
    hsv[3 * i + 1] = (uint8_t)S;
    hsv[3 * i + 2] = (uint8_t)V;
  }
}

void color_host_hsv2rgb(const uint8_t *hsv, int64_t n, uint8_t *rgb) {
  for (int64_t i = 0; i < n; ++i) {
    int r, g, b;
    color_hsv2rgb(hsv[3 * i], hsv[3 * i + 1], hsv[3 * i + 2], r, g, b);
    rgb[3 * i] = (uint8_t)r;
    rgb[3 * i + 1] = (uint8_t)g;
    rgb[3 * i + 2] = (uint8_t)b;
  }
}

// int(mean + 0.5) of n values, as the kernels form it from the summed L.
int color_host_mean_round(uint32_t sum, uint32_t count) { return color_mean_round(sum, count); }

// The rounded L mean of the image (n pixels) in the state it has when
// contrast's turn comes in entry c: what k_color_mean and k_color_apply
// compute between them.
int color_host_mean(const uint8_t *rgb, int64_t n, const ldt_color *c) {
  uint32_t sum = 0;
  for (int64_t i = 0; i < n; ++i) {
    int r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
    color_before_contrast(*c, r, g, b);
    sum += (uint32_t)color_l(r, g, b);
  }
  return color_mean_round(sum, (uint32_t)n);
}

// The whole chain of entry c on n pixels, with the given contrast mean.
void color_host_chain(const uint8_t *rgb, int64_t n, const ldt_color *c, int mean, uint8_t *out) {
  for (int64_t i = 0; i < n; ++i) {
    int r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
    color_chain(*c, mean, r, g, b);
    out[3 * i] = (uint8_t)r;
    out[3 * i + 1] = (uint8_t)g;
    out[3 * i + 2] = (uint8_t)b;
  }
}

} // extern "C"

#ifdef COLOR_HOST_MAIN
static int fail(const char *what, long a, long b, long c) {
  fprintf(stderr, "color_host: %s at (%ld, %ld, %ld)\n", what, a, b, c);
  return 1;
}

static bool byte3(int r, int g, int b) { return r >= 0 && r <= 255 && g >= 0 && g <= 255 && b >= 0 && b <= 255; }

int main() {
  // every RGB value through RGB -> HSV and every HSV value back: bytes only
  for (int r = 0; r < 256; ++r)
    for (int g = 0; g < 256; ++g)
      for (int b = 0; b < 256; ++b) {
        int H, S, V, x, y, z;
        color_rgb2hsv(r, g, b, H, S, V);
        if (!byte3(H, S, V)) return fail("rgb2hsv out of range", r, g, b);
        color_hsv2rgb(r, g, b, x, y, z); // (r, g, b) read as (H, S, V)
        if (!byte3(x, y, z)) return fail("hsv2rgb out of range", r, g, b);
        const int l = color_l(r, g, b);
        if (l < 0 || l > 255) return fail("L out of range", r, g, b);
      }
  // the blend at every (degenerate, pixel) pair, in every factor class
  const float factors[] = {0.0f, 0.33333f, 0.6f, 0.999f, 1.0f, 1.0000001f, 1.4f, 2.5f, 1000.0f, 3.0e38f};
  for (float a : factors)
    for (int d = 0; d < 256; ++d)
      for (int p = 0; p < 256; ++p) {
        const int v = color_blend(d, p, a);
        if (v < 0 || v > 255) return fail("blend out of range", d, p, (long)a);
        if (a == 1.0f && v != p) return fail("blend(1) is not the pixel", d, p, v);
        if (a == 0.0f && v != d) return fail("blend(0) is not the degenerate", d, p, v);
      }
  // the rounded mean at its edges
  if (color_mean_round(0, 1) != 0 || color_mean_round(255, 1) != 255 || color_mean_round(1, 2) != 1 ||
      color_mean_round(255u << 20, 1u << 20) != 255 || color_mean_round((1u << 19) - 1, 1u << 20) != 0 ||
      color_mean_round(1u << 19, 1u << 20) != 1)
    return fail("mean_round", 0, 0, 0);
  // every order: the chain equals its ops one by one, then gray, then solarize
  static const uint8_t perms[24][4] = {{0, 1, 2, 3}, {0, 1, 3, 2}, {0, 2, 1, 3}, {0, 2, 3, 1}, {0, 3, 1, 2}, {0, 3, 2, 1},
                                       {1, 0, 2, 3}, {1, 0, 3, 2}, {1, 2, 0, 3}, {1, 2, 3, 0}, {1, 3, 0, 2}, {1, 3, 2, 0},
                                       {2, 0, 1, 3}, {2, 0, 3, 1}, {2, 1, 0, 3}, {2, 1, 3, 0}, {2, 3, 0, 1}, {2, 3, 1, 0},
                                       {3, 0, 1, 2}, {3, 0, 2, 1}, {3, 1, 0, 2}, {3, 1, 2, 0}, {3, 2, 0, 1}, {3, 2, 1, 0}};
  for (int k = 0; k < 24; ++k)
    for (int gray = 0; gray < 2; ++gray)
      for (int sol = -1; sol <= 256; sol += 129) {
        ldt_color c;
        memset(&c, 0, sizeof(c));
        c.brightness = 1.3f;
        c.contrast = 0.7f;
        c.saturation = 1.9f;
        c.hue_shift = 231;
        memcpy(c.order, perms[k], 4);
        c.mask = 15;
        c.gray = (uint8_t)gray;
        c.solarize = (int16_t)sol;
        for (int px = 0; px < 4096; ++px) {
          const int r0 = (px * 37) & 255, g0 = (px * 101 + 7) & 255, b0 = (px * 13 + 200) & 255;
          int r = r0, g = g0, b = b0;
          color_chain(c, 117, r, g, b);
          int x = r0, y = g0, z = b0;
          for (int j = 0; j < 4; ++j) color_op(c, perms[k][j], 117, x, y, z);
          if (gray) x = y = z = color_l(x, y, z);
          if (sol >= 0) {
            x = x < sol ? x : 255 - x;
            y = y < sol ? y : 255 - y;
            z = z < sol ? z : 255 - z;
          }
          if (r != x || g != y || b != z || !byte3(r, g, b)) return fail("chain", k, gray, sol);
        }
      }
  printf("color ok\n");
  return 0;
}
#endif
