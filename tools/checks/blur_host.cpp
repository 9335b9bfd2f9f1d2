// blur_host.cpp — csrc/ldt_blur.hpp compiled for the host, for
// tests/test_blur_ops.py: the blur's arithmetic as the kernel runs it, callable
// through ctypes on numpy arrays and compared there with Pillow's
// ImageFilter.GaussianBlur itself (zero mismatches allowed).
//
//   g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC blur_host.cpp -o libblur_host.so
//
// With -DBLUR_HOST_MAIN it is a stand-alone program instead (build it with
// -fsanitize=address,undefined): the sweep of radii 0..8 in steps of 0.002 on a
// 9 x 11 image and the short axes, which checks that every pair of weights is
// one a pass can run, that every access stays inside its line and that radius 0
// is the identity; it prints "blur ok".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../lance-distributed-training_amd/csrc/ldt_blur.hpp"

using namespace ldt;

extern "C" {

// 0 and (*r, *ww) for Pillow's radius, -1 when the radius is out of range.
int blur_host_weights(float radius, int32_t *r, uint32_t *ww) { return blur_weights(radius, *r, *ww) ? 0 : -1; }

int blur_host_pair_ok(int r, uint32_t ww) { return blur_pair_ok(r, ww) ? 1 : 0; }

// The whole blur of an interleaved h x w x ch image with the weights (r, ww):
// three passes along the rows, then three along the columns, every channel on
// its own, each pass on the bytes of the one before.
void blur_host_image(const uint8_t *in, int h, int w, int ch, int r, uint32_t ww, uint8_t *out) {
  const uint32_t fw = blur_fw(r, ww);
  const size_t n = (size_t)h * w * ch;
  std::vector<uint8_t> a(in, in + n), b(n);
  for (int pass = 0; pass < 6; ++pass) {
    const bool rows = pass < 3;
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x)
        for (int c = 0; c < ch; ++c) {
          const uint8_t *line = rows ? a.data() + (size_t)y * w * ch + c : a.data() + (size_t)x * ch + c;
          b[((size_t)y * w + x) * ch + c] =
              (uint8_t)blur_pass_at(line, rows ? ch : w * ch, rows ? w : h, rows ? x : y, r, ww, fw);
        }
    a.swap(b);
  }
  memcpy(out, a.data(), n);
}

} // extern "C"

#ifdef BLUR_HOST_MAIN
static int fail(const char *what, double radius, int h, int w) {
  fprintf(stderr, "blur_host: %s at radius %.4f, %d x %d\n", what, radius, h, w);
  return 1;
}

int main() {
  static const int sizes[][2] = {{9, 11}, {1, 1}, {1, 7}, {5, 3}, {2, 2}};
  uint8_t img[9 * 11 * 3], out[9 * 11 * 3];
  uint32_t seed = 12345;
  for (uint8_t &v : img) {
    seed = seed * 1664525u + 1013904223u;
    v = (uint8_t)(seed >> 24);
  }
  for (int k = 0; k <= 4000; ++k) {
    const float radius = (float)(k * 0.002);
    int32_t r;
    uint32_t ww;
    if (!blur_weights(radius, r, ww)) return fail("radius refused", radius, 0, 0);
    if (!blur_pair_ok(r, ww)) return fail("weights out of range", radius, r, (int)ww);
    for (const auto &s : sizes) {
      if (k % 50 && s[0] != 9) continue; // the short axes at every 50th radius
      blur_host_image(img, s[0], s[1], 3, r, ww, out);
      if (k == 0 && memcmp(img, out, (size_t)s[0] * s[1] * 3)) return fail("radius 0 is not the identity", radius, s[0], s[1]);
    }
  }
  int32_t r;
  uint32_t ww;
  const float nan = __builtin_nanf("");
  if (blur_weights(8.5f, r, ww) || blur_weights(-1.0f, r, ww) || blur_weights(nan, r, ww) ||
      blur_weights(__builtin_inff(), r, ww))
    return fail("a bad radius was accepted", 0, 0, 0);
  // a flat image stays flat at every weight: the weights sum to 2^24 - (0 or 1)
  memset(img, 255, sizeof(img));
  for (int k = 1; k <= 4000; k += 7) {
    if (!blur_weights((float)(k * 0.002), r, ww)) return fail("radius refused", k * 0.002, 0, 0);
    blur_host_image(img, 9, 11, 3, r, ww, out);
    for (uint8_t v : out)
      if (v != 255) return fail("a flat image changed", k * 0.002, 9, 11);
  }
  printf("blur ok\n");
  return 0;
}
#endif
