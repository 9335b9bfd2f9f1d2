// mix_host.cpp — csrc/ldt_mix.hpp compiled for the host: the C entry points
// tests/test_mix_ops.py calls through ctypes, and (with -DMIX_HOST_MAIN) a
// stand-alone sweep of the same functions for an ASan / UBSan build.
// Build: c++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC mix_host.cpp
#include <initializer_list>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../lance-distributed-training_amd/csrc/ldt_mix.hpp"

using namespace ldt;

extern "C" {

// out[i] = mix_element(x[i], p[i], w_self, w_partner, boxed)
void mix_host_element(const float *x, const float *p, int64_t n, float w_self, float w_partner, int boxed,
                      float *out) {
  for (int64_t i = 0; i < n; ++i) out[i] = mix_element(x[i], p[i], w_self, w_partner, boxed != 0);
}

// out[i] = the 16-bit form of float32 bits[i]; dtype: LDT_DTYPE_F16 / LDT_DTYPE_BF16
void mix_host_to16(const uint32_t *bits, int64_t n, int dtype, uint16_t *out) {
  for (int64_t i = 0; i < n; ++i) {
    float f;
    memcpy(&f, &bits[i], 4);
    out[i] = (uint16_t)mix_store_bits(f, dtype);
  }
}

// out[i][c] for rows of labels a[i], b[i]
void mix_host_labels(const int64_t *a, const int64_t *b, int64_t n, int num_classes, float lw_self,
                     float lw_partner, float *out) {
  for (int64_t i = 0; i < n; ++i)
    for (int c = 0; c < num_classes; ++c) out[i * num_classes + c] = mix_soft_label(c, a[i], b[i], lw_self, lw_partner);
}

int mix_host_in_box(int y, int x, int top, int left, int height, int width) {
  return mix_in_box(y, x, top, left, height, width) ? 1 : 0;
}

} // extern "C"

#ifdef MIX_HOST_MAIN
int main() {
  uint64_t acc = 0;
  // every float32 whose low 13 bits are a tie or a tie's neighbour, both dtypes
  for (uint32_t hi = 0; hi < (1u << 19); ++hi)
    for (uint32_t lo : {0x0000u, 0x0FFFu, 0x1000u, 0x1001u}) {
      const uint32_t b = (hi << 13) | lo;
      acc += mix_f16_bits(b) + mix_bf16_bits(b);
    }
  const float w[] = {0.0f, 1.0f, 0.5f, 0.123456789f, 3.0e38f, -3.0e38f};
  for (int a = 0; a < 256; ++a)
    for (int b = 0; b < 256; ++b)
      for (float ws : w)
        for (float wp : w) {
          const float v = mix_element((float)a / 255.0f, (float)b / 255.0f, ws, wp, (a ^ b) & 1);
          acc += mix_store_bits(v, LDT_DTYPE_F32) + mix_store_bits(v, LDT_DTYPE_F16) + mix_store_bits(v, LDT_DTYPE_BF16);
        }
  for (int y = -2; y < 6; ++y)
    for (int x = -2; x < 6; ++x) acc += mix_in_box(y, x, 1, 1, 3, 2) + mix_in_box(y, x, 0, 0, 0, 0);
  for (int64_t a = 0; a < 4; ++a)
    for (int64_t b = 0; b < 4; ++b)
      for (int64_t c = 0; c < 4; ++c) acc += mix_f32_bits(mix_soft_label(c, a, b, 0.25f, 0.75f));
  printf("mix_host sweep %llu\n", (unsigned long long)acc);
  return 0;
}
#endif
