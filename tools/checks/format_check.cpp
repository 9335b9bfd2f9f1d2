// format_check.cpp — host check of the planner's 16-bit output tables
// (csrc/ldt_plan.cpp: f32_to_f16_bits, f32_to_bf16_bits, build_lut,
// build_lut16, write_plan's table section), the rounding every fp16 / bf16
// output of the resize kernels carries, built with ASan/UBSan together with
// the planner by tests/test_output_format.py:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off \
//       -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ tools/checks/format_check.cpp \
//       lance-distributed-training_amd/csrc/ldt_plan.cpp -o format_check
//
//   format_check convert in.f32 out.f16 out.bf16
//       in.f32 holds float32 values; writes each one's fp16 bits to out.f16
//       and its bf16 bits to out.bf16 (uint16 each). Prints "convert ok".
//   format_check table M0 M1 M2 S0 S1 S2 | none   out.f32 out.f16 out.bf16
//       build_lut's 768 float32 entries for Normalize(mean, std) (or none) to
//       out.f32 and build_lut16's to out.f16 / out.bf16; write_plan's table
//       section for an empty batch must hold the same bytes in each dtype
//       (and zeros behind the 16-bit forms). Prints "table ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../lance-distributed-training_amd/csrc/ldt_plan.hpp"

using namespace ldt;

namespace {

bool put(const char *path, const void *p, size_t bytes) {
  FILE *f = fopen(path, "wb");
  if (!f) return false;
  const bool ok = fwrite(p, 1, bytes, f) == bytes;
  return fclose(f) == 0 && ok;
}

int convert(const char *in, const char *o16, const char *ob16) {
  FILE *f = fopen(in, "rb");
  if (!f) return 2;
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  if (bytes < 0 || bytes % 4) return 2;
  const size_t n = (size_t)bytes / 4;
  float *x = (float *)malloc(n ? bytes : 4); // exactly the file's size
  uint16_t *h = (uint16_t *)malloc(n ? 2 * n : 2), *b = (uint16_t *)malloc(n ? 2 * n : 2);
  if (fread(x, 4, n, f) != n) return 2;
  fclose(f);
  for (size_t i = 0; i < n; ++i) {
    h[i] = f32_to_f16_bits(x[i]);
    b[i] = f32_to_bf16_bits(x[i]);
  }
  const bool ok = put(o16, h, 2 * n) && put(ob16, b, 2 * n);
  free(x);
  free(h);
  free(b);
  if (!ok) return 2;
  printf("convert ok\n");
  return 0;
}

int table(const ldt_norm *norm, const char *o32, const char *o16, const char *ob16) {
  float *f = (float *)malloc(768 * 4);
  uint16_t *h = (uint16_t *)malloc(768 * 2), *b = (uint16_t *)malloc(768 * 2);
  build_lut(norm, f);
  build_lut16(norm, kDtypeF16, h);
  build_lut16(norm, kDtypeBF16, b);
  // the plan blob of an empty batch: its table section in every dtype
  BatchPlan B;
  const PlanLayout L = plan_layout(B, false);
  uint8_t *blob = (uint8_t *)malloc((size_t)L.plan_bytes);
  const uint8_t zeros[768 * 2] = {};
  int rc = 0;
  for (int dtype = kDtypeF32; dtype <= kDtypeU8 && rc == 0; ++dtype) {
    memset(blob, 0xA5, (size_t)L.plan_bytes);
    write_plan(B, L, norm, nullptr, blob, dtype);
    const uint8_t *t = blob + L.off_lut;
    if (dtype == kDtypeF16 || dtype == kDtypeBF16) {
      if (memcmp(t, dtype == kDtypeF16 ? h : b, 768 * 2) != 0 || memcmp(t + 768 * 2, zeros, 768 * 2) != 0) rc = 3;
    } else if (memcmp(t, f, 768 * 4) != 0) {
      rc = 3;
    }
  }
  if (rc == 0 && !(put(o32, f, 768 * 4) && put(o16, h, 768 * 2) && put(ob16, b, 768 * 2))) rc = 2;
  free(blob);
  free(f);
  free(h);
  free(b);
  if (rc) {
    printf("FAIL table rc=%d\n", rc);
    return rc;
  }
  printf("table ok\n");
  return 0;
}

} // namespace

int main(int argc, char **argv) {
  if (argc == 5 && !strcmp(argv[1], "convert")) return convert(argv[2], argv[3], argv[4]);
  if (argc == 6 && !strcmp(argv[1], "table") && !strcmp(argv[2], "none")) return table(nullptr, argv[3], argv[4], argv[5]);
  if (argc == 11 && !strcmp(argv[1], "table")) {
    ldt_norm nm;
    for (int c = 0; c < 3; ++c) {
      nm.mean[c] = strtof(argv[2 + c], nullptr);
      nm.std[c] = strtof(argv[5 + c], nullptr);
    }
    return table(&nm, argv[8], argv[9], argv[10]);
  }
  fprintf(stderr, "usage: format_check convert in.f32 out.f16 out.bf16 | table (none | M0 M1 M2 S0 S1 S2) out.f32 out.f16 out.bf16\n");
  return 1;
}
