// resample_check.cpp — host check of the resize's coefficient arithmetic
// (csrc/ldt_resample.hpp), the code the streaming kernel k_resize runs per
// output column and row, built with ASan/UBSan by tests/test_interpolation.py:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off \
//       -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ tools/checks/resample_check.cpp -o resample_check
//
//   resample_check resize H W OH OW FILTER in.rgb out.rgb
//       Pillow's two-pass resize of the H x W x 3 uint8 image in in.rgb to
//       OH x OW with FILTER (0 BILINEAR, 1 BICUBIC), as k_resize does it:
//       resample_coeffs<FILTER> with resample_ksize_host taps per index, the
//       horizontal pass into a uint8 image through clip8, then the vertical
//       pass through clip8. Every buffer is a heap block of exactly its size.
//   resample_check ksize
//       resample_ksize_host over in, out in 1..1200: BILINEAR equals the
//       formula it had before it took a filter, BICUBIC equals Pillow's
//       (int)ceil(support) * 2 + 1 evaluated in double, and no index of any
//       sampled pair has more taps than that. Prints "ksize ok".
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../lance-distributed-training_amd/csrc/ldt_resample.hpp"

using namespace ldt;

namespace {

template <int FILT>
int resize(int H, int W, int OH, int OW, const uint8_t *src, uint8_t *dst) {
  const int ks_h = resample_ksize_host(W, OW, FILT), ks_v = resample_ksize_host(H, OH, FILT);
  int32_t *kh = (int32_t *)malloc(sizeof(int32_t) * (size_t)OW * ks_h);
  int *hb = (int *)malloc(sizeof(int) * 2 * (size_t)OW);
  for (int x = 0; x < OW; ++x) {
    hb[2 * x + 1] = resample_coeffs<FILT>(W, OW, x, ks_h, kh + (size_t)x * ks_h, &hb[2 * x]);
    if (hb[2 * x + 1] > ks_h || hb[2 * x] < 0 || hb[2 * x] + hb[2 * x + 1] > W) return 3;
  }
  uint8_t *mid = (uint8_t *)malloc((size_t)H * OW * 3); // the uint8 image between the passes
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < OW; ++x)
      for (int c = 0; c < 3; ++c) {
        int32_t s = 1 << (kPrecisionBits - 1);
        const uint8_t *p = src + ((size_t)y * W + hb[2 * x]) * 3 + c;
        for (int t = 0; t < hb[2 * x + 1]; ++t) s += (int32_t)p[3 * t] * kh[(size_t)x * ks_h + t];
        mid[((size_t)y * OW + x) * 3 + c] = (uint8_t)clip8(s);
      }
  int32_t *kv = (int32_t *)malloc(sizeof(int32_t) * (size_t)ks_v);
  for (int y = 0; y < OH; ++y) {
    int ymin;
    const int cnt = resample_coeffs<FILT>(H, OH, y, ks_v, kv, &ymin);
    if (cnt > ks_v || ymin < 0 || ymin + cnt > H) return 3;
    for (int x = 0; x < OW * 3; ++x) {
      int32_t s = 1 << (kPrecisionBits - 1);
      for (int t = 0; t < cnt; ++t) s += (int32_t)mid[(size_t)(ymin + t) * OW * 3 + x] * kv[t];
      dst[(size_t)y * OW * 3 + x] = (uint8_t)clip8(s);
    }
  }
  free(kv);
  free(mid);
  free(hb);
  free(kh);
  return 0;
}

template <int FILT>
int max_count(int in, int out, int ks) {
  int32_t *k = (int32_t *)malloc(sizeof(int32_t) * (size_t)ks);
  int most = 0;
  for (int x = 0; x < out; ++x) {
    int xmin;
    const int cnt = resample_coeffs<FILT>(in, out, x, ks, k, &xmin);
    most = cnt > most ? cnt : most;
  }
  free(k);
  return most;
}

int check_ksize() {
  long pairs = 0, swept = 0;
  for (int in = 1; in <= 1200; ++in)
    for (int out = 1; out <= 1200; ++out, ++pairs) {
      // the formula resample_ksize_host had before it took a filter
      int s = (in + out - 1) / out;
      if (s < 1) s = 1;
      if (resample_ksize_host(in, out) != s * 2 + 1 || resample_ksize_host(in, out, kFilterBilinear) != s * 2 + 1) {
        printf("FAIL bilinear ksize %d -> %d: %d, was %d\n", in, out, resample_ksize_host(in, out), s * 2 + 1);
        return 1;
      }
      // Resample.c precompute_coeffs: support = filter support * filterscale, ksize = (int)ceil(support) * 2 + 1
      for (int f = 0; f < 2; ++f) {
        const double scale = (double)in / (double)out, filterscale = scale < 1.0 ? 1.0 : scale;
        const int pil = (int)ceil((f ? 2.0 : 1.0) * filterscale) * 2 + 1;
        if (resample_ksize_host(in, out, f) != pil) {
          printf("FAIL filter %d ksize %d -> %d: %d, Pillow %d\n", f, in, out, resample_ksize_host(in, out, f), pil);
          return 1;
        }
      }
      const int want = 2 * ((2 * in + out - 1) / out > 2 ? (2 * in + out - 1) / out : 2) + 1;
      if (resample_ksize_host(in, out, kFilterBicubic) != want) {
        printf("FAIL bicubic ksize %d -> %d: %d, the integer formula gives %d\n", in, out,
               resample_ksize_host(in, out, kFilterBicubic), want);
        return 1;
      }
      if ((in * 7 + out * 13) % 97 == 0) { // a sample of the pairs: no index has more taps than the capacity
        ++swept;
        const int kb = resample_ksize_host(in, out, kFilterBicubic), kl = resample_ksize_host(in, out);
        if (max_count<kFilterBicubic>(in, out, kb) > kb || max_count<kFilterBilinear>(in, out, kl) > kl) {
          printf("FAIL %d -> %d: an index has more taps than resample_ksize_host\n", in, out);
          return 1;
        }
      }
    }
  printf("ksize ok: %ld pairs, %ld swept\n", pairs, swept);
  return 0;
}

} // namespace

int main(int argc, char **argv) {
  if (argc == 2 && !strcmp(argv[1], "ksize")) return check_ksize();
  if (argc != 9 || strcmp(argv[1], "resize")) {
    fprintf(stderr, "usage: %s resize H W OH OW FILTER in.rgb out.rgb | %s ksize\n", argv[0], argv[0]);
    return 2;
  }
  const int H = atoi(argv[2]), W = atoi(argv[3]), OH = atoi(argv[4]), OW = atoi(argv[5]), filter = atoi(argv[6]);
  if (H < 1 || W < 1 || OH < 1 || OW < 1 || H > 8192 || W > 8192 || OH > 8192 || OW > 8192 ||
      (filter != kFilterBilinear && filter != kFilterBicubic))
    return 2;
  const size_t nin = (size_t)H * W * 3, nout = (size_t)OH * OW * 3;
  uint8_t *src = (uint8_t *)malloc(nin), *dst = (uint8_t *)malloc(nout);
  FILE *f = fopen(argv[7], "rb");
  if (!f || fread(src, 1, nin, f) != nin) return 2;
  fclose(f);
  const int rc = filter == kFilterBicubic ? resize<kFilterBicubic>(H, W, OH, OW, src, dst)
                                          : resize<kFilterBilinear>(H, W, OH, OW, src, dst);
  if (rc) return rc;
  f = fopen(argv[8], "wb");
  if (!f || fwrite(dst, 1, nout, f) != nout) return 2;
  fclose(f);
  free(dst);
  free(src);
  printf("resize ok\n");
  return 0;
}
