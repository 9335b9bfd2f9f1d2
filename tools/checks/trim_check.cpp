// trim_check.cpp — host check of the two things k_resize4 (csrc/ldt_resize4.hip)
// relies on since it dropped its clamps and stopped staging boundary rows
// nobody reads, built with ASan/UBSan by tests/test_resize4_trim.py:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off \
//       -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ tools/checks/trim_check.cpp -o trim_check
//
// 1. No clip8. With resample_coeffs (csrc/ldt_resample.hpp, BILINEAR) every
//    weight is >= 0 and every row of weights sums to at most kMaxRowSum =
//    4,202,528 = floor((256 * 2^22 - 2^21 - 1) / 255): then 255 * sum + 2^21 <
//    256 * 2^22 and bits 22..29 of a tap sum are the byte, whatever bytes the
//    taps read. (The bound first proposed for this check, 4,202,554, is too
//    lax: 255 * 4,202,554 + 2^21 > 2^30. The largest sum found is printed.)
//    Swept: every input 1..1120 at output 224 and at every other output size
//    of kOuts (those the tests and workloads use, and the table limits), over
//    every input the tables of that output admit (resamp_cached, horizontal
//    or vertical); a strided sweep of the remaining (input, output) pairs,
//    outputs 1..1024 in steps of 29 and inputs in steps of 13 from a start
//    that moves with the output; and heights past the tables (computed
//    vertical coefficients), up to 75 taps.
// 2. Row skipping. With make_geom4 (csrc/ldt_geom4.hpp) and the same windows,
//    for every band of every band height the geometry can choose and both
//    kinds of source: the kernel stages row pairs y, y + 1 from the band's
//    first row ya (JPEG: the even row at or below it) while y < yb and skips
//    row y when y < ya and row y + 1 when y + 1 >= yb. Every skipped row lies
//    outside [ymin, ymin + cnt) of every output row of the band, every row
//    inside some window is staged, and every staged row is a row of the image.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../lance-distributed-training_amd/csrc/ldt_geom4.hpp"
#include "../../lance-distributed-training_amd/csrc/ldt_resample.hpp"

using namespace ldt;

#define CHECK(c, ...)                   \
  do {                                  \
    if (!(c)) {                         \
      fprintf(stderr, "FAIL %s: ", #c); \
      fprintf(stderr, __VA_ARGS__);     \
      fprintf(stderr, "\n");            \
      exit(1);                          \
    }                                   \
  } while (0)

constexpr int64_t kMaxRowSum = 4202528;
static_assert(255 * kMaxRowSum + (1 << (kPrecisionBits - 1)) < ((int64_t)256 << kPrecisionBits), "the bound");
static_assert(255 * (kMaxRowSum + 1) + (1 << (kPrecisionBits - 1)) >= ((int64_t)256 << kPrecisionBits), "and no smaller one");

static const int kOuts[] = {1, 7, 32, 64, 96, 128, 160, 192, 224, 250, 255, 256, 384, 512, 1024};
static long g_rows = 0, g_pairs = 0, g_bands = 0, g_skipped = 0;
static int64_t g_max_sum = 0;

struct Windows {
  std::vector<int> ymin, cnt;
};

// Every window of (in -> out) with Pillow's ksize; part 1's checks on the way.
static Windows windows_of(int in, int out) {
  const int ksize = resample_ksize_host(in, out);
  std::vector<int32_t> k((size_t)ksize);
  Windows w;
  w.ymin.resize((size_t)out);
  w.cnt.resize((size_t)out);
  for (int xx = 0; xx < out; ++xx) {
    int xmin = -1;
    const int n = resample_coeffs<kFilterBilinear>(in, out, xx, ksize, k.data(), &xmin);
    CHECK(n >= 1 && n <= ksize && xmin >= 0 && xmin + n <= in, "%d -> %d index %d: window %d + %d", in, out, xx, xmin, n);
    int64_t sum = 0;
    for (int t = 0; t < ksize; ++t) {
      CHECK(k[(size_t)t] >= 0, "%d -> %d index %d: weight %d is %d", in, out, xx, t, k[(size_t)t]);
      sum += k[(size_t)t];
    }
    CHECK(sum <= kMaxRowSum, "%d -> %d index %d: weights sum to %lld", in, out, xx, (long long)sum);
    if (sum > g_max_sum) g_max_sum = sum;
    w.ymin[(size_t)xx] = xmin;
    w.cnt[(size_t)xx] = n;
    ++g_rows;
  }
  ++g_pairs;
  return w;
}

// Part 2 for one geometry: the rows each band stages against its windows.
static void bands(const Windows &v, int in, int oh, const Geom4 &g, bool jpeg) {
  std::vector<char> staged, skipped;
  for (int band = 0; band < g.nbands; ++band) {
    const int oy0 = band * g.bh, nb = g.bh < oh - oy0 ? g.bh : oh - oy0;
    CHECK(nb >= 1, "empty band");
    const int ya = v.ymin[(size_t)oy0], yb = v.ymin[(size_t)(oy0 + nb - 1)] + v.cnt[(size_t)(oy0 + nb - 1)];
    const int ya0 = jpeg ? (ya & ~1) : ya;
    CHECK(ya0 >= 0 && yb <= in && ya < yb, "%d -> %d band %d: rows %d .. %d", in, oh, band, ya, yb);
    // rows ya0 .. yb (one past the last pair's second row at most)
    staged.assign((size_t)(yb + 2 - ya0), 0);
    skipped.assign((size_t)(yb + 2 - ya0), 0);
    for (int y = ya0; y < yb; y += 2) {
      const bool need0 = y >= ya, need1 = y + 1 < yb;
      CHECK(need0 || need1, "%d -> %d band %d: pair %d has no row", in, oh, band, y);
      (need0 ? staged : skipped)[(size_t)(y - ya0)] = 1;
      (need1 ? staged : skipped)[(size_t)(y + 1 - ya0)] = 1;
      if (need0) CHECK(y < in, "%d -> %d band %d: row %d staged", in, oh, band, y);
      if (need1) CHECK(y + 1 < in, "%d -> %d band %d: row %d staged", in, oh, band, y + 1);
      g_skipped += !need0 + !need1;
    }
    for (int j = 0; j < nb; ++j) {
      const int ymin = v.ymin[(size_t)(oy0 + j)], cnt = v.cnt[(size_t)(oy0 + j)];
      CHECK(ymin >= ya && ymin + cnt <= yb, "%d -> %d band %d row %d: window %d + %d outside %d .. %d", in, oh, band, j, ymin,
            cnt, ya, yb);
      for (int t = 0; t < cnt; ++t) {
        const int y = ymin + t - ya0;
        CHECK(staged[(size_t)y] && !skipped[(size_t)y], "%d -> %d bh %d jpeg %d band %d: output row %d reads row %d, not staged", in,
              oh, g.bh, (int)jpeg, band, oy0 + j, ymin + t);
      }
    }
    ++g_bands;
  }
}

static void heights(const Windows &w, int in, int out, int ks_v, int vmax_in) {
  int last_bh = -1;
  for (int nb = 1; nb <= (out + 7) / 8; ++nb)
    for (int jpeg = 0; jpeg < 2; ++jpeg) {
      Geom4 g{};
      make_geom4(1, 64, in, 3, ks_v, nb, g, 1, jpeg != 0, out, out, vmax_in);
      if (g.bh == last_bh) continue; // the same bands as the last count
      bands(w, in, out, g, jpeg != 0);
      if (jpeg) last_bh = g.bh;
    }
}

static void pair(int in, int out) {
  const int vmax_in = out == kOut ? kResampMaxSize : resamp_max_in(out, kResampTableBytesV);
  const int hmax_in = out == kOut ? kResampMaxSize : resamp_max_in(out, kResampTableBytesH);
  const bool as_h = out <= kTileCols && resamp_cached(in, out, hmax_in), as_v = resamp_cached(in, out, vmax_in);
  if (!as_h && !as_v) return; // no table row of this pair is ever read
  const Windows w = windows_of(in, out);
  if (resample_ksize_host(in, out) <= kResampTaps) heights(w, in, out, as_v ? resample_taps_host(in, out) : resample_ksize_host(in, out), vmax_in);
}

int main() {
  for (int out : kOuts)
    for (int in = 1; in <= kResampMaxSize; ++in) pair(in, out);
  for (int out = 1; out <= kMaxOut; out += 29)
    for (int in = 1 + out % 13; in <= kResampMaxSize; in += 13) pair(in, out);
  // heights past the tables: coefficients computed in the kernel, up to 2 * kMaxReduce + 1 taps
  for (int in : {1121, 1200, 2000, 2463, 4095, 8191, 8288}) {
    const Windows w = windows_of(in, kOut);
    heights(w, in, kOut, resample_ksize_host(in, kOut), kResampMaxSize);
  }
  CHECK(g_skipped > 0, "no band skipped a row");
  printf("trim ok: %ld pairs, %ld weight rows (largest sum %lld of %lld), %ld bands, %ld rows skipped\n", g_pairs, g_rows,
         (long long)g_max_sum, (long long)kMaxRowSum, g_bands, g_skipped);
  return 0;
}
