// geom4_check.cpp — host check of k_resize4's launch geometry
// (csrc/ldt_geom4.hpp make_geom4) for every output size, built with
// ASan/UBSan by tests/test_output_size.py:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ tools/checks/geom4_check.cpp -o geom4_check
//
// For every out_h, out_w in 1..1024, representative sources, batch sizes,
// wave targets and waves per workgroup it checks that
//   - the bands cover each output row exactly once,
//   - the ring holds at least ks_v + 1 rows and a ring row is a multiple of 4
//     columns not narrower than the output,
//   - the workgroup's LDS is at most 160 KB, or the shape is refused,
//   - the per-wave LDS holds every region the kernel carves out of it,
// and that at 224 x 224 the result equals the geometry the kernel had while
// its size was a compile-time constant (parent_geom below, kept as the record
// of those values, plus the documented 11.2 KB wave of a 512 px JPEG batch).
#include <stdio.h>
#include <stdlib.h>

#include "../../lance-distributed-training_amd/csrc/ldt_geom4.hpp"

using namespace ldt;

#define CHECK(c, ...)                  \
  do {                                 \
    if (!(c)) {                        \
      fprintf(stderr, "FAIL %s: ", #c); \
      fprintf(stderr, __VA_ARGS__);    \
      fprintf(stderr, "\n");           \
      exit(1);                         \
    }                                  \
  } while (0)

// The geometry at the fixed 224 x 224 output, as it was before the size
// became a parameter.
struct ParentGeom {
  int nbands, bh, ring, ks_v, spad, ntask, wave_bytes, vcalc;
  bool fits;
};
static ParentGeom parent_geom(int n, int max_w, int max_h, int ks_h, int waves_target, int wpg, bool jpeg) {
  ParentGeom p;
  p.ks_v = resample_ksize_host(max_h, 224);
  p.vcalc = max_h > 1120 ? 1 : 0;
  p.ring = p.ks_v + 1;
  const int px = ((max_w + 15) / 16) * 16 + ks_h + 16;
  p.spad = (px + (jpeg ? 0 : (px >> 5) << 2) + 4 + 3) & ~3;
  const int b = 8 * p.spad + (jpeg ? 4 : 3) * p.ring * 224 + (p.vcalc ? 4 * (8 * p.ks_v + 2 * 8) : 0);
  p.wave_bytes = (b + 15) & ~15;
  int nb = (waves_target + n - 1) / n;
  if (nb < 1) nb = 1;
  if (nb > 28) nb = 28;
  p.bh = (224 + nb - 1) / nb;
  p.nbands = (224 + p.bh - 1) / p.bh;
  p.ntask = n * p.nbands;
  p.fits = 3072 + wpg * (size_t)p.wave_bytes <= 160 * 1024;
  return p;
}

static long g_calls = 0, g_refused = 0;

static void check_one(int n, int w, int h, int oh, int ow, int target, int wpg, bool jpeg, int vmax_in) {
  const int ks_h = resample_ksize_host(w, ow);
  Geom4 g{};
  const bool ok = make_geom4(n, w, h, ks_h, target, g, wpg, jpeg, oh, ow, vmax_in);
  ++g_calls;
  const size_t lds = kResize4Lut + (size_t)wpg * (size_t)g.wave_bytes;
  CHECK(ok == (lds <= (size_t)kResize4LdsMax), "%dx%d -> %dx%d: fits=%d lds=%zu", h, w, oh, ow, (int)ok, lds);
  if (!ok) ++g_refused;
  // bands: every output row exactly once
  CHECK(g.bh >= 1 && g.nbands >= 1, "oh %d: bh %d nbands %d", oh, g.bh, g.nbands);
  // (band b writes rows [b * bh, b * bh + nb) as the kernel computes them:
  // consecutive, none empty, ending at oh)
  int next_row = 0;
  for (int band = 0; band < g.nbands; ++band) {
    const int oy0 = band * g.bh, nb = (g.bh < oh - oy0 ? g.bh : oh - oy0);
    CHECK(nb >= 1, "oh %d: band %d of %d x %d rows is empty", oh, band, g.nbands, g.bh);
    CHECK(oy0 == next_row, "oh %d: band %d starts at row %d, the previous one ended at %d", oh, band, oy0, next_row);
    next_row = oy0 + nb;
  }
  CHECK(next_row == oh, "oh %d: the bands end at row %d", oh, next_row);
  CHECK(g.ntask == n * g.nbands, "ntask");
  // ring and row stride
  CHECK(g.ks_v == resample_ksize_host(h, oh) && g.ring >= g.ks_v + 1, "ring %d ks_v %d", g.ring, g.ks_v);
  CHECK(g.ows % 4 == 0 && g.ows >= ow && g.ows < ow + 4, "ow %d ows %d", ow, g.ows);
  CHECK(g.spad % 4 == 0 && g.spad >= w + ks_h, "spad %d for width %d", g.spad, w);
  // a height without a table entry has room for computed coefficients
  CHECK((g.vcalc != 0) == !resamp_cached(h, oh, vmax_in), "vcalc %d for %d -> %d", g.vcalc, h, oh);
  // the wave's LDS regions, in the kernel's order: two staging rows, the ring, kv + vb
  const size_t need = 8u * (size_t)g.spad + (size_t)(jpeg ? 4 : 3) * g.ring * g.ows +
                      (g.vcalc ? 4u * (size_t)(kKvRows * g.ks_v + 2 * kKvRows) : 0u);
  CHECK((size_t)g.wave_bytes >= need && g.wave_bytes % 16 == 0, "wave_bytes %d < %zu", g.wave_bytes, need);
  if (oh == 224 && ow == 224 && vmax_in == kResampMaxSize) {
    const ParentGeom p = parent_geom(n, w, h, ks_h, target, wpg, jpeg);
    CHECK(p.nbands == g.nbands && p.bh == g.bh && p.ring == g.ring && p.ks_v == g.ks_v && p.spad == g.spad &&
              p.ntask == g.ntask && p.wave_bytes == g.wave_bytes && p.vcalc == g.vcalc && p.fits == ok,
          "224x224 differs from the fixed-size geometry: n %d src %dx%d target %d wpg %d jpeg %d", n, h, w, target,
          wpg, (int)jpeg);
  }
}

int main() {
  static const int kSrc[][2] = {{1, 1},     {64, 48},    {500, 375},  {512, 512},
                                {1024, 1024}, {1120, 1300}, {333, 8192}, {1280, 5000}}; // (w, h)
  static const int kN[] = {1, 7, 256};
  static const int kTarget[] = {1, 3072};
  // a 512 px JPEG batch's wave is 11.2 KB, four of them and the LUT per workgroup
  {
    Geom4 g{};
    CHECK(make_geom4(256, 512, 512, 7, 3072, g, 4, true), "c2 geometry refused");
    CHECK(g.spad == 540 && g.ring == 8 && g.wave_bytes == 11488 && g.bh == 19 && g.nbands == 12,
          "c2 geometry: spad %d ring %d wave %d bh %d nbands %d", g.spad, g.ring, g.wave_bytes, g.bh, g.nbands);
  }
  for (int oh = 1; oh <= kMaxOut; ++oh) {
    const int vmax_in = oh == kOut ? kResampMaxSize : resamp_max_in(oh, kResampTableBytesV);
    for (int ow = 1; ow <= kMaxOut; ++ow) {
      if (ow > kTileCols) {
        // wider than the band kernel serves: one shape each, still well-formed
        const int i = (oh + ow) % 8;
        check_one(kN[(oh ^ ow) % 3], kSrc[i][0], kSrc[i][1], oh, ow, kTarget[ow & 1], 1 << (oh % 3), (ow >> 1) & 1,
                  vmax_in);
        continue;
      }
      for (const auto &s : kSrc) {
        if (resample_ksize_host(s[0], ow) > 11) continue; // the band kernel's horizontal limit
        if ((s[1] + oh - 1) / oh > kMaxReduce) continue;  // refused before any launch
        const int sel = (oh * 31 + ow * 7 + s[0]) % 6;     // rotate n, target and wpg over the sizes
        check_one(kN[sel % 3], s[0], s[1], oh, ow, kTarget[sel & 1], 1 << (sel % 3), true, vmax_in);
        check_one(kN[(sel + 1) % 3], s[0], s[1], oh, ow, kTarget[(sel + 1) & 1], 2, false, vmax_in);
      }
    }
  }
  // 224 x 224 against the fixed-size geometry, the full cross of the shapes above
  for (const auto &s : kSrc)
    for (int n : kN)
      for (int t : kTarget)
        for (int wpg : {1, 2, 4})
          for (int jpeg = 0; jpeg < 2; ++jpeg)
            if (resample_ksize_host(s[0], kOut) <= 11) check_one(n, s[0], s[1], kOut, kOut, t, wpg, jpeg != 0, kResampMaxSize);
  printf("geom4 ok: %ld geometries, %ld refused for LDS\n", g_calls, g_refused);
  return 0;
}
