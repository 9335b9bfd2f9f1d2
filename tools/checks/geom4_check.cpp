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
//   - the ring holds ks_v + 1 rows, ks_v being the height's real tap count
//     (resample_taps_host) where it has a table entry and Pillow's capacity
//     where it has none, and a ring row is a multiple of 4 columns not narrower
//     than the output,
//   - a JPEG source's staging stride is its width in whole 8-pixel blocks and
//     the taps' reads past a row's end stay inside the wave's bytes; a raw
//     source's skewed stride holds the row and its taps,
//   - the workgroup's LDS is at most 160 KB, or the shape is refused,
//   - the per-wave LDS holds every region the kernel carves out of it,
// and that at 224 x 224 the bands equal those the kernel had while its size
// was a compile-time constant (parent_geom below, kept as the record of those
// values), plus the documented 9,472 B wave of a 512 px JPEG batch, four
// 4-wave workgroups of which fill the CU's 160 KB. tools/checks/taps_check.cpp
// replays the kernel's schedule against the ring and the staging rows.
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <utility>

#include "../../lance-distributed-training_amd/csrc/ldt_geom4.hpp"
#include "../../lance-distributed-training_amd/csrc/ldt_resample.hpp"

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

// The bands at the fixed 224 x 224 output, as they were before the size
// became a parameter, and a raw source's stride (ks_h: the kernel's taps).
struct ParentGeom {
  int nbands, bh, ntask, vcalc, spad_raw;
};
static ParentGeom parent_geom(int n, int max_w, int max_h, int ks_h, int waves_target) {
  ParentGeom p;
  p.vcalc = max_h > 1120 ? 1 : 0;
  const int px = ((max_w + 15) / 16) * 16 + ks_h + 16;
  p.spad_raw = (px + ((px >> 5) << 2) + 4 + 3) & ~3;
  int nb = (waves_target + n - 1) / n;
  if (nb < 1) nb = 1;
  if (nb > 28) nb = 28;
  p.bh = (224 + nb - 1) / nb;
  p.nbands = (224 + p.bh - 1) / p.bh;
  p.ntask = n * p.nbands;
  return p;
}

// The taps a single-size batch hands make_geom4 (ldt_resize4.hip): the width's
// real count rounded up to an instantiation; the height's real count, or
// Pillow's capacity without a table entry. Kept per (size, out): the sweep
// asks for the same few sources at every output size.
static int taps_of(int in, int out) {
  static std::map<std::pair<int, int>, int> memo;
  const auto it = memo.find({in, out});
  if (it != memo.end()) return it->second;
  return memo[{in, out}] = resample_taps_host(in, out);
}

static long g_calls = 0, g_refused = 0;

static void check_one(int n, int w, int h, int oh, int ow, int target, int wpg, bool jpeg, int vmax_in) {
  const int ks_h = resize4_taps(taps_of(w, ow));
  const int ks_v = resamp_cached(h, oh, vmax_in) ? taps_of(h, oh) : resample_ksize_host(h, oh);
  Geom4 g{};
  const bool ok = make_geom4(n, w, h, ks_h, ks_v, target, g, wpg, jpeg, oh, ow, vmax_in);
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
  CHECK(g.ks_v == ks_v && g.ks_v <= resample_ksize_host(h, oh) && g.ring == g.ks_v + 1, "ring %d ks_v %d", g.ring, g.ks_v);
  CHECK(g.ows % 4 == 0 && g.ows >= ow && g.ows < ow + 4, "ow %d ows %d", ow, g.ows);
  if (jpeg) {
    // whole 8-pixel blocks; the second row's last tap inside the wave
    CHECK(g.spad == (w + 7) / 8 * 8, "spad %d for width %d", g.spad, w);
    CHECK(4 * (2 * g.spad + ks_h) <= g.wave_bytes, "width %d, %d taps: reach past wave_bytes %d", w, ks_h, g.wave_bytes);
  } else {
    CHECK(g.spad % 4 == 0 && g.spad >= w + ks_h, "spad %d for width %d", g.spad, w);
  }
  // a height without a table entry has room for computed coefficients
  CHECK((g.vcalc != 0) == !resamp_cached(h, oh, vmax_in), "vcalc %d for %d -> %d", g.vcalc, h, oh);
  // the wave's LDS regions, in the kernel's order: two staging rows, the ring, kv + vb
  const size_t need = 8u * (size_t)g.spad + (size_t)(jpeg ? 4 : 3) * g.ring * g.ows +
                      (g.vcalc ? 4u * (size_t)(kKvRows * g.ks_v + 2 * kKvRows) : 0u);
  CHECK((size_t)g.wave_bytes >= need && g.wave_bytes % 16 == 0, "wave_bytes %d < %zu", g.wave_bytes, need);
  if (oh == 224 && ow == 224 && vmax_in == kResampMaxSize) {
    const ParentGeom p = parent_geom(n, w, h, ks_h, target);
    CHECK(p.nbands == g.nbands && p.bh == g.bh && p.ntask == g.ntask && p.vcalc == g.vcalc &&
              (jpeg || p.spad_raw == g.spad),
          "224x224 differs from the fixed-size geometry: n %d src %dx%d target %d wpg %d jpeg %d", n, h, w, target,
          wpg, (int)jpeg);
  }
}

int main() {
  static const int kSrc[][2] = {{1, 1},     {64, 48},    {500, 375},  {512, 512},
                                {1024, 1024}, {1120, 1300}, {333, 8192}, {1280, 5000}}; // (w, h)
  static const int kN[] = {1, 7, 256};
  static const int kTarget[] = {1, 3072};
  // a 512 px JPEG batch has 5 real taps of Pillow's 7 on both axes; its wave is 9,472 B, four
  // of them and the LUT per workgroup, four workgroups per CU
  {
    Geom4 g{};
    CHECK(taps_of(512, kOut) == 5, "512 -> 224 has %d taps", taps_of(512, kOut));
    CHECK(make_geom4(256, 512, 512, 5, 5, 3072, g, 4, true), "c2 geometry refused");
    CHECK(g.spad == 512 && g.ring == 6 && g.wave_bytes == 9472 && g.bh == 19 && g.nbands == 12,
          "c2 geometry: spad %d ring %d wave %d bh %d nbands %d", g.spad, g.ring, g.wave_bytes, g.bh, g.nbands);
    CHECK(4 * (kResize4Lut + 4 * g.wave_bytes) <= kResize4LdsMax, "four c2 workgroups: %d B", 4 * (kResize4Lut + 4 * g.wave_bytes));
    CHECK(make_geom4(256, 512, 512, 5, 5, 4096, g, 4, true) && g.bh == 14 && g.nbands == 16, "c2 at 16 waves per CU");
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
