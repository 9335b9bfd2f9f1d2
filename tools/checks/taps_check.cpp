// taps_check.cpp — host check of the real tap counts k_resize4 is sized by
// (csrc/ldt_resample.hpp resample_taps_host) and of the geometry that follows
// from them (csrc/ldt_geom4.hpp make_geom4), built with ASan/UBSan by
// tests/test_resize4_taps.py:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off \
//       -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ tools/checks/taps_check.cpp -o taps_check
//
// For every input size 1..1120 and every output size of kOuts it checks that
//   - resample_taps_host is the largest count resample_coeffs returns,
//   - a row computed with Pillow's ksize is zero from its count on (so a
//     kernel that stops at the real count drops only products with zero),
//   - taps <= ksize and taps <= floor(2 * support) + 1,
// and, where the band kernel serves the pair (at most kResampTaps of Pillow's
// taps), with the size as a height: for every band height make_geom4 can choose
// and both kinds of source, a replay of the kernel's schedule (row pairs from
// the band's first row, for JPEG sources the even row at or below it;
// vertical(y), then horizontal(y)) in which every ring row an output row reads
// still holds the source row it needs; with the size as a width: every staged
// dword the horizontal taps read lies inside the wave's own LDS bytes and every
// staged dword written inside the row's stride. Last, the flagship geometry:
// 512 x 512 -> 224 x 224 takes 9,472 B per wave and four 4-wave workgroups
// fit the CU's 160 KB.
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

static const int kOuts[] = {1, 7, 96, 224, 255, 256};
static long g_windows = 0, g_replays = 0, g_reads = 0;

struct Windows {
  std::vector<int> xmin, cnt;
  int taps = 0;
};

// Every window of (in -> out), each row computed with Pillow's ksize.
static Windows windows_of(int in, int out) {
  const int ksize = resample_ksize_host(in, out);
  std::vector<int32_t> k((size_t)ksize);
  Windows w;
  w.xmin.resize((size_t)out);
  w.cnt.resize((size_t)out);
  for (int xx = 0; xx < out; ++xx) {
    int xmin = -1;
    const int n = resample_coeffs<kFilterBilinear>(in, out, xx, ksize, k.data(), &xmin);
    CHECK(n >= 1 && n <= ksize && xmin >= 0 && xmin + n <= in, "%d -> %d index %d: window %d + %d", in, out, xx, xmin, n);
    for (int t = n; t < ksize; ++t) CHECK(k[(size_t)t] == 0, "%d -> %d index %d: weight %d of count %d is %d", in, out, xx, t, n, k[(size_t)t]);
    w.xmin[(size_t)xx] = xmin;
    w.cnt[(size_t)xx] = n;
    if (n > w.taps) w.taps = n;
    ++g_windows;
  }
  return w;
}

// The kernel's schedule for one band height: no ring row is overwritten while
// an unfinished output row still needs it.
static void replay(const Windows &v, int in, int oh, const Geom4 &g, bool jpeg) {
  std::vector<int> owner((size_t)g.ring);
  for (int band = 0; band < g.nbands; ++band) {
    const int oy0 = band * g.bh, nb = g.bh < oh - oy0 ? g.bh : oh - oy0;
    CHECK(nb >= 1, "empty band");
    const int ya = v.xmin[(size_t)oy0], yb = v.xmin[(size_t)(oy0 + nb - 1)] + v.cnt[(size_t)(oy0 + nb - 1)];
    const int ya0 = jpeg ? (ya & ~1) : ya;
    for (int &o : owner) o = -1;
    int next = 0, slot = 0;
    auto vertical = [&](int done) {
      while (next < nb) {
        const int ymin = v.xmin[(size_t)(oy0 + next)], cnt = v.cnt[(size_t)(oy0 + next)];
        if (ymin + cnt > done) break;
        const int s0 = (ymin - ya0) % g.ring;
        for (int t = 0; t < cnt; ++t) {
          const int sl = s0 + t < g.ring ? s0 + t : s0 + t - g.ring;
          CHECK(owner[(size_t)sl] == ymin + t, "%d -> %d bh %d ring %d jpeg %d: output row %d tap %d reads source row %d, slot holds %d",
                in, oh, g.bh, g.ring, (int)jpeg, oy0 + next, t, ymin + t, owner[(size_t)sl]);
        }
        ++next;
      }
    };
    auto horizontal = [&](int y) {
      for (int r = 0; r < 2; ++r) {
        // what the slot held is gone: no pending output row may still need it
        if (next < nb && owner[(size_t)slot] >= 0)
          CHECK(owner[(size_t)slot] < v.xmin[(size_t)(oy0 + next)], "%d -> %d bh %d ring %d: row %d overwritten, output row %d pending",
                in, oh, g.bh, g.ring, owner[(size_t)slot], oy0 + next);
        owner[(size_t)slot] = y + r;
        slot = slot + 1 == g.ring ? 0 : slot + 1;
      }
    };
    for (int y = ya0; y < yb; y += 2) {
      vertical(y);
      horizontal(y);
    }
    vertical(yb + 1);
    CHECK(next == nb, "%d -> %d bh %d: band %d finished %d of %d rows", in, oh, g.bh, band, next, nb);
    ++g_replays;
  }
}

// The staged dwords a wave reads and writes for a width `in`, output width ow.
static void staging(const Windows &h, int in, int ow, const Geom4 &g, int ks, bool jpeg) {
  const long wave_dwords = g.wave_bytes / 4;
  CHECK(g.spad % 4 == 0 && g.wave_bytes % 16 == 0, "spad %d wave %d", g.spad, g.wave_bytes);
  // writes: JPEG rows whole 8-pixel blocks, raw rows whole skewed 16-pixel blocks
  if (jpeg) {
    CHECK((in + 7) / 8 * 8 <= g.spad, "width %d: staged blocks end at %d, stride %d", in, (in + 7) / 8 * 8, g.spad);
    // any narrower width of the same batch with these taps
    CHECK(4L * (2 * g.spad + ks) <= g.wave_bytes, "width %d ks %d: reach past wave_bytes %d", in, ks, g.wave_bytes);
  } else {
    const int x0 = (in + 15) / 16 * 16 - 16;
    CHECK(x0 + ((x0 >> 5) << 2) + 16 <= g.spad, "width %d: skewed blocks end past stride %d", in, g.spad);
  }
  for (int ox = 0; ox < ow; ++ox) {
    const int xm = h.xmin[(size_t)ox];
    for (int r = 0; r < 2; ++r)
      for (int t = 0; t < ks; ++t) {
        long idx;
        if (jpeg) {
          idx = xm + t;
        } else {
          const int xsk = xm + ((xm >> 5) << 2), xcr = 32 - (xm & 31);
          idx = (t < xcr ? xsk : xsk + 4) + t;
          // a tap with a weight reads the pixel's skewed dword inside its row
          if (t < h.cnt[(size_t)ox]) CHECK(idx == (xm + t) + (((xm + t) >> 5) << 2) && idx < g.spad, "skew %d + %d", xm, t);
        }
        if (t < h.cnt[(size_t)ox]) CHECK(idx < g.spad, "width %d column %d tap %d: dword %ld of stride %d", in, ox, t, idx, g.spad);
        CHECK((long)r * g.spad + idx < wave_dwords, "width %d -> %d column %d tap %d row %d: dword %ld of %ld", in, ow, ox, t, r,
              (long)r * g.spad + idx, wave_dwords);
        ++g_reads;
      }
  }
}

int main() {
  for (int out : kOuts) {
    const int vmax_in = out == kOut ? kResampMaxSize : resamp_max_in(out, kResampTableBytesV);
    const int hmax_in = out == kOut ? kResampMaxSize : resamp_max_in(out, kResampTableBytesH);
    for (int in = 1; in <= kResampMaxSize; ++in) {
      const Windows w = windows_of(in, out);
      const int ksize = resample_ksize_host(in, out);
      const int taps = resample_taps_host(in, out);
      CHECK(taps == w.taps, "%d -> %d: taps %d, largest count %d", in, out, taps, w.taps);
      // floor(2 * support) + 1, support = max(in / out, 1)
      const int bound = in > out ? (2 * in) / out + 1 : 3;
      CHECK(taps <= ksize && taps <= bound, "%d -> %d: taps %d ksize %d bound %d", in, out, taps, ksize, bound);
      if (ksize > kResampTaps) continue; // not the band kernel's
      const int ks = resize4_taps(taps);
      CHECK(ks >= taps && ks <= kResampTaps && ks >= 3, "%d -> %d: KS %d for %d taps", in, out, ks, taps);
      // as a height: the ring under every band height, both kinds of source
      const int ks_v = resamp_cached(in, out, vmax_in) ? taps : ksize;
      int last_bh = -1;
      for (int nb = 1; nb <= (out + 7) / 8; ++nb) {
        for (int jpeg = 0; jpeg < 2; ++jpeg) {
          Geom4 g{};
          make_geom4(1, 64, in, 3, ks_v, nb, g, 1, jpeg != 0, out, out, vmax_in);
          CHECK(g.ring == ks_v + 1 && g.ks_v == ks_v, "ring %d ks_v %d", g.ring, g.ks_v);
          if (g.bh == last_bh) continue; // the same bands as the last count
          replay(w, in, out, g, jpeg != 0);
          if (jpeg) last_bh = g.bh;
        }
      }
      // as a width: reads and writes of the staging rows, beside the smallest
      // ring (a one-row source) and a square source's
      if (!resamp_cached(in, out, hmax_in)) continue;
      for (int jpeg = 0; jpeg < 2; ++jpeg)
        for (int hh : {1, in}) {
          Geom4 g{};
          const int tv = hh == 1 ? 1 : ks_v;
          if (!make_geom4(1, in, hh, ks, tv, 1, g, 1, jpeg != 0, out, out, vmax_in)) continue;
          staging(w, in, out, g, ks, jpeg != 0);
        }
    }
  }
  // heights past the cache (Geom4::vcalc): Pillow's capacity, as before
  for (int in : {1121, 1200, 2000, 2463}) {
    const Windows w = windows_of(in, kOut);
    const int ksize = resample_ksize_host(in, kOut);
    for (int nb = 1; nb <= 28; ++nb) {
      Geom4 g{};
      make_geom4(1, 64, in, 3, ksize, nb, g, 1, true, kOut, kOut, kResampMaxSize);
      CHECK(g.vcalc == 1 && g.ring == ksize + 1, "vcalc geometry of height %d", in);
      replay(w, in, kOut, g, true);
    }
  }
  // the flagship shape: 256 images of 512 x 512, 5 real taps of Pillow's 7 on both axes
  {
    CHECK(resample_ksize_host(512, kOut) == 7 && resample_taps_host(512, kOut) == 5, "512 -> 224: %d taps",
          resample_taps_host(512, kOut));
    Geom4 g{};
    CHECK(make_geom4(256, 512, 512, 5, 5, 256 * 16, g, 4, true), "c2 geometry refused");
    CHECK(g.spad == 512 && g.ring == 6 && g.wave_bytes == 9472, "c2: spad %d ring %d wave %d", g.spad, g.ring, g.wave_bytes);
    const int wg = kResize4Lut + 4 * g.wave_bytes;
    CHECK(wg == 40960 && 4 * wg <= kResize4LdsMax, "c2: workgroup %d B, four of them %d B", wg, 4 * wg);
  }
  printf("taps ok: %ld windows, %ld band replays, %ld staged reads\n", g_windows, g_replays, g_reads);
  return 0;
}
