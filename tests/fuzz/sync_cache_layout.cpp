// Stand-alone driver of csrc/ldt_sync_cache.hpp (tests/test_sync_cache_layout.py
// builds it with -fsanitize=address,undefined): the table's index arithmetic
// and the validation every hint passes before k_huff_image uses it, on random
// and boundary geometries. Prints "ok <checks>" and exits 0, or prints the
// failed check and exits 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "ldt_sync_cache.hpp"

using namespace ldt;

static long g_checks = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    ++g_checks;                                                       \
    if (!(c)) {                                                       \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);           \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

constexpr int kRecCap = 8192; // ldt_huffman.hip: block records an image keeps in LDS

// Budget -> sets -> byte ranges: every header and payload inside the table,
// no two overlapping. The table itself is modelled by a byte vector the
// ranges are touched in (the sanitizer sees any range outside it).
static void check_budget(int64_t bytes, bool touch) {
  const int64_t sets = sc_sets(bytes);
  CHECK(sets >= 0 && sets <= kScMaxSets);
  CHECK(sets * kScSetBytes <= bytes || sets == 0 || sets == kScMaxSets);
  if (bytes < kScSetBytes) CHECK(sets == 0);
  if (sets == 0) return;
  const int64_t total = sc_table_bytes(sets);
  CHECK(sc_off_headers() == kScStats * 8);
  CHECK(sc_off_headers() % 64 == 0); // a set's four headers: one 64-byte line
  CHECK(sc_off_payloads(sets) == sc_off_headers() + sets * 64);
  CHECK(total == sc_off_payloads(sets) + sc_entries(sets) * kScPayloadBytes);
  if (!touch) return;
  std::vector<uint8_t> table((size_t)total, 0);
  for (int64_t e = 0; e < sc_entries(sets); ++e) {
    uint8_t *h = table.data() + sc_off_headers() + e * (int64_t)sizeof(ScHeader);
    uint8_t *p = table.data() + sc_off_payloads(sets) + e * kScPayloadBytes;
    for (size_t i = 0; i < sizeof(ScHeader); ++i) h[i]++;
    p[0]++;
    p[kScPayloadBytes - 1]++;
  }
  for (int64_t e = 0; e < sc_entries(sets); ++e) {
    const uint8_t *h = table.data() + sc_off_headers() + e * (int64_t)sizeof(ScHeader);
    const uint8_t *p = table.data() + sc_off_payloads(sets) + e * kScPayloadBytes;
    CHECK(h[0] == 1 && h[15] == 1 && p[0] == 1 && p[kScPayloadBytes - 1] == 1); // touched once: disjoint
  }
}

struct Seg {
  int32_t bits;
  int mcu_count;
};

// One image: segments cut into slots of S bits; hints built as a converged
// decode leaves them, then checked the way image_decode consumes them.
static void check_image(std::mt19937_64 &rng, int S, const std::vector<Seg> &segs, int bpm, bool full) {
  const int b3end = 3 * bpm;
  std::vector<int> seg_first;
  int slots = 0;
  for (const Seg &s : segs) {
    seg_first.push_back(slots);
    const int cnt = (s.bits + S - 1) / S;
    slots += cnt < 1 ? 1 : cnt;
  }
  seg_first.push_back(slots);
  if (slots > kScSlots) return;
  const int nseg = (int)segs.size();
  const uint32_t geom = sc_geom(S, slots, nseg);
  CHECK((int)(geom & 0xFFFu) << 5 == S);
  CHECK((int)((geom >> 12) & 0x3FFu) + 1 == slots);
  CHECK((int)((geom >> 22) & 0xFFu) + 1 == nseg);
  int64_t blocks = 0;
  for (const Seg &s : segs) blocks += (int64_t)s.mcu_count * bpm;
  for (uint32_t st : {kScEmpty, kScWriting, kScReady}) {
    const uint64_t m = sc_meta(geom, st, blocks);
    CHECK(sc_meta_state(m) == st);
    CHECK((uint32_t)m == geom);
    CHECK((int64_t)(m >> 34) == blocks);
  }
  // converged hints
  std::vector<ScSlot> h((size_t)slots);
  for (int si = 0; si < nseg; ++si) {
    const int cnt = seg_first[si + 1] - seg_first[si];
    int64_t left = (int64_t)segs[si].mcu_count * bpm;
    for (int j = 0; j < cnt; ++j) {
      const int64_t end = (int64_t)(j + 1) * S;
      const int64_t stop = end < segs[si].bits ? end : segs[si].bits;
      ScSlot &x = h[(size_t)(seg_first[si] + j)];
      x.ex_p = (int32_t)(stop + (int64_t)(rng() % 32));
      const uint32_t b3 = 3 * (uint32_t)(rng() % bpm), k = (uint32_t)(rng() % 64);
      // (the last slot's count steps take the segment's pad bits for blocks)
      int64_t n = j == cnt - 1 ? left + (int64_t)(rng() % 3) : (int64_t)(rng() % (uint64_t)(left + 1));
      if (n > 0xFFFF) n = 0xFFFF;
      if (j == cnt - 1 && n < left) return; // more blocks than 16 bits count: not a decodable layout
      left -= j == cnt - 1 ? left : n;
      x.bk_n = ((b3 << 8) | k) | ((uint32_t)n << 16);
    }
  }
  auto plausible = [&](const std::vector<ScSlot> &v) {
    for (int si = 0; si < nseg; ++si) {
      const int cnt = seg_first[si + 1] - seg_first[si];
      int64_t sum = 0; // over all slots but the last
      for (int j = 0; j < cnt; ++j) {
        const ScSlot &x = v[(size_t)(seg_first[si] + j)];
        if (!hints_plausible(x.ex_p, x.bk_n & 0xFFFFu, j, cnt, S, segs[si].bits, b3end)) return false;
        if (j < cnt - 1) sum += x.bk_n >> 16;
      }
      if (!hints_sum_ok(sum, segs[si].mcu_count, bpm)) return false;
    }
    return true;
  };
  CHECK(plausible(h));
  // what the write pass derives from accepted hints stays inside the image:
  // entry positions inside the segment's bits (+31), first blocks and limits
  // inside the segment's blocks, units inside its 8 per block
  int64_t seg_block0 = 0;
  for (int si = 0; si < nseg; ++si) {
    const int cnt = seg_first[si + 1] - seg_first[si];
    const int64_t total = (int64_t)segs[si].mcu_count * bpm;
    int64_t bstart = 0;
    for (int j = 0; j < cnt; ++j) {
      const ScSlot &x = h[(size_t)(seg_first[si] + j)];
      if (j > 0) {
        const ScSlot &pr = h[(size_t)(seg_first[si] + j - 1)];
        CHECK(pr.ex_p >= 0 && pr.ex_p <= segs[si].bits + 31); // the reader's seek
        CHECK(pr.ex_p >= (int64_t)j * S || pr.ex_p >= segs[si].bits);
      }
      const int64_t base = seg_block0 + bstart, lim = total - bstart;
      CHECK(bstart >= 0 && bstart <= total && lim >= 0);
      CHECK(base >= seg_block0 && base + lim == seg_block0 + total);
      CHECK(base * 8 + lim * 8 <= blocks * 8);
      if (j < cnt - 1) CHECK(x.ex_p <= segs[si].bits + 31); // the lane's stop
      bstart += x.bk_n >> 16;
    }
    seg_block0 += total;
  }
  if (!full) return;
  // every single-field damage outside the ranges is rejected
  for (int q = 0; q < slots; ++q) {
    int si = 0;
    while (seg_first[si + 1] <= q) ++si;
    const int cnt = seg_first[si + 1] - seg_first[si], j = q - seg_first[si];
    const bool last = j == cnt - 1;
    std::vector<ScSlot> v(h);
    const int64_t end = (int64_t)(j + 1) * S;
    const int64_t stop = end < segs[si].bits ? end : segs[si].bits;
    v[(size_t)q].ex_p = (int32_t)(stop + 32);
    CHECK(plausible(v) == last); // a last slot's exit position is never used
    v[(size_t)q].ex_p = (int32_t)(stop - 1);
    CHECK(plausible(v) == last);
    v[(size_t)q].ex_p = 0x7FFFFFF0;
    CHECK(plausible(v) == last);
    v[(size_t)q].ex_p = -1;
    CHECK(plausible(v) == last);
    v = h;
    v[(size_t)q].bk_n = (v[(size_t)q].bk_n & 0xFFFF0000u) | ((uint32_t)b3end << 8);
    CHECK(!plausible(v)); // block phase at the MCU's block count
    v = h;
    v[(size_t)q].bk_n = (v[(size_t)q].bk_n & 0xFFFF0000u) | 64u;
    CHECK(!plausible(v)); // k = 64
    if (bpm > 1) {
      v = h;
      v[(size_t)q].bk_n = (v[(size_t)q].bk_n & 0xFFFF0000u) | (1u << 8);
      CHECK(!plausible(v)); // b3 not a multiple of 3
    }
    // block counts: the slots before the last may not claim more than the
    // segment has; the last slot's count is read by nothing
    const int64_t total = (int64_t)segs[si].mcu_count * bpm;
    int64_t before = 0;
    for (int i = 0; i < cnt - 1; ++i) before += h[(size_t)(seg_first[si] + i)].bk_n >> 16;
    v = h;
    if (last) {
      v[(size_t)q].bk_n |= 0xFFFF0000u;
      CHECK(plausible(v));
    } else if (total - before + (h[(size_t)q].bk_n >> 16) + 1 <= 0xFFFF) {
      const uint32_t n = (uint32_t)(total - before + (h[(size_t)q].bk_n >> 16) + 1);
      v[(size_t)q].bk_n = (v[(size_t)q].bk_n & 0xFFFFu) | (n << 16);
      CHECK(!plausible(v)); // one block more than the segment holds
      v[(size_t)q].bk_n -= 1u << 16;
      CHECK(plausible(v)); // exactly the segment's blocks before the last slot
    }
  }
  CHECK(!hints_plausible(0, 0, -1, 1, S, 0, b3end));
  CHECK(!hints_plausible(0, 0, 1, 1, S, 0, b3end));
}

int main() {
  std::mt19937_64 rng(20261021);
  // budgets: too small for one set, exactly one, the default, the cap
  for (int64_t b : {(int64_t)0, (int64_t)1, kScSetBytes - 1, kScSetBytes, kScSetBytes + 1, 2 * kScSetBytes - 1,
                    (int64_t)1 << 20, (int64_t)3 << 20})
    check_budget(b, true);
  CHECK(sc_sets(kScSetBytes - 1) == 0 && sc_sets(kScSetBytes) == 1);
  CHECK(sc_entries(sc_sets((int64_t)1 << 20)) == 128);
  CHECK(sc_entries(sc_sets((int64_t)1024 << 20)) == 131072);
  check_budget((int64_t)1024 << 20, false);
  check_budget((int64_t)65536 << 20, false);
  check_budget(INT64_MAX, false);
  CHECK(sc_sets(INT64_MAX) == kScMaxSets);
  CHECK(sc_sets(-5) == 0);
  // the set index stays below the set count
  for (int64_t sets : {(int64_t)1, (int64_t)2, (int64_t)3, (int64_t)32, (int64_t)32768, kScMaxSets}) {
    for (int i = 0; i < 20000; ++i) {
      const int64_t s = sc_set_index(rng(), sets);
      CHECK(s >= 0 && s < sets);
    }
    CHECK(sc_set_index(0, sets) == 0);
    CHECK(sc_set_index(~0ull, sets) == sets - 1);
  }
  // keys: the length and the geometry are part of them
  CHECK(sc_key(1, 100, 5) != sc_key(1, 101, 5));
  CHECK(sc_key(1, 100, 5) != sc_key(1, 100, 6));
  CHECK(sc_key(1, 100, 5) != sc_key(2, 100, 5));
  // boundary geometries: slot counts 1, 2, 1023, 1024; 1 and 256 segments; a
  // segment of a single slot; block counts at kRecCap and above
  check_image(rng, 64, {{40, 1}}, 1, true);                 // one slot
  check_image(rng, 64, {{0, 1}}, 3, true);                  // an empty segment still owns a slot
  check_image(rng, 64, {{100, 2}}, 6, true);                // two slots
  check_image(rng, 64, {{64 * 1023, 400}}, 6, true);        // 1023 slots
  check_image(rng, 64, {{64 * 1024, 400}}, 6, true);        // 1024 slots
  check_image(rng, 64, {{64 * 1024 - 63, 1}}, 10, true);    // 1024, the last one bit long
  check_image(rng, 32768, {{32768 * 3, kRecCap / 6}}, 6, true);
  check_image(rng, 1088, {{540000, kRecCap}}, 1, true);     // blocks at kRecCap
  check_image(rng, 1088, {{540000, kRecCap + 1}}, 1, true); // ... and above
  check_image(rng, 4000 - 32, {{3000000, 180000}}, 6, true);
  {
    std::vector<Seg> s256(256, Seg{190, 3}); // 256 segments, most of them a single slot
    s256[7].bits = 1000;
    s256[255].bits = 64 * 40;
    check_image(rng, 256 + 32, s256, 6, true);
    std::vector<Seg> tight(256, Seg{256, 1}); // 256 x 4 slots = 1024
    check_image(rng, 64, tight, 4, true);
  }
  // random geometries
  for (int it = 0; it < 3000; ++it) {
    const int S = 32 * (2 + (int)(rng() % 1023));
    const int nseg = 1 + (int)(rng() % (it % 7 == 0 ? 256 : 6));
    const int bpm = 1 + (int)(rng() % 10);
    std::vector<Seg> segs;
    for (int s = 0; s < nseg; ++s)
      segs.push_back(Seg{(int32_t)(rng() % (uint64_t)(S * (1 + 1000 / nseg))), 1 + (int)(rng() % 900)});
    check_image(rng, S, segs, bpm, it % 16 == 0);
  }
  printf("ok %ld\n", g_checks);
  return 0;
}
