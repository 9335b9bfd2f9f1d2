// Driver for the per-view output sizes of libldt's host planner
// (csrc/ldt_plan.cpp, csrc/ldt_view_index.hpp), built for the CPU with
// -fsanitize=address,undefined by tests/test_view_sizes.py and run directly.
// It calls the plan_batch that libldt.so calls, with the sizes that
// ldt_set_view_sizes hands it unchanged, and decodes every workgroup index with
// the view_work that k_resize_views calls.
//
// Input on stdin: records of [uint32 little-endian length][bytes], five
// decodable JPEG cells, the first 500 x 375. Cells, offsets, crops, windows
// and sizes live in heap buffers of exactly their size, so a read past any of
// them is an ASan report. Every check that fails prints a line and makes the
// exit status 1; "view_sizes_plan_ok" is printed at the end of a clean run.
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/ldt.h"
#include "../../lance-distributed-training_amd/csrc/ldt_plan.hpp"
#include "../../lance-distributed-training_amd/csrc/ldt_view_index.hpp"

using namespace ldt;

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      printf("FAIL %s:%d: ", #cond, __LINE__); \
      printf(__VA_ARGS__);                     \
      printf("\n");                            \
      g_fail = 1;                              \
    }                                          \
  } while (0)

struct Cells {
  uint8_t *data = nullptr;
  int64_t *off = nullptr; // rows + 1
  int64_t rows = 0;
};

template <typename T>
T *heap_copy(const std::vector<T> &v) {
  if (v.empty()) return nullptr;
  T *p = (T *)malloc(sizeof(T) * v.size());
  memcpy(p, v.data(), sizeof(T) * v.size());
  return p;
}

typedef std::vector<int32_t> Sizes; // (h, w) per view

void plan(const Cells &C, const std::vector<ldt_crop> &crops, const std::vector<ldt_window> &wins, const Sizes &sz,
          int filter, BatchPlan &B) {
  ldt_crop *hc = heap_copy(crops);
  ldt_window *hw = heap_copy(wins);
  int32_t *hs = heap_copy(sz);
  PlanOptions opt;
  opt.out_h = 211; // the context's own size: a sized plan must not read it
  opt.out_w = 3;
  opt.filter = filter;
  HuffCache cache;
  plan_batch(C.data, C.off, 0, C.rows, nullptr, opt, cache, B, hc, hw, (int)(sz.size() / 2), hs);
  // the blob with the table: laid out and written under the sanitizers too
  const PlanLayout L = plan_layout(B, false);
  uint8_t *blob = (uint8_t *)malloc(L.plan_bytes ? (size_t)L.plan_bytes : 1);
  write_plan(B, L, nullptr, nullptr, blob);
  CHECK(L.off_view + (int64_t)(sizeof(ViewDesc) * B.views.size()) <= L.plan_bytes, "the view table leaves the blob");
  free(blob);
  free(hs);
  free(hw);
  free(hc);
}

int ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
int ksize(int in, int out, int support) { return 2 * std::max(support, ceil_div((int64_t)support * in, out)) + 1; }

// The geometry table against sums recomputed here.
void check_geom(const ViewGeomTab &t, int64_t n, const Sizes &sz, const char *what) {
  const int V = (int)(sz.size() / 2);
  CHECK(t.views == V, "%s: table of %d views", what, t.views);
  const int64_t groups = (n + 7) / 8;
  int64_t pre = 0, base = 0;
  int mw = 0;
  for (int v = 0; v < V; ++v) {
    const int h = sz[2 * v], w = sz[2 * v + 1];
    const int nb = ceil_div(h, 8), nt = ceil_div(w, 256);
    const ViewGeom &g = t.g[v];
    CHECK(g.oh == h && g.ow == w && g.nb == nb && g.nt == nt, "%s view %d: %dx%d bands %d tiles %d", what, v, g.oh, g.ow,
          g.nb, g.nt);
    CHECK(g.pre0 == pre && g.pre1 == pre * groups, "%s view %d: prefixes %d %d, recomputed %lld %lld", what, v, g.pre0,
          g.pre1, (long long)pre, (long long)(pre * groups));
    CHECK(g.base == base, "%s view %d: base %lld, recomputed %lld", what, v, (long long)g.base, (long long)base);
    CHECK(g.pre0 % 8 == 0 && g.pre1 % 8 == 0, "%s view %d: a prefix is no multiple of 8", what, v);
    pre += (int64_t)8 * nb * nt;
    base += n * 3 * h * w;
    mw = std::max(mw, w);
  }
  CHECK(t.per_group == pre && t.groups == groups && t.total == pre * groups && t.elems == base && t.max_ow == mw,
        "%s: totals %d %d %lld %lld %d", what, t.per_group, t.groups, (long long)t.total, (long long)t.elems, t.max_ow);
}

// Every workgroup index of both orders: each (image, view, band, tile) with
// image < n exactly once, index % 8 == image % 8, padding decodes to image >= n.
void check_walk(const ViewGeomTab &t, int64_t n, const char *what) {
  std::vector<int64_t> first(t.views + 1, 0); // slots before view v: n * nb * nt each
  for (int v = 0; v < t.views; ++v) first[v + 1] = first[v] + n * t.g[v].nb * t.g[v].nt;
  for (int order = 0; order < 2; ++order) {
    std::vector<uint8_t> seen((size_t)first[t.views], 0);
    int64_t pad = 0, bad = 0;
    for (int64_t L = 0; L < t.total; ++L) {
      const ViewWork w = view_work(t, order, (int32_t)L);
      if (w.view < 0 || w.view >= t.views || w.band < 0 || w.band >= t.g[w.view].nb || w.tile < 0 ||
          w.tile >= t.g[w.view].nt || w.img < 0 || w.img >= 8 * (int64_t)t.groups || L % 8 != w.img % 8) {
        if (bad++ < 5)
          printf("FAIL %s order %d index %lld: image %d view %d band %d tile %d\n", what, order, (long long)L, w.img,
                 w.view, w.band, w.tile);
        g_fail = 1;
        continue;
      }
      if (w.img >= n) {
        ++pad;
        continue;
      }
      const int64_t slot = first[w.view] + ((int64_t)w.img * t.g[w.view].nb + w.band) * t.g[w.view].nt + w.tile;
      if (seen[(size_t)slot]++ && bad++ < 5) {
        printf("FAIL %s order %d index %lld: (%d, %d, %d, %d) a second time\n", what, order, (long long)L, w.img,
               w.view, w.band, w.tile);
        g_fail = 1;
      }
    }
    const int64_t hit = std::count(seen.begin(), seen.end(), 1);
    CHECK(hit == first[t.views], "%s order %d: %lld of %lld work items occur once", what, order, (long long)hit,
          (long long)first[t.views]);
    CHECK(pad == t.total - first[t.views], "%s order %d: %lld padding indices of %lld", what, order, (long long)pad,
          (long long)(t.total - first[t.views]));
  }
}

} // namespace

int main() {
  std::vector<uint8_t> all;
  std::vector<int64_t> off(1, 0);
  uint32_t len;
  while (fread(&len, 4, 1, stdin) == 1) {
    std::vector<uint8_t> cell(len);
    if (len && fread(cell.data(), 1, len, stdin) != len) return 2;
    all.insert(all.end(), cell.begin(), cell.end());
    off.push_back((int64_t)all.size());
  }
  Cells C;
  C.rows = (int64_t)off.size() - 1;
  if (C.rows != 5) return 2;
  C.data = (uint8_t *)malloc(all.size());
  memcpy(C.data, all.data(), all.size());
  C.off = (int64_t *)malloc(sizeof(int64_t) * off.size());
  memcpy(C.off, off.data(), sizeof(int64_t) * off.size());
  const size_t n = (size_t)C.rows;

  int32_t *wh = (int32_t *)malloc(8 * n), *st = (int32_t *)malloc(4 * n);
  CHECK(ldt_image_sizes(C.data, C.off, 1, 0, C.rows, nullptr, wh, st) == LDT_OK, "ldt_image_sizes");
  std::vector<int> W(n), H(n);
  for (size_t i = 0; i < n; ++i) {
    CHECK(st[i] == LDT_IMG_OK && wh[2 * i] >= 8 && wh[2 * i + 1] >= 8, "cell %zu: status %d", i, st[i]);
    W[i] = wh[2 * i];
    H[i] = wh[2 * i + 1];
    printf("size %d %d\n", W[i], H[i]);
  }
  free(wh);
  free(st);
  CHECK(W[0] == 500 && H[0] == 375, "cell 0 is %d x %d, the checks below take it for 500 x 375", W[0], H[0]);

  // size lists B and C of tests/test_gpu_view_sizes.py
  const Sizes SB = {7, 5, 299, 260, 1, 1, 8, 256, 9, 257};
  Sizes SC;
  for (int k = 0; k < 8; ++k) {
    const int32_t two[4] = {32, 40, 16, 24};
    SC.insert(SC.end(), two, two + 4);
  }
  const Sizes *lists[2] = {&SB, &SC};
  const char *names[2] = {"B", "C"};
  for (int li = 0; li < 2; ++li) {
    const Sizes &S = *lists[li];
    const int V = (int)(S.size() / 2);
    char what[64];
    for (int filter = 0; filter < 2; ++filter) {
      const int sup = filter ? 2 : 1;
      // ---- windows res = size + 32 + (3v, 2v): no row fails, every view in the table ----
      std::vector<ldt_crop> crops(n * V);
      std::vector<ldt_window> wins(n * V);
      for (size_t i = 0; i < n; ++i)
        for (int v = 0; v < V; ++v) {
          crops[i * V + v] = ldt_crop{(int)(i & 1), v & 1, H[i] - 1 - v % 3, W[i] - 2, (int)((i + v) & 1)};
          wins[i * V + v] = ldt_window{S[2 * v] + 32 + 3 * v, S[2 * v + 1] + 32 + 2 * v, 3 * v, 32 + 2 * v};
        }
      BatchPlan B;
      plan(C, crops, wins, S, filter, B);
      snprintf(what, sizeof(what), "%s filter %d windows", names[li], filter);
      CHECK(!B.geom_bad && B.n_views == V && B.views.size() == n * (size_t)V, "%s: %d views, %zu entries", what, B.n_views,
            B.views.size());
      check_geom(B.geom, (int64_t)n, S, what);
      int kh = 3, kv = 3;
      for (size_t i = 0; i < n; ++i) {
        CHECK(B.status[i] == LDT_IMG_OK, "%s row %zu: status %d", what, i, B.status[i]);
        for (int v = 0; v < V; ++v) {
          const ldt_crop &c = crops[i * V + v];
          const ldt_window &w = wins[i * V + v];
          const int32_t exp[12] = {c.top, c.left, c.height, c.width, c.flip, w.res_h, w.res_w, w.top, w.left,
                                   S[2 * v], S[2 * v + 1], 0};
          CHECK(memcmp(&B.views[(size_t)v * n + i], exp, sizeof(exp)) == 0, "%s row %zu view %d: table entry", what, i, v);
          kh = std::max(kh, ksize(c.width, w.res_w, sup));
          kv = std::max(kv, ksize(c.height, w.res_h, sup));
        }
      }
      CHECK(B.max_ks_h == kh && B.max_ks_v == kv, "%s: max_ks %d %d, every view's (box -> res) gives %d %d", what,
            B.max_ks_h, B.max_ks_v, kh, kv);

      // ---- no windows: the defaults (h_v, w_v, 0, 0), the reduction limit per view ----
      BatchPlan D;
      plan(C, {}, {}, S, filter, D);
      snprintf(what, sizeof(what), "%s filter %d defaults", names[li], filter);
      check_geom(D.geom, (int64_t)n, S, what);
      kh = kv = 3;
      for (size_t i = 0; i < n; ++i) {
        int want = LDT_IMG_OK;
        for (int v = 0; v < V && want == LDT_IMG_OK; ++v)
          if (ceil_div((int64_t)sup * W[i], S[2 * v + 1]) > 37 || ceil_div((int64_t)sup * H[i], S[2 * v]) > 37)
            want = LDT_IMG_TOO_LARGE;
        CHECK(D.status[i] == want, "%s row %zu: status %d, its views give %d", what, i, D.status[i], want);
        for (int v = 0; v < V; ++v) {
          const int32_t good[12] = {0, 0, H[i], W[i], 0, S[2 * v], S[2 * v + 1], 0, 0, S[2 * v], S[2 * v + 1], 0};
          const int32_t failed[12] = {0, 0, 1, 1, 0, S[2 * v], S[2 * v + 1], 0, 0, S[2 * v], S[2 * v + 1], 0};
          CHECK(memcmp(&D.views[(size_t)v * n + i], want == LDT_IMG_OK ? good : failed, sizeof(good)) == 0,
                "%s row %zu view %d: table entry (status %d)", what, i, v, want);
          if (want != LDT_IMG_OK) continue;
          kh = std::max(kh, ksize(W[i], S[2 * v + 1], sup));
          kv = std::max(kv, ksize(H[i], S[2 * v], sup));
        }
      }
      CHECK(D.max_ks_h == kh && D.max_ks_v == kv, "%s: max_ks %d %d, the good rows' views give %d %d", what, D.max_ks_h,
            D.max_ks_v, kh, kv);
      // the 500 x 375 cell passes every size of C with BILINEAR and fails B's 7 x 5 (and 1 x 1)
      if (filter == 0)
        CHECK(D.status[0] == (li == 0 ? LDT_IMG_TOO_LARGE : LDT_IMG_OK), "%s: the 500 x 375 cell has status %d", what,
              D.status[0]);
    }
    for (int64_t nn : {1, 5, 8, 9, 17}) {
      ViewGeomTab t;
      CHECK(view_geom_build(nn, V, S.data(), LDT_MAX_OUT, t), "list %s n %lld refused", names[li], (long long)nn);
      snprintf(what, sizeof(what), "%s n=%lld", names[li], (long long)nn);
      check_geom(t, nn, S, what);
      check_walk(t, nn, what);
    }
  }

  // ---- one box, two sizes: passes the reduction limit at one, fails at the other ----
  {
    const Sizes S = {10, 10, 5, 5, 10, 10}; // a 370 x 370 box: 37 at 10, 74 at 5
    const int V = 3;
    std::vector<ldt_crop> crops(n * V, ldt_crop{0, 0, 8, 8, 0});
    for (int v = 0; v < V; ++v) crops[v] = ldt_crop{0, 0, 370, 370, 0};
    BatchPlan B;
    plan(C, crops, {}, S, 0, B);
    CHECK(B.status[0] == LDT_IMG_TOO_LARGE, "370 box at (10, 5, 10): status %d", B.status[0]);
    for (size_t i = 1; i < n; ++i) CHECK(B.status[i] == LDT_IMG_OK, "its neighbour %zu: status %d", i, B.status[i]);
    const Sizes S2 = {10, 10, 10, 10, 10, 10};
    plan(C, crops, {}, S2, 0, B);
    CHECK(B.status[0] == LDT_IMG_OK, "370 box at 10 x 10 three times: status %d", B.status[0]);
    // and a window that fits the small size only
    std::vector<ldt_window> wins(n * V, ldt_window{12, 12, 1, 1});
    plan(C, crops, wins, S2, 0, B);
    for (size_t i = 0; i < n; ++i) CHECK(B.status[i] == LDT_IMG_OK, "12 x 12 window at 10 x 10 row %zu: %d", i, B.status[i]);
    const Sizes S3 = {10, 10, 12, 12, 10, 10};
    plan(C, crops, wins, S3, 0, B);
    for (size_t i = 0; i < n; ++i)
      CHECK(B.status[i] == LDT_IMG_BAD_WINDOW, "12 x 12 window at origin 1 for a 12 x 12 view, row %zu: %d", i, B.status[i]);
  }

  // ---- V = 1 with a size: the table exists, the descriptor carries the view ----
  {
    const Sizes S = {40, 40};
    BatchPlan B;
    plan(C, {}, {}, S, 0, B);
    CHECK(B.n_views == 1 && B.views.size() == n && B.geom.views == 1, "V = 1: %zu entries", B.views.size());
    for (size_t i = 0; i < n; ++i)
      CHECK(B.status[i] == LDT_IMG_OK && B.descs[i].res_h == 40 && B.descs[i].res_w == 40, "V = 1 row %zu", i);
    // and no sizes: as before
    BatchPlan P;
    plan(C, {}, {}, {}, 0, P);
    CHECK(P.geom.views == 0 && P.views.empty() && !P.geom_bad, "a plain plan has a geometry table");
  }

  // ---- hostile sizes and counts: refused, never overflowed ----
  {
    Sizes big;
    for (int v = 0; v < 16; ++v) {
      big.push_back(1024);
      big.push_back(1024);
    }
    ViewGeomTab t;
    // 16 views x 128 bands x 4 tiles = 8192 workgroups per image: 2^31 at n = 2^18
    CHECK(view_geom_build(262136, 16, big.data(), LDT_MAX_OUT, t) && t.total == (int64_t)262136 * 8192,
          "16 x 1024 x 1024 at n = 262136 refused");
    CHECK(!view_geom_build(262144, 16, big.data(), LDT_MAX_OUT, t) && t.views == 0, "n = 262144 accepted");
    CHECK(!view_geom_build(INT_MAX, 16, big.data(), LDT_MAX_OUT, t), "n = INT_MAX accepted");
    CHECK(!view_geom_build((int64_t)1 << 40, 16, big.data(), LDT_MAX_OUT, t), "n = 2^40 accepted");
    CHECK(!view_geom_build(-1, 16, big.data(), LDT_MAX_OUT, t), "n = -1 accepted");
    CHECK(!view_geom_build(5, 17, big.data(), LDT_MAX_OUT, t) && !view_geom_build(5, 0, big.data(), LDT_MAX_OUT, t) &&
              !view_geom_build(5, 1, nullptr, LDT_MAX_OUT, t),
          "a bad count or no sizes accepted");
    for (int32_t bad : {0, -1, 1025, INT_MAX, INT_MIN}) {
      Sizes s = {8, 8, 8, 8};
      s[3] = bad;
      CHECK(!view_geom_build(5, 2, s.data(), LDT_MAX_OUT, t), "width %d accepted", bad);
      s[3] = 8;
      s[0] = bad;
      CHECK(!view_geom_build(5, 2, s.data(), LDT_MAX_OUT, t), "height %d accepted", bad);
      // and through plan_batch: every row fails, no table of hostile size is formed
      s[0] = 8;
      s[2] = bad;
      BatchPlan B;
      plan(C, {}, {}, s, 0, B);
      CHECK(B.geom_bad && B.geom.views == 0 && B.any_bad, "plan_batch took height %d", bad);
      for (size_t i = 0; i < n; ++i) CHECK(B.status[i] != LDT_IMG_OK, "height %d row %zu planned", bad, i);
    }
  }

  free(C.off);
  free(C.data);
  if (!g_fail) printf("view_sizes_plan_ok\n");
  return g_fail;
}
