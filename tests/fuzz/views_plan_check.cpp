// Driver for the views handling of libldt's host planner (csrc/ldt_plan.cpp),
// built for the CPU with -fsanitize=address,undefined by tests/test_views.py
// and run directly. It calls the plan_batch that libldt.so calls, with
// views = V (ldt_set_views hands it to plan_batch unchanged) and n * V crops
// and windows, image-major.
//
// Input on stdin: records of [uint32 little-endian length][bytes], at least
// three decodable JPEG cells, each at least 8 x 8. The cells, their offsets and
// every crop and window array live in heap buffers of exactly their size, so a
// read past any of them is an ASan report. Every check that fails prints a
// line and makes the exit status 1; "views_plan_ok" is printed at the end of a
// clean run.
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/ldt.h"
#include "../../lance-distributed-training_amd/csrc/ldt_plan.hpp"

using namespace ldt;

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                   \
  do {                                     \
    if (!(cond)) {                         \
      printf("FAIL %s:%d: ", #cond, __LINE__); \
      printf(__VA_ARGS__);                 \
      printf("\n");                        \
      g_fail = 1;                          \
    }                                      \
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

int kOh = 30, kOw = 33; // the output size of the plans that follow

// the view table is a section of its own: the descriptor keeps its size
static_assert(sizeof(ImgDesc) == 320, "ImgDesc changed its size");

// Plans all rows with `views` views: crops and wins hold rows * views entries
// (image-major, exact-size heap buffers; empty = none). The blob is laid out
// and written too, and the view table read back from it.
void plan(const Cells &C, const std::vector<ldt_crop> &crops, const std::vector<ldt_window> &wins, int views,
          BatchPlan &B, PlanLayout &L, std::vector<ViewDesc> &table) {
  ldt_crop *hc = heap_copy(crops);
  ldt_window *hw = heap_copy(wins);
  PlanOptions opt;
  opt.out_h = kOh;
  opt.out_w = kOw;
  HuffCache cache;
  plan_batch(C.data, C.off, 0, C.rows, nullptr, opt, cache, B, hc, hw, views);
  L = plan_layout(B, false);
  uint8_t *blob = (uint8_t *)malloc(L.plan_bytes ? (size_t)L.plan_bytes : 1);
  write_plan(B, L, nullptr, nullptr, blob);
  table.assign(B.views.size(), ViewDesc());
  CHECK(L.off_view + (int64_t)(sizeof(ViewDesc) * B.views.size()) <= L.plan_bytes, "the view table leaves the blob");
  if (!B.views.empty()) memcpy(table.data(), blob + L.off_view, sizeof(ViewDesc) * B.views.size());
  free(blob);
  free(hw);
  free(hc);
}

// resample_ksize restated: 2 * max(1, ceil(in / out)) + 1
int ksize(int in, int out) { return 2 * std::max(1, (in + out - 1) / out) + 1; }

// The status one view of a W x H image must get, in the order window, crop,
// too large; restated here, not taken from check_window / check_crop.
int view_status(const ldt_crop &c, const ldt_window &w, int W, int H) {
  const int64_t rh = w.res_h, rw = w.res_w, t = w.top, l = w.left;
  if (rh < 1 || rh > LDT_MAX_RES || rw < 1 || rw > LDT_MAX_RES || t < 0 || l < 0 || t + kOh > rh || l + kOw > rw)
    return LDT_IMG_BAD_WINDOW;
  const int64_t ct = c.top, cl = c.left, ch = c.height, cw = c.width;
  if (ct < 0 || cl < 0 || ch < 1 || cw < 1 || ct + ch > H || cl + cw > W || (c.flip != 0 && c.flip != 1))
    return LDT_IMG_BAD_CROP;
  if ((cw + rw - 1) / rw > 37 || (ch + rh - 1) / rh > 37) return LDT_IMG_TOO_LARGE;
  return LDT_IMG_OK;
}

// Everything a plan with views must satisfy, from what it was given.
void check_plan(const Cells &C, const std::vector<int> &W, const std::vector<int> &H, const std::vector<ldt_crop> &crops,
                const std::vector<ldt_window> &wins, int V, const char *what) {
  const size_t n = (size_t)C.rows;
  BatchPlan B;
  PlanLayout L;
  std::vector<ViewDesc> tab;
  plan(C, crops, wins, V, B, L, tab);
  CHECK(B.n_views == V, "%s: n_views %d", what, B.n_views);
  CHECK(B.views.size() == (V > 1 ? n * (size_t)V : 0), "%s: %zu view entries for %zu rows of %d views", what,
        B.views.size(), n, V);
  int kh = 3, kv = 3, mw = 1, mh = 1;
  bool any_bad = false;
  for (size_t i = 0; i < n; ++i) {
    // the first view that fails gives the row its status
    int want = LDT_IMG_OK;
    for (int v = 0; v < V && want == LDT_IMG_OK; ++v) {
      const ldt_crop c = crops.empty() ? ldt_crop{0, 0, H[i], W[i], 0} : crops[i * V + v];
      const ldt_window w = wins.empty() ? ldt_window{kOh, kOw, 0, 0} : wins[i * V + v];
      want = view_status(c, w, W[i], H[i]);
    }
    CHECK(B.status[i] == want, "%s row %zu: status %d, the first bad view gives %d", what, i, B.status[i], want);
    any_bad = any_bad || want != LDT_IMG_OK;
    const ImgDesc &d = B.descs[i];
    if (want != LDT_IMG_OK)
      CHECK(d.width == 1 && d.height == 1 && d.box_h == 1 && d.box_w == 1 && d.nseg == 0 && d.res_h == kOh &&
                d.res_w == kOw,
            "%s row %zu: a failed row's descriptor is not the 1x1 one", what, i);
    else
      CHECK(d.width == W[i] && d.height == H[i], "%s row %zu: image size %dx%d", what, i, d.width, d.height);
    for (int v = 0; v < V; ++v) {
      const ldt_crop c = crops.empty() ? ldt_crop{0, 0, H[i], W[i], 0} : crops[i * V + v];
      const ldt_window w = wins.empty() ? ldt_window{kOh, kOw, 0, 0} : wins[i * V + v];
      // word for word: the table entry of output image v * n + i
      const int32_t good[12] = {c.top, c.left, c.height, c.width, c.flip, w.res_h, w.res_w, w.top, w.left, 0, 0, 0};
      const int32_t failed[12] = {0, 0, 1, 1, 0, kOh, kOw, 0, 0, 0, 0, 0};
      const int32_t *exp = want == LDT_IMG_OK ? good : failed;
      if (V > 1) {
        int32_t got[12];
        static_assert(sizeof(ViewDesc) == sizeof(got), "ViewDesc is twelve words");
        memcpy(got, &tab[(size_t)v * n + i], sizeof(got));
        CHECK(memcmp(got, exp, sizeof(got)) == 0,
              "%s row %zu view %d: table (%d %d %d %d %d | %d %d %d %d), expected (%d %d %d %d %d | %d %d %d %d)", what, i,
              v, got[0], got[1], got[2], got[3], got[4], got[5], got[6], got[7], got[8], exp[0], exp[1], exp[2], exp[3],
              exp[4], exp[5], exp[6], exp[7], exp[8]);
      }
      if (v == 0 && want == LDT_IMG_OK)
        CHECK(d.box_top == c.top && d.box_left == c.left && d.box_h == c.height && d.box_w == c.width &&
                  d.flip == c.flip && d.res_h == w.res_h && d.res_w == w.res_w && d.win_top == w.top &&
                  d.win_left == w.left,
              "%s row %zu: the descriptor does not carry view 0", what, i);
      if (want != LDT_IMG_OK) continue;
      kh = std::max(kh, ksize(c.width, w.res_w));
      kv = std::max(kv, ksize(c.height, w.res_h));
      mw = std::max(mw, c.width);
      mh = std::max(mh, c.height);
    }
  }
  CHECK(B.any_bad == any_bad, "%s: any_bad %d", what, (int)B.any_bad);
  CHECK(B.max_ks_h == kh && B.max_ks_v == kv, "%s: max_ks_h %d max_ks_v %d, the widest good view gives %d %d", what,
        B.max_ks_h, B.max_ks_v, kh, kv);
  CHECK(B.max_w == mw && B.max_h == mh, "%s: max_w %d max_h %d, the good views give %d %d", what, B.max_w, B.max_h, mw,
        mh);
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
  if (C.rows < 3) return 2;
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

  const int Vs[] = {1, 3, 16};
  for (int V : Vs) {
    // in-range views: every view its own box (growing with v), window and flip
    std::vector<ldt_crop> crops(n * V);
    std::vector<ldt_window> wins(n * V);
    for (size_t i = 0; i < n; ++i)
      for (int v = 0; v < V; ++v) {
        const int bw = std::max(1, W[i] * (v + 1) / (V + 1)), bh = std::max(1, H[i] * (V - v) / (V + 1));
        crops[i * V + v] = ldt_crop{(H[i] - bh) / 2, W[i] - bw, bh, bw, (int)((i + v) & 1)};
        wins[i * V + v] = ldt_window{kOh + 7 * v, kOw + 3 * v + (int)i, 7 * v, (3 * v + (int)i) / 2};
      }
    char what[64];
    snprintf(what, sizeof(what), "V=%d in range", V);
    check_plan(C, W, H, crops, wins, V, what);
    snprintf(what, sizeof(what), "V=%d crops only", V);
    check_plan(C, W, H, crops, {}, V, what);
    snprintf(what, sizeof(what), "V=%d windows only", V);
    check_plan(C, W, H, {}, wins, V, what);
    snprintf(what, sizeof(what), "V=%d neither", V);
    check_plan(C, W, H, {}, {}, V, what);

    // out-of-range views: every view of every row bad, hostile values included
    {
      std::vector<ldt_crop> bc = crops;
      std::vector<ldt_window> bw = wins;
      for (size_t k = 0; k < bc.size(); ++k) {
        if (k % 3 == 0) bc[k] = ldt_crop{INT_MAX, INT_MIN, INT_MAX, INT_MAX, 7};
        else if (k % 3 == 1) bw[k] = ldt_window{INT_MAX, INT_MIN, INT_MAX, INT_MIN};
        else bc[k].height = H[k / V] + 1;
      }
      snprintf(what, sizeof(what), "V=%d out of range", V);
      check_plan(C, W, H, bc, bw, V, what);
    }

    // mixed: one bad view per row at a different place each, the last row good;
    // row 0 has a bad crop in view 0 and a bad window in its last view: the
    // crop's status, because view 0 is checked first
    {
      std::vector<ldt_crop> mc = crops;
      std::vector<ldt_window> mw = wins;
      for (size_t i = 0; i + 1 < n; ++i) {
        const int v = (int)(i % (size_t)V);
        if (i == 0) {
          mc[0].flip = 2;
          mw[(size_t)V - 1] = ldt_window{kOh - 1, kOw, 0, 0};
        } else if (i & 1) {
          mw[i * V + v] = ldt_window{kOh, kOw, 1, 0}; // one row past res
        } else {
          mc[i * V + v] = ldt_crop{0, 0, 1, W[i], 0};
          mw[i * V + v] = ldt_window{kOh, 1 + (W[i] - 1) / 38, 0, 0}; // the box reduced by 38 or more, or res too narrow
        }
      }
      snprintf(what, sizeof(what), "V=%d mixed", V);
      check_plan(C, W, H, mc, mw, V, what);
      BatchPlan B;
      PlanLayout L;
      std::vector<ViewDesc> tab;
      plan(C, mc, mw, V, B, L, tab);
      CHECK(B.status[0] == (V == 1 ? LDT_IMG_BAD_WINDOW : LDT_IMG_BAD_CROP), "V=%d row 0: status %d", V, B.status[0]);
      CHECK(B.status[n - 1] == LDT_IMG_OK, "V=%d: the good row failed (%d)", V, B.status[n - 1]);
    }
  }

  // ---- the reduction limit inside a row's views, at 7 x 5: row 0's view 1 of 3 is one column over ----
  {
    kOh = 7;
    kOw = 5;
    const int V = 3;
    std::vector<ldt_crop> crops(n * V);
    std::vector<ldt_window> wins(n * V);
    for (size_t i = 0; i < n; ++i)
      for (int v = 0; v < V; ++v) {
        wins[i * V + v] = ldt_window{7 + v, 5 + v, v, 0};
        crops[i * V + v] = ldt_crop{0, 0, std::min(H[i], 37 * (7 + v)), std::min(W[i], 37 * (5 + v)), v & 1};
      }
    check_plan(C, W, H, crops, wins, V, "7x5 at the limit");
    {
      BatchPlan B;
      PlanLayout L;
      std::vector<ViewDesc> tab;
      plan(C, crops, wins, V, B, L, tab);
      for (size_t i = 0; i < n; ++i) CHECK(B.status[i] == LDT_IMG_OK, "7x5 at the limit row %zu: status %d", i, B.status[i]);
    }
    CHECK(W[0] > 37 * 6, "cell 0 is %d wide", W[0]);
    crops[1].width = 37 * 6 + 1;
    check_plan(C, W, H, crops, wins, V, "7x5 view 1 over the limit");
    BatchPlan B;
    PlanLayout L;
    std::vector<ViewDesc> tab;
    plan(C, crops, wins, V, B, L, tab);
    CHECK(B.status[0] == LDT_IMG_TOO_LARGE, "7x5 view 1 over the limit: status %d", B.status[0]);
    for (size_t i = 1; i < n; ++i) CHECK(B.status[i] == LDT_IMG_OK, "its neighbour %zu: status %d", i, B.status[i]);
    kOh = 30;
    kOw = 33;
  }

  // ---- views = 1 is the call without the argument ----
  {
    std::vector<ldt_crop> crops(n);
    std::vector<ldt_window> wins(n);
    for (size_t i = 0; i < n; ++i) {
      crops[i] = ldt_crop{1, 2, H[i] - 2, W[i] - 3, (int)(i & 1)};
      wins[i] = ldt_window{kOh + 5, kOw + 9, 5, 4};
    }
    ldt_crop *hc = heap_copy(crops);
    ldt_window *hw = heap_copy(wins);
    PlanOptions opt;
    opt.out_h = kOh;
    opt.out_w = kOw;
    HuffCache c0, c1;
    BatchPlan B0, B1;
    plan_batch(C.data, C.off, 0, C.rows, nullptr, opt, c0, B0, hc, hw);
    plan_batch(C.data, C.off, 0, C.rows, nullptr, opt, c1, B1, hc, hw, 1);
    free(hw);
    free(hc);
    CHECK(B1.views.empty() && B0.views.empty() && B0.n_views == 1 && B1.n_views == 1, "views = 1 made a view table");
    CHECK(B0.descs.size() == B1.descs.size() &&
              memcmp(B0.descs.data(), B1.descs.data(), sizeof(ImgDesc) * B0.descs.size()) == 0,
          "views = 1: the descriptors differ");
    CHECK(B0.status == B1.status && B0.max_w == B1.max_w && B0.max_h == B1.max_h && B0.max_ks_h == B1.max_ks_h &&
              B0.max_ks_v == B1.max_ks_v,
          "views = 1: status or maxima differ");
    const PlanLayout L0 = plan_layout(B0, true), L1 = plan_layout(B1, true);
    CHECK(memcmp(&L0, &L1, sizeof(PlanLayout)) == 0, "views = 1: the layout differs");
    CHECK(L0.off_view == L0.plan_bytes, "an empty view table takes room");
    CHECK(L0.off_desc < L0.off_seg && L0.off_seg <= L0.off_huff && L0.off_huff <= L0.off_quant &&
              L0.off_quant <= L0.off_lut && L0.off_lut < L0.off_labels && L0.off_labels < L0.off_status &&
              L0.off_status < L0.off_par && L0.off_par <= L0.off_chunk && L0.off_chunk <= L0.off_redo &&
              L0.off_redo < L0.off_pscan && L0.off_pscan <= L0.off_ptab && L0.off_ptab <= L0.off_pimg &&
              L0.off_pimg <= L0.off_view,
          "the sections changed their order");
    // and with views the earlier sections stay where they are: the table is appended
    BatchPlan B3;
    HuffCache c3;
    std::vector<ldt_crop> c3v(n * 3);
    for (size_t k = 0; k < c3v.size(); ++k) c3v[k] = crops[k / 3];
    ldt_crop *h3 = heap_copy(c3v);
    plan_batch(C.data, C.off, 0, C.rows, nullptr, opt, c3, B3, h3, nullptr, 3);
    free(h3);
    const PlanLayout L3 = plan_layout(B3, true);
    CHECK(L3.off_view >= L3.off_pimg && L3.plan_bytes >= L3.off_view + (int64_t)(sizeof(ViewDesc) * n * 3),
          "the view table is not the last section");
  }

  free(C.off);
  free(C.data);
  if (!g_fail) printf("views_plan_ok\n");
  return g_fail;
}
