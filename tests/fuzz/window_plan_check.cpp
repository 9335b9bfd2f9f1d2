// Driver for the window handling of libldt's host planner (csrc/ldt_plan.cpp),
// built for the CPU with -fsanitize=address,undefined by tests/test_window.py
// and run directly. It calls the check_window / plan_batch that libldt.so
// calls, with windows (ldt_set_windows hands them to plan_batch unchanged),
// with and without crops.
//
// Input on stdin: records of [uint32 little-endian length][bytes], at least
// three decodable JPEG cells, the first at least 380 x 380 (37 * 10 + 1 fits
// both axes). The cells, their offsets and every crop and window array live
// in heap buffers of exactly their size, so a read past any of them is an ASan
// report. Every check that fails prints a line and makes the exit status 1;
// "window_plan_ok" is printed at the end of a clean run.
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

// Plans rows [arr_offset, rows) with `crops` and `wins` (one per planned row
// each, in exact-size heap buffers; empty = none).
void plan(const Cells &C, int64_t arr_offset, const std::vector<ldt_crop> &crops, const std::vector<ldt_window> &wins,
          int oh, int ow, BatchPlan &B) {
  const int64_t n = C.rows - arr_offset;
  ldt_crop *hc = heap_copy(crops);
  ldt_window *hw = heap_copy(wins);
  PlanOptions opt;
  opt.out_h = oh;
  opt.out_w = ow;
  HuffCache cache;
  plan_batch(C.data, C.off, arr_offset, n, nullptr, opt, cache, B, hc, hw);
  // the blob is written from the descriptors: lay it out and write it too
  const PlanLayout L = plan_layout(B, false);
  uint8_t *blob = (uint8_t *)malloc(L.plan_bytes ? (size_t)L.plan_bytes : 1);
  write_plan(B, L, nullptr, nullptr, blob);
  free(blob);
  free(hw);
  free(hc);
}

// resample_ksize restated: 2 * max(1, ceil(in / out)) + 1
int ksize(int in, int out) { return 2 * std::max(1, (in + out - 1) / out) + 1; }

// What the batch's tap maxima must be: the maximum of resample_ksize(source ->
// res) over the rows that did not fail; 3, 3 when every row failed.
void check_taps(const BatchPlan &B, const std::vector<ldt_crop> &src, const std::vector<ldt_window> &wins,
                const char *what) {
  int kh = 3, kv = 3, mw = 1, mh = 1;
  for (size_t i = 0; i < src.size(); ++i) {
    if (B.status[i] != LDT_IMG_OK) continue;
    kh = std::max(kh, ksize(src[i].width, wins[i].res_w));
    kv = std::max(kv, ksize(src[i].height, wins[i].res_h));
    mw = std::max(mw, src[i].width);
    mh = std::max(mh, src[i].height);
  }
  CHECK(B.max_ks_h == kh && B.max_ks_v == kv, "%s: max_ks_h %d max_ks_v %d, (source -> res) gives %d %d", what,
        B.max_ks_h, B.max_ks_v, kh, kv);
  CHECK(B.max_w == mw && B.max_h == mh, "%s: max_w %d max_h %d, the sources give %d %d", what, B.max_w, B.max_h, mw, mh);
}

void check_desc(const BatchPlan &B, size_t i, const ldt_crop &box, const ldt_window &w, const char *what) {
  const ImgDesc &d = B.descs[i];
  CHECK(d.res_h == w.res_h && d.res_w == w.res_w && d.win_top == w.top && d.win_left == w.left,
        "%s row %zu: window (%d, %d, %d, %d), expected (%d, %d, %d, %d)", what, i, d.res_h, d.res_w, d.win_top,
        d.win_left, w.res_h, w.res_w, w.top, w.left);
  CHECK(d.box_top == box.top && d.box_left == box.left && d.box_h == box.height && d.box_w == box.width &&
            d.flip == box.flip,
        "%s row %zu: box (%d, %d, %d, %d, %d), expected (%d, %d, %d, %d, %d)", what, i, d.box_top, d.box_left, d.box_h,
        d.box_w, d.flip, box.top, box.left, box.height, box.width, box.flip);
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
    CHECK(st[i] == LDT_IMG_OK && wh[2 * i] > 0 && wh[2 * i + 1] > 0, "cell %zu: status %d", i, st[i]);
    W[i] = wh[2 * i];
    H[i] = wh[2 * i + 1];
    printf("size %d %d\n", W[i], H[i]);
  }
  free(wh);
  free(st);
  CHECK(W[0] >= 371 && H[0] >= 371, "cell 0 is %dx%d", W[0], H[0]);

  // ---- check_window: every bad class, the last good value at each edge, hostile values ----
  {
    const int oh = 224, ow = 200;
    const ldt_window good[] = {
        {224, 200, 0, 0},     {225, 201, 1, 1},         {256, 341, 16, 70},           {LDT_MAX_RES, LDT_MAX_RES, 0, 0},
        {LDT_MAX_RES, LDT_MAX_RES, LDT_MAX_RES - 224, LDT_MAX_RES - 200}, {224, 2000, 0, 1800}, {2000, 200, 1776, 0},
    };
    for (const ldt_window &w : good)
      CHECK(check_window(w, oh, ow) == LDT_IMG_OK, "good window (%d, %d, %d, %d) refused", w.res_h, w.res_w, w.top, w.left);
    const ldt_window bad[] = {
        {0, 200, 0, 0},         {224, 0, 0, 0},          {-1, 200, 0, 0},          {224, -1, 0, 0},          // res < 1
        {LDT_MAX_RES + 1, 200, 0, 0}, {224, LDT_MAX_RES + 1, 0, 0}, {INT_MAX, INT_MAX, 0, 0}, {INT_MIN, INT_MIN, 0, 0}, // res > max
        {224, 200, -1, 0},      {224, 200, 0, -1},       {300, 300, INT_MIN, 0},   {300, 300, 0, INT_MIN},   // negative origin
        {223, 200, 0, 0},       {224, 199, 0, 0},        {224, 200, 1, 0},         {224, 200, 0, 1},         // not inside
        {300, 300, 77, 0},      {300, 300, 0, 101},      {300, 300, INT_MAX, 0},   {300, 300, 0, INT_MAX},
        {300, 300, INT_MAX, INT_MAX}, {INT_MAX, 300, INT_MAX, 0}, {INT_MIN, INT_MAX, INT_MIN, INT_MAX}, {1, 1, 0, 0},
        {300, 300, 300, 0},     {300, 300, 0, 300},      {300, 300, 301, 0},       {LDT_MAX_RES, LDT_MAX_RES, LDT_MAX_RES - 223, 0},
    };
    for (const ldt_window &w : bad)
      CHECK(check_window(w, oh, ow) == LDT_IMG_BAD_WINDOW, "bad window (%d, %d, %d, %d) accepted", w.res_h, w.res_w, w.top,
            w.left);
    CHECK(check_window(ldt_window{300, 300, 76, 100}, oh, ow) == LDT_IMG_OK, "flush bottom-right window refused");
    CHECK(check_window(ldt_window{1, 1, 0, 0}, 1, 1) == LDT_IMG_OK, "1x1 of 1x1 refused");
    CHECK(check_window(ldt_window{LDT_MAX_RES, 1, LDT_MAX_RES - 1, 0}, 1, 1) == LDT_IMG_OK, "last row refused");
    CHECK(check_window(ldt_window{LDT_MAX_RES, 1, LDT_MAX_RES, 0}, 1, 1) == LDT_IMG_BAD_WINDOW, "row past the end accepted");
  }

  BatchPlan B;
  std::vector<ldt_crop> whole(n);
  for (size_t i = 0; i < n; ++i) whole[i] = ldt_crop{0, 0, H[i], W[i], 0};

  // ---- no windows: the descriptors carry out_h, out_w, 0, 0 ----
  {
    std::vector<ldt_window> none(n, ldt_window{30, 33, 0, 0});
    plan(C, 0, {}, {}, 30, 33, B);
    for (size_t i = 0; i < n; ++i) {
      CHECK(B.status[i] == LDT_IMG_OK, "unwindowed row %zu: status %d", i, B.status[i]);
      check_desc(B, i, whole[i], none[i], "unwindowed");
    }
    check_taps(B, whole, none, "unwindowed");
    BatchPlan Bw;
    plan(C, 0, {}, none, 30, 33, Bw); // the same through explicit res == out windows
    CHECK(Bw.max_w == B.max_w && Bw.max_h == B.max_h && Bw.max_ks_h == B.max_ks_h && Bw.max_ks_v == B.max_ks_v,
          "res == out windows change the maxima");
    for (size_t i = 0; i < n; ++i) check_desc(Bw, i, whole[i], none[i], "res == out");
  }

  // ---- valid windows without crops: fields, taps of (image -> res) ----
  const int oh = 30, ow = 33;
  std::vector<ldt_window> ok(n);
  for (size_t i = 0; i < n; ++i) {
    // the shorter edge to 64, as Resize(64) does; the window flush bottom-right
    const int rw = W[i] <= H[i] ? 64 : 64 * W[i] / H[i], rh = W[i] <= H[i] ? 64 * H[i] / W[i] : 64;
    ok[i] = ldt_window{rh, rw, rh - oh, rw - ow};
  }
  plan(C, 0, {}, ok, oh, ow, B);
  for (size_t i = 0; i < n; ++i) {
    CHECK(B.status[i] == LDT_IMG_OK, "valid window row %zu: status %d", i, B.status[i]);
    check_desc(B, i, whole[i], ok[i], "valid window");
    CHECK(B.descs[i].width == W[i] && B.descs[i].height == H[i], "valid window row %zu: image size changed", i);
  }
  check_taps(B, whole, ok, "valid windows");
  {
    // res far above out: an upscale, three taps whatever the output size
    std::vector<ldt_window> up(n, ldt_window{9000, 20000, 9000 - oh, 20000 - ow});
    plan(C, 0, {}, up, oh, ow, B);
    for (size_t i = 0; i < n; ++i) CHECK(B.status[i] == LDT_IMG_OK, "upscale row %zu: status %d", i, B.status[i]);
    CHECK(B.max_ks_h == 3 && B.max_ks_v == 3, "upscale taps %d %d", B.max_ks_h, B.max_ks_v);
    check_taps(B, whole, up, "upscale");
  }

  // ---- with crops: the source is the box ----
  std::vector<ldt_crop> boxes(n);
  for (size_t i = 0; i < n; ++i) {
    const int bw = std::max(1, W[i] / 2), bh = std::max(1, H[i] / 3);
    boxes[i] = ldt_crop{H[i] - bh, W[i] - bw, bh, bw, (int)(i & 1)};
  }
  plan(C, 0, boxes, ok, oh, ow, B);
  for (size_t i = 0; i < n; ++i) {
    CHECK(B.status[i] == LDT_IMG_OK, "box + window row %zu: status %d", i, B.status[i]);
    check_desc(B, i, boxes[i], ok[i], "box + window");
  }
  check_taps(B, boxes, ok, "boxes + windows");

  // ---- bad windows, each on row 1 between good rows, with and without crops ----
  const ldt_window hostile[] = {
      {0, 64, 0, 0},          {64, 0, 0, 0},         {LDT_MAX_RES + 1, 64, 0, 0}, {64, LDT_MAX_RES + 1, 0, 0},
      {64, 64, -1, 0},        {64, 64, 0, -1},       {64, 64, 35, 0},             {64, 64, 0, 32},
      {29, 64, 0, 0},         {64, 32, 0, 0},        {INT_MAX, INT_MAX, INT_MAX, INT_MAX},
      {INT_MIN, INT_MIN, INT_MIN, INT_MIN},          {64, 64, INT_MAX, INT_MIN},  {INT_MAX, 64, 0, 0},
  };
  for (int with_crops = 0; with_crops < 2; ++with_crops)
    for (const ldt_window &bad : hostile) {
      std::vector<ldt_window> wn = ok;
      wn[1] = bad;
      const std::vector<ldt_crop> &src = with_crops ? boxes : whole;
      plan(C, 0, with_crops ? boxes : std::vector<ldt_crop>(), wn, oh, ow, B);
      CHECK(B.status[1] == LDT_IMG_BAD_WINDOW, "window (%d, %d, %d, %d) crops %d: status %d", bad.res_h, bad.res_w,
            bad.top, bad.left, with_crops, B.status[1]);
      CHECK(B.any_bad, "any_bad not set");
      const ImgDesc &d = B.descs[1];
      CHECK(d.width == 1 && d.height == 1 && d.box_h == 1 && d.box_w == 1 && d.nseg == 0 && d.res_h == oh &&
                d.res_w == ow && d.win_top == 0 && d.win_left == 0,
            "failed row's descriptor is not the 1x1 one");
      for (size_t i = 0; i < n; ++i)
        if (i != 1) {
          CHECK(B.status[i] == LDT_IMG_OK, "neighbour %zu of a bad window: status %d", i, B.status[i]);
          check_desc(B, i, src[i], ok[i], "neighbour");
        }
      check_taps(B, src, wn, "hostile window");
    }
  {
    // a bad box under a good window keeps its own status
    std::vector<ldt_crop> cr = boxes;
    cr[1] = ldt_crop{0, 0, H[1] + 1, W[1], 0};
    plan(C, 0, cr, ok, oh, ow, B);
    CHECK(B.status[1] == LDT_IMG_BAD_CROP, "bad box under a good window: status %d", B.status[1]);
    CHECK(B.status[0] == LDT_IMG_OK && B.status[2] == LDT_IMG_OK, "its neighbours failed");
  }

  // ---- the reduction limit is against res: 37 accepted, 38 refused ----
  {
    // cell 0 whole: res 10 x 10 needs ceil(W / 10), ceil(H / 10) <= 37, i.e. W, H <= 370
    std::vector<ldt_window> wn(n, ldt_window{oh, ow, 0, 0});
    std::vector<ldt_crop> cr = whole;
    cr[0] = ldt_crop{1, 1, 370, 370, 1};
    wn[0] = ldt_window{10, 10, 3, 2};
    plan(C, 0, cr, wn, 7, 5, B); // a 7 x 5 window of the 10 x 10 result
    // rows 1.. have res == (30, 33) but the output is (7, 5): still windows inside res
    CHECK(B.status[0] == LDT_IMG_OK, "370 -> 10 (reduction 37): status %d", B.status[0]);
    check_desc(B, 0, cr[0], wn[0], "reduction 37");
    CHECK(B.max_ks_h == 75 && B.max_ks_v == 75, "taps at the limit %d %d", B.max_ks_h, B.max_ks_v);
    check_taps(B, cr, wn, "reduction 37");
    cr[0] = ldt_crop{0, 0, 370, 371, 0};
    plan(C, 0, cr, wn, 7, 5, B);
    CHECK(B.status[0] == LDT_IMG_TOO_LARGE, "371 -> 10 wide (reduction 38): status %d", B.status[0]);
    for (size_t i = 1; i < n; ++i) CHECK(B.status[i] == LDT_IMG_OK, "neighbour %zu: status %d", i, B.status[i]);
    check_taps(B, cr, wn, "reduction 38 wide");
    cr[0] = ldt_crop{0, 0, 371, 370, 0};
    plan(C, 0, cr, wn, 7, 5, B);
    CHECK(B.status[0] == LDT_IMG_TOO_LARGE, "371 -> 10 tall (reduction 38): status %d", B.status[0]);
    // without crops the source is the whole image
    wn[0] = ldt_window{(H[0] + 36) / 37, (W[0] + 36) / 37, 0, 0};
    plan(C, 0, {}, wn, 7, 5, B);
    CHECK(B.status[0] == LDT_IMG_OK, "whole image at reduction 37: status %d", B.status[0]);
    check_taps(B, whole, wn, "whole image at 37");
    if (wn[0].res_w > 7) { // one resized column fewer: ceil(W / res_w) = 38 when W > 37 * (res_w - 1)
      wn[0].res_w -= 1;
      plan(C, 0, {}, wn, 7, 5, B);
      CHECK(B.status[0] == ((W[0] + wn[0].res_w - 1) / wn[0].res_w > 37 ? LDT_IMG_TOO_LARGE : LDT_IMG_OK),
            "whole image one column past the limit: status %d", B.status[0]);
    }
    // the output size no longer bounds the reduction: out 7 x 5 of a res that is large enough
    wn[0] = ldt_window{H[0], W[0], H[0] - 7, W[0] - 5};
    plan(C, 0, {}, wn, 7, 5, B);
    CHECK(B.status[0] == LDT_IMG_OK, "identity res with a 7 x 5 window: status %d", B.status[0]);
    plan(C, 0, {}, {}, 7, 5, B);
    CHECK(B.status[0] == LDT_IMG_TOO_LARGE, "cell 0 unwindowed at 7 x 5: status %d", B.status[0]);
  }

  // ---- a batch that is a slice of the array: windows are indexed by batch row ----
  {
    std::vector<ldt_window> wn(ok.begin() + 1, ok.end());
    std::vector<ldt_crop> cr(boxes.begin() + 1, boxes.end());
    plan(C, 1, cr, wn, oh, ow, B);
    CHECK(B.descs.size() == n - 1, "slice: %zu rows", B.descs.size());
    for (size_t i = 0; i + 1 < n; ++i) {
      CHECK(B.status[i] == LDT_IMG_OK, "slice row %zu: status %d", i, B.status[i]);
      check_desc(B, i, boxes[i + 1], ok[i + 1], "slice");
    }
    check_taps(B, cr, wn, "slice");
  }

  free(C.off);
  free(C.data);
  if (!g_fail) printf("window_plan_ok\n");
  return g_fail;
}
