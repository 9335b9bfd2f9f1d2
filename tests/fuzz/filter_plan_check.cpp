// Driver for the filter handling of libldt's host planner (csrc/ldt_plan.cpp),
// built for the CPU with -fsanitize=address,undefined by
// tests/test_interpolation.py and run directly. It calls the check_crop /
// plan_batch that libldt.so calls, with PlanOptions::filter set as
// ldt_set_filter sets it, with and without crops and windows.
//
// Input on stdin: records of [uint32 little-endian length][bytes], at least
// three decodable JPEG cells, the first at least 160 x 160 (a box of 149 fits
// both axes), another at least 16 x 16. The cells, their offsets and every
// crop and window array live in heap buffers of exactly their size, so a read
// past any of them is an ASan report. Every check that fails prints a line and
// makes the exit status 1; "filter_plan_ok" is printed at the end of a clean
// run.
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

void plan(const Cells &C, const std::vector<ldt_crop> &crops, const std::vector<ldt_window> &wins, int oh, int ow,
          int filter, BatchPlan &B) {
  ldt_crop *hc = heap_copy(crops);
  ldt_window *hw = heap_copy(wins);
  PlanOptions opt;
  opt.out_h = oh;
  opt.out_w = ow;
  opt.filter = filter;
  HuffCache cache;
  plan_batch(C.data, C.off, 0, C.rows, nullptr, opt, cache, B, hc, hw);
  const PlanLayout L = plan_layout(B, false);
  uint8_t *blob = (uint8_t *)malloc(L.plan_bytes ? (size_t)L.plan_bytes : 1);
  write_plan(B, L, nullptr, nullptr, blob);
  free(blob);
  free(hw);
  free(hc);
}

// the taps restated: bilinear 2 * max(ceil(in / out), 1) + 1, bicubic 2 * max(ceil(2 * in / out), 2) + 1
int ksize(int in, int out, int filter) {
  return filter ? 2 * std::max(2, (2 * in + out - 1) / out) + 1 : 2 * std::max(1, (in + out - 1) / out) + 1;
}
int reduce(int in, int out, int filter) { return ((filter ? 2 : 1) * in + out - 1) / out; }

// Every row's status by the rule (the cells decode and the boxes and windows
// are good, so only the reduction decides) and the batch's tap maxima.
void check_plan(const BatchPlan &B, const std::vector<ldt_crop> &src, const std::vector<ldt_window> &wins, int filter,
                const char *what) {
  int kh = 3, kv = 3;
  for (size_t i = 0; i < src.size(); ++i) {
    const bool big = reduce(src[i].width, wins[i].res_w, filter) > 37 || reduce(src[i].height, wins[i].res_h, filter) > 37;
    CHECK(B.status[i] == (big ? LDT_IMG_TOO_LARGE : LDT_IMG_OK), "%s filter %d row %zu (%dx%d -> %dx%d): status %d", what,
          filter, i, src[i].height, src[i].width, wins[i].res_h, wins[i].res_w, B.status[i]);
    if (B.status[i] != LDT_IMG_OK) continue;
    kh = std::max(kh, ksize(src[i].width, wins[i].res_w, filter));
    kv = std::max(kv, ksize(src[i].height, wins[i].res_h, filter));
  }
  CHECK(B.max_ks_h == kh && B.max_ks_v == kv, "%s filter %d: max_ks_h %d max_ks_v %d, expected %d %d", what, filter,
        B.max_ks_h, B.max_ks_v, kh, kv);
  CHECK(B.max_ks_h <= 75 && B.max_ks_v <= 75, "%s filter %d: more than 75 taps", what, filter);
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
  CHECK(W[0] >= 160 && H[0] >= 160, "cell 0 is %dx%d", W[0], H[0]);

  // ---- the tap capacity and the limit, as functions ----
  for (int in = 1; in <= 8192; in += (in < 400 ? 1 : 37))
    for (int out : {1, 2, 5, 7, 8, 33, 224, 256, 1024, 65535})
      for (int f = 0; f < 2; ++f) {
        CHECK(resample_ksize_host(in, out, f) == ksize(in, out, f), "ksize %d -> %d filter %d", in, out, f);
        CHECK(resample_reduce(in, out, f) == reduce(in, out, f), "reduce %d -> %d filter %d", in, out, f);
        if (in <= out) CHECK(resample_ksize_host(in, out, f) == (f ? 5 : 3), "upscale taps %d -> %d filter %d", in, out, f);
      }
  CHECK(resample_ksize_host(512, 224, kFilterBicubic) == 11, "512 -> 224 bicubic taps");
  CHECK(resample_ksize_host(4144, 224, kFilterBicubic) == 75 && resample_reduce(4145, 224, kFilterBicubic) == 38,
        "the 4144 px limit at 224");

  // ---- check_crop: the boundary, both axes, both filters; the default argument is bilinear ----
  {
    const ldt_crop b148{0, 0, 148, 148, 0}, b149w{0, 0, 148, 149, 0}, b149h{0, 0, 149, 148, 0}, b296{0, 0, 296, 296, 0},
        b297{0, 0, 296, 297, 0};
    CHECK(check_crop(b148, 400, 400, 8, 8, kFilterBicubic) == LDT_IMG_OK, "148 -> 8 bicubic refused");
    CHECK(check_crop(b149w, 400, 400, 8, 8, kFilterBicubic) == LDT_IMG_TOO_LARGE, "149 wide -> 8 bicubic accepted");
    CHECK(check_crop(b149h, 400, 400, 8, 8, kFilterBicubic) == LDT_IMG_TOO_LARGE, "149 tall -> 8 bicubic accepted");
    CHECK(check_crop(b149w, 400, 400, 8, 8, kFilterBilinear) == LDT_IMG_OK && check_crop(b149w, 400, 400, 8, 8) == LDT_IMG_OK,
          "149 -> 8 bilinear refused");
    CHECK(check_crop(b296, 400, 400, 8, 8) == LDT_IMG_OK && check_crop(b297, 400, 400, 8, 8) == LDT_IMG_TOO_LARGE,
          "the bilinear limit moved");
    // a bad box stays a bad box under either filter: crop 6 before too large 4
    CHECK(check_crop(ldt_crop{0, 0, 401, 149, 0}, 400, 400, 8, 8, kFilterBicubic) == LDT_IMG_BAD_CROP, "bad box order");
    CHECK(check_crop(ldt_crop{0, 0, 8192, 8192, 0}, 8192, 8192, 224, 224, kFilterBicubic) == LDT_IMG_TOO_LARGE, "8192 bicubic");
    CHECK(check_crop(ldt_crop{0, 0, 4144, 4144, 0}, 8192, 8192, 224, 224, kFilterBicubic) == LDT_IMG_OK, "4144 bicubic");
    CHECK(check_crop(ldt_crop{0, 0, 8192, 8192, 0}, 8192, 8192, 224, 224) == LDT_IMG_OK, "8192 bilinear");
  }

  BatchPlan B;
  std::vector<ldt_crop> whole(n);
  for (size_t i = 0; i < n; ++i) whole[i] = ldt_crop{0, 0, H[i], W[i], 0};

  // ---- whole images at several output sizes, both filters ----
  static const int kSizes[][2] = {{224, 224}, {7, 5}, {30, 33}, {299, 299}, {1, 1}, {1024, 1024}};
  for (int f = 0; f < 2; ++f)
    for (const auto &sz : kSizes) {
      std::vector<ldt_window> none(n, ldt_window{sz[0], sz[1], 0, 0});
      plan(C, {}, {}, sz[0], sz[1], f, B);
      check_plan(B, whole, none, f, "whole");
      for (size_t i = 0; i < n; ++i)
        if (B.status[i] == LDT_IMG_OK)
          CHECK(B.descs[i].res_h == sz[0] && B.descs[i].res_w == sz[1] && B.descs[i].box_w == W[i], "row %zu desc", i);
    }
  {
    // the default PlanOptions is bilinear: the same plan as filter 0
    BatchPlan B0;
    plan(C, {}, {}, 30, 33, kFilterBilinear, B0);
    PlanOptions opt;
    CHECK(opt.filter == kFilterBilinear, "PlanOptions default filter %d", opt.filter);
    plan(C, {}, {}, 30, 33, kFilterBicubic, B);
    CHECK(B.max_ks_h >= B0.max_ks_h && B.max_ks_v >= B0.max_ks_v && B.max_w == B0.max_w && B.max_h == B0.max_h,
          "bicubic plan against bilinear");
  }

  // ---- the boundary through plan_batch: a box of 148 -> res 8 is 75 taps, 149 fails alone ----
  for (int with_window = 0; with_window < 2; ++with_window) {
    // with_window: the output is a 7 x 5 window of res 8 x 8; without: the output size is 8 x 8
    const int oh = with_window ? 7 : 8, ow = with_window ? 5 : 8;
    std::vector<ldt_window> wn(n, ldt_window{8, 8, 0, 0});
    if (with_window) wn[0] = ldt_window{8, 8, 1, 3};
    std::vector<ldt_crop> cr(n);
    for (size_t i = 0; i < n; ++i) cr[i] = ldt_crop{0, 0, std::min(H[i], 16), std::min(W[i], 16), (int)(i & 1)};
    cr[0] = ldt_crop{3, 5, 148, 148, 1};
    plan(C, cr, with_window ? wn : std::vector<ldt_window>(), oh, ow, kFilterBicubic, B);
    CHECK(B.status[0] == LDT_IMG_OK, "148 -> 8 bicubic (window %d): status %d", with_window, B.status[0]);
    CHECK(B.max_ks_h == 75 && B.max_ks_v == 75, "taps at the limit: %d %d", B.max_ks_h, B.max_ks_v);
    check_plan(B, cr, wn, kFilterBicubic, "148");
    for (const ldt_crop &over : {ldt_crop{3, 5, 148, 149, 1}, ldt_crop{3, 5, 149, 148, 0}}) {
      cr[0] = over;
      plan(C, cr, with_window ? wn : std::vector<ldt_window>(), oh, ow, kFilterBicubic, B);
      CHECK(B.status[0] == LDT_IMG_TOO_LARGE, "149 -> 8 bicubic (window %d): status %d", with_window, B.status[0]);
      for (size_t i = 1; i < n; ++i) CHECK(B.status[i] == LDT_IMG_OK, "neighbour %zu: status %d", i, B.status[i]);
      CHECK(B.max_ks_h == 9 && B.max_ks_v == 9, "taps without the failed row: %d %d", B.max_ks_h, B.max_ks_v);
      check_plan(B, cr, wn, kFilterBicubic, "149");
      plan(C, cr, with_window ? wn : std::vector<ldt_window>(), oh, ow, kFilterBilinear, B);
      CHECK(B.status[0] == LDT_IMG_OK, "149 -> 8 bilinear (window %d): status %d", with_window, B.status[0]);
      check_plan(B, cr, wn, kFilterBilinear, "149 bilinear");
    }
  }

  // ---- the order of a row's errors under bicubic: window 7, then crop 6, then too large 4 ----
  {
    std::vector<ldt_window> wn(n, ldt_window{8, 8, 0, 0});
    std::vector<ldt_crop> cr = whole;
    for (size_t i = 0; i < n; ++i) cr[i] = ldt_crop{0, 0, std::min(H[i], 16), std::min(W[i], 16), 0};
    cr[0] = ldt_crop{0, 0, 149, 149, 0};
    wn[0] = ldt_window{8, 8, 2, 0}; // 7 rows from row 2 of 8: outside
    plan(C, cr, wn, 7, 5, kFilterBicubic, B);
    CHECK(B.status[0] == LDT_IMG_BAD_WINDOW, "bad window + too large: status %d", B.status[0]);
    wn[0] = ldt_window{8, 8, 0, 0};
    cr[0] = ldt_crop{0, 0, H[0] + 1, 149, 0};
    plan(C, cr, wn, 7, 5, kFilterBicubic, B);
    CHECK(B.status[0] == LDT_IMG_BAD_CROP, "bad crop + too large: status %d", B.status[0]);
    cr[0] = ldt_crop{0, 0, 149, 149, 0};
    plan(C, cr, wn, 7, 5, kFilterBicubic, B);
    CHECK(B.status[0] == LDT_IMG_TOO_LARGE, "too large alone: status %d", B.status[0]);
    const ImgDesc &d = B.descs[0];
    CHECK(d.width == 1 && d.height == 1 && d.box_h == 1 && d.box_w == 1 && d.nseg == 0 && d.res_h == 7 && d.res_w == 5,
          "failed row's descriptor is not the 1x1 one");
  }

  free(C.off);
  free(C.data);
  if (!g_fail) printf("filter_plan_ok\n");
  return g_fail;
}
