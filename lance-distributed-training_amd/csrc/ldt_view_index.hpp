// ldt_view_index.hpp — the geometry of a call whose views have their own
// output sizes (ldt_set_view_sizes): the per-view table, and the map from a
// linear workgroup index of k_resize_views to (image, view, band, tile) under
// both grid orders. Shared by the host planner (plan_batch builds the table),
// the kernel (ldt_resize_stream.hip decodes blockIdx.x with it) and the CPU
// test that walks every index (tests/fuzz/view_sizes_plan_check.cpp), so it is
// plain integer code with no HIP call.
//
// A view of h x w takes NB = ceil(h / 8) bands times NT = ceil(w / 256) tiles
// per image. Workgroups are counted per group of 8 images: view v has
// wg[v] = 8 * NB_v * NT_v of them in a group, a multiple of 8, so in both
// orders index % 8 == image % 8 (ldt_resize_stream.hip says why that matters):
//   order 0   group of 8 images, then view, then band and tile, then image % 8:
//             index = g * P + pre0[v] + (band * NT_v + tile) * 8 + image % 8,
//             pre0[v] = sum of wg[u] over u < v, P their sum over all views
//   order 1   view-major: index = pre1[v] + g * wg[v] + (band * NT_v + tile) * 8
//             + image % 8, pre1[v] = groups * pre0[v]
// Images past n in the last group are padding: they decode to image >= n.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LDT_HD __host__ __device__
#else
#define LDT_HD
#endif

namespace ldt {

constexpr int kViewGeomMax = 16;     // kMaxViews / LDT_MAX_VIEWS
constexpr int kViewGeomBandRows = 8; // kBandRows
constexpr int kViewGeomTileCols = 256; // kTileCols

struct ViewGeom {
  int32_t oh, ow;     // the view's output size
  int32_t nb, nt;     // bands ceil(oh / 8), tiles ceil(ow / 256)
  int32_t pre0, pre1; // workgroups before the view: in a group of 8 images (order 0), in the grid (order 1)
  int64_t base;       // first element of the view's dense [n, 3, oh, ow] block in the output
};

struct ViewGeomTab {
  ViewGeom g[kViewGeomMax];
  int32_t views;     // 0: the call has no per-view sizes
  int32_t per_group; // P: workgroups of one group of 8 images, all views
  int32_t groups;    // ceil(n / 8)
  int32_t max_ow;    // the widest view: what the LDS layout is sized for
  int64_t total;     // groups * per_group: the grid
  int64_t elems;     // elements of the whole output: n * 3 * sum h * w
};

// Fills `t` for n images and `views` sizes hw[v] = (h, w). False, with
// t.views = 0, when an argument is out of range (views outside 1..16, a size
// outside 1..max_out, n < 0) or the grid would pass what a launch takes (2^31
// - 1 workgroups); every product is formed in 64 bits from bounded factors, so
// nothing overflows on the way to that answer.
inline bool view_geom_build(int64_t n, int views, const int32_t *hw, int max_out, ViewGeomTab &t) {
  t = ViewGeomTab();
  if (views < 1 || views > kViewGeomMax || hw == nullptr || n < 0 || n > 0x7FFFFFFF) return false;
  const int64_t groups = (n + 7) / 8;
  int64_t pre = 0, base = 0;
  int max_ow = 1;
  ViewGeom g[kViewGeomMax] = {};
  for (int v = 0; v < views; ++v) {
    const int32_t h = hw[2 * v], w = hw[2 * v + 1];
    if (h < 1 || h > max_out || w < 1 || w > max_out) return false;
    g[v].oh = h;
    g[v].ow = w;
    g[v].nb = (h + kViewGeomBandRows - 1) / kViewGeomBandRows;
    g[v].nt = (w + kViewGeomTileCols - 1) / kViewGeomTileCols;
    // pre <= 16 * 8 * 128 * 4 and groups < 2^28: pre * groups < 2^45
    if (pre * groups > 0x7FFFFFFF) return false;
    g[v].pre0 = (int32_t)pre;
    g[v].pre1 = (int32_t)(pre * groups);
    g[v].base = base;
    pre += (int64_t)8 * g[v].nb * g[v].nt;
    base += n * 3 * h * w; // n < 2^31, 3 * h * w < 2^22, 16 views: < 2^57
    if (w > max_ow) max_ow = w;
  }
  if (pre * groups > 0x7FFFFFFF || n * views > 0x7FFFFFFF) return false;
  for (int v = 0; v < views; ++v) t.g[v] = g[v];
  t.views = views;
  t.per_group = (int32_t)pre;
  t.groups = (int32_t)groups;
  t.max_ow = max_ow;
  t.total = pre * groups;
  t.elems = base;
  return true;
}

struct ViewWork {
  int32_t img, view, band, tile;
};

// Workgroup `index` (0 <= index < t.total) of grid order `order`. The view is
// found by walking the at most 16 prefixes: uniform over the workgroup.
LDT_HD inline ViewWork view_work(const ViewGeomTab &t, int order, int32_t index) {
  int32_t g, q = index;
  if (order == 0) {
    g = index / t.per_group;
    q = index - g * t.per_group;
  }
  int view = 0;
  for (int u = 1; u < kViewGeomMax; ++u)
    if (u < t.views && q >= (order == 0 ? t.g[u].pre0 : t.g[u].pre1)) view = u;
  const int32_t nt = t.g[view].nt;
  int32_t rr;
  if (order == 0) {
    rr = q - t.g[view].pre0;
  } else {
    const int32_t wg = 8 * t.g[view].nb * nt;
    q -= t.g[view].pre1;
    g = q / wg;
    rr = q - g * wg;
  }
  ViewWork r;
  r.img = g * 8 + (rr & 7);
  r.view = view;
  r.band = (rr >> 3) / nt;
  r.tile = (rr >> 3) % nt;
  return r;
}

} // namespace ldt
