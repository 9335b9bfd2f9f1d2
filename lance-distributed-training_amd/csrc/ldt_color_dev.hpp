// ldt_color_dev.hpp — device helpers shared by the kernels that follow the
// resize of a call with a workspace (ldt_color.hip, ldt_augment.hip): the work
// of a workgroup from the call's ColorGeom, the quad load from the workspace's
// planes and the quad store in the call's dtype and layout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ldt_device.hpp"
#include "ldt_kernels.hpp"

namespace ldt {

namespace {

constexpr int kColorThreads = 256;

// The work of workgroup L: its output image, view and rows.
struct ColorWork {
  int img, view, y0, rows, oh, ow;
  int64_t base; // first element of the image's three planes (bytes in the workspace)
};

__device__ __forceinline__ ColorWork color_work(const ColorGeom &g, int L, int n) {
  ColorWork k;
  k.img = L / g.tiles;
  const int t = L - k.img * g.tiles;
  int view = 0;
#pragma unroll
  for (int u = 1; u < kMaxViews; ++u)
    if (u < g.views && t >= g.tile0[u]) view = u;
  k.view = view;
  k.oh = g.oh[view];
  k.ow = g.ow[view];
  k.y0 = (t - g.tile0[view]) * kColorRows;
  k.rows = min(kColorRows, k.oh - k.y0);
  k.base = g.base[view] + (int64_t)k.img * 3 * k.oh * k.ow;
  return k;
}

// Four consecutive pixels of one plane row at p (cnt of them inside the row),
// as bytes of a dword: one load when p is dword-aligned and the quad is whole.
__device__ __forceinline__ uint32_t load_quad(const uint8_t *p, int cnt) {
  if (cnt == 4 && (((uintptr_t)p) & 3) == 0) return *reinterpret_cast<const uint32_t *>(p);
  uint32_t v = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (e < cnt) v |= (uint32_t)p[e] << (8 * e);
  return v;
}

// The table's values v[channel][pixel] of four consecutive pixels of a row
// (cnt of them inside it), the first at pixel `at` of the image's planes, whose
// first element is ob: the store in the call's dtype and layout.
__device__ __forceinline__ void store_quad(uint8_t *ob, const OutFmt &fmt, int es, int64_t plane, int64_t at, int cnt,
                                           const uint32_t (&v)[3][4]) {
  if (fmt.layout == kLayoutNHWC) {
    // twelve consecutive elements
    uint8_t *q = ob + at * 3 * es;
    if (cnt == 4 && (((uintptr_t)q) & (4 * es - 1)) == 0) {
      fmt_store4(q, es, v[0][0], v[1][0], v[2][0], v[0][1]);
      fmt_store4(q + 4 * es, es, v[1][1], v[2][1], v[0][2], v[1][2]);
      fmt_store4(q + 8 * es, es, v[2][2], v[0][3], v[1][3], v[2][3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < cnt) {
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) fmt_store1(q + (3 * e + ch) * es, es, v[ch][e]);
        }
    }
  } else {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      uint8_t *q = ob + (ch * plane + at) * es;
      if (cnt == 4 && (((uintptr_t)q) & (4 * es - 1)) == 0) {
        fmt_store4(q, es, v[ch][0], v[ch][1], v[ch][2], v[ch][3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < cnt) fmt_store1(q + e * es, es, v[ch][e]);
      }
    }
  }
}

} // namespace

} // namespace ldt
