// affine_filter_host.cpp — csrc/ldt_augment.hpp's filtered affine op compiled
// for the host: the arithmetic k_aug_affine_filt runs, on an [h][w][3] uint8
// image, for the check against Pillow's Image.transform(AFFINE, BILINEAR |
// BICUBIC) in tests/test_affine_filter_ops.py. Build with -ffp-contract=off.
#include <stdint.h>

#include "../../lance-distributed-training_amd/csrc/ldt_augment.hpp"

namespace {

struct HostTap {
  const uint8_t *rgb;
  int w;
  uint32_t operator()(int xc, int yc) const {
    const uint8_t *p = rgb + ((int64_t)yc * w + xc) * 3;
    return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
  }
};

} // namespace

extern "C" {

// The kernel's tile (rows, columns) and the texels its LDS stages, for the
// check of the Python mirror (_lib.AFFINE_TILE, _lib.AFFINE_LDS_TEXELS).
void affine_filter_host_consts(int *c) {
  c[0] = ldt::kAffTileH, c[1] = ldt::kAffTileW, c[2] = ldt::kAffLdsTexels;
}

// filter: 1 bilinear, 2 bicubic. The image is walked in the kernel's tiles,
// and a tap outside its tile's box (aug_filt_box) counts as an error: the
// return value is their number.
int affine_filter_host_run(const uint8_t *rgb, int h, int w, int filter, const double *m, const uint8_t *fill,
                           uint8_t *out) {
  using namespace ldt;
  const int th = kAffTileH, tw = kAffTileW;
  int escaped = 0;
  for (int ty = 0; ty < h; ty += th)
    for (int tx = 0; tx < w; tx += tw) {
      const int x1 = (tx + tw < w ? tx + tw : w) - 1, y1 = (ty + th < h ? ty + th : h) - 1;
      int box[4] = {0, 0, -1, -1};
      const bool any = aug_filt_box(m, filter, tx, ty, x1, y1, w, h, box);
      for (int y = ty; y <= y1; ++y)
        for (int x = tx; x <= x1; ++x) {
          uint8_t *o = out + ((int64_t)y * w + x) * 3;
          double xin, yin;
          aug_filt_coords(m, x, y, xin, yin);
          if (!any || !aug_filt_inside(xin, yin, w, h)) { // !any: the kernel's fill without the coordinates
            o[0] = fill[0], o[1] = fill[1], o[2] = fill[2];
            continue;
          }
          const HostTap base{rgb, w};
          const auto tap = [&](int xc, int yc) {
            if (xc < box[0] || xc > box[2] || yc < box[1] || yc > box[3]) ++escaped;
            return base(xc, yc);
          };
          int px[3];
          if (filter == kAffBicubic) aug_filt_pixel<kAffBicubic>(xin, yin, w, h, tap, px);
          else aug_filt_pixel<kAffBilinear>(xin, yin, w, h, tap, px);
          o[0] = (uint8_t)px[0], o[1] = (uint8_t)px[1], o[2] = (uint8_t)px[2];
        }
    }
  return escaped;
}

} // extern "C"
