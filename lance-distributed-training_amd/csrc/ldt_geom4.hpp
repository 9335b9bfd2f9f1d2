// ldt_geom4.hpp — launch geometry of the one-wave-per-band resize kernel
// (k_resize4, ldt_resize4.hip): how an output of out_h x out_w is cut into
// bands and how much LDS a wave needs. Plain host arithmetic, no HIP call, so
// tools/checks/geom4_check.cpp sweeps it on the CPU under ASan/UBSan
// (tests/test_output_size.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ldt_types.hpp"

namespace ldt {

struct Geom4 {
  int nbands, bh;  // bands per image, output rows per band
  int ring;        // intermediate ring rows (ks_v + 1)
  int ks_v;        // vertical taps (max over the batch): the real counts of heights with a table entry
                   // (resample_taps_host), Pillow's capacity (resample_ksize_host) for the others
  int spad;        // staging row stride in dwords (multiple of 4)
  int ntask;       // n * nbands
  int wave_bytes;  // LDS per wave
  int fill;        // JPEG: this launch zero-fills failed images' bands (label -100)
  int wpg;         // waves (tasks) per workgroup
  int rgbx;        // ring rows of RGBx dwords (JPEG sources) instead of three byte planes
  int vcalc;       // an image has no vertical table entry: LDS for computed vertical coefficients
  // the generic-width kernel only (the kOut x kOut instantiations have these compiled in)
  int oh, ow;      // output size
  int ows;         // ring row stride in columns: ow rounded up to a multiple of 4
  int vec4;        // float4 stores: ow % 4 == 0 and the output 16-byte aligned; the FMT instantiations
                   // (ldt_set_output_format), which test every store's own address: kDtype* | kLayout* << 8
  int vmax_in;     // heights up to this may have a vertical table entry (resamp_cached)
  const int32_t *tab_v; // the vertical table (rows of oh entries)
};

constexpr int kKvRows = 8; // computed vertical coefficient rows held per wave (Geom4::vcalc)
constexpr int kResize4Lut = 3072;          // the workgroup's LUT ahead of the waves' buffers
constexpr int kResize4LdsMax = 160 * 1024; // LDS of a gfx950 workgroup

inline int wave_bytes4(const Geom4 &g) {
  const int b = 8 * g.spad + (g.rgbx ? 4 : 3) * g.ring * g.ows +
                (g.vcalc ? 4 * (kKvRows * g.ks_v + 2 * kKvRows) : 0);
  return (b + 15) & ~15;
}

// Geometry for n images of up to max_w x max_h resized to oh x ow (ow <=
// kTileCols) in about waves_target bands. ks_h: the kernel's horizontal taps
// (its KS: the batch's real count, resize4_taps); ks_v: the batch's vertical
// taps (Geom4::ks_v). vmax_in: the vertical table's input limit
// (kResampMaxSize for the kOut table). False: a workgroup's LDS does not hold
// wpg waves of this shape.
inline bool make_geom4(int n, int max_w, int max_h, int ks_h, int ks_v, int waves_target, Geom4 &g, int wpg,
                       bool jpeg, int oh = kOut, int ow = kOut, int vmax_in = kResampMaxSize) {
  g.wpg = wpg;
  g.rgbx = jpeg ? 1 : 0;
  g.oh = oh;
  g.ow = ow;
  g.ows = (ow + 3) & ~3;
  g.vmax_in = vmax_in;
  g.ks_v = ks_v;
  g.vcalc = resamp_cached(max_h, oh, vmax_in) ? 0 : 1;
  // Rows come in pairs and a pair's finished output rows are stored before
  // the pair's own horizontal pass (vertical(y), then horizontal(y)): a
  // pending row's window then spans at most ks_v - 1 ring rows ahead of the
  // pair, which writes two more (tools/checks/taps_check.cpp replays it).
  g.ring = g.ks_v + 1;
  if (jpeg) {
    // Plain rows: the staging writes whole 8-pixel blocks up to the row's end.
    // The taps read [xmin, xmin + ks_h) with xmin + count <= width, so past a
    // row's last pixel they read at most ks_h - 1 dwords of what follows in
    // the wave's buffer (the second row, then the ring), each times a zero
    // weight; wave_bytes below keeps those reads inside the wave's own bytes.
    g.spad = ((max_w + 7) / 8) * 8;
  } else {
    // raw rows are skewed (skw)
    const int px = ((max_w + 15) / 16) * 16 + ks_h + 16;
    g.spad = (px + ((px >> 5) << 2) + 4 + 3) & ~3;
  }
  g.wave_bytes = wave_bytes4(g);
  const int reach = (4 * (2 * g.spad + ks_h) + 15) & ~15; // the second row's last tap
  if (jpeg && g.wave_bytes < reach) g.wave_bytes = reach;
  int nb = (waves_target + n - 1) / n;
  const int nb_max = (oh + 7) / 8; // bands of at least 8 rows (28 at 224)
  if (nb < 1) nb = 1;
  if (nb > nb_max) nb = nb_max;
  g.bh = (oh + nb - 1) / nb;
  g.nbands = (oh + g.bh - 1) / g.bh;
  g.ntask = n * g.nbands;
  return kResize4Lut + g.wpg * (size_t)g.wave_bytes <= (size_t)kResize4LdsMax;
}

} // namespace ldt
