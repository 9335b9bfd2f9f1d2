// ldt_resample.hpp — Pillow's resample coefficients (Resample.c
// precompute_coeffs + normalize_coeffs_8bpc) for one output index, for the
// convolution filters the resize serves. __host__ __device__ and free of HIP
// calls, so the streaming kernel (k_resize), the cached-table fill
// (k_fill_resample) and a plain C++ program include the same arithmetic:
// tools/checks/resample_check.cpp runs it on the CPU under ASan/UBSan and
// tests/test_interpolation.py compares the two-pass result with Pillow bit for
// bit. IEEE double with contraction off (the pragma under clang/hipcc,
// -ffp-contract=off under another compiler), so the result equals the x86-64
// build of Pillow.
#pragma once
#include <stdint.h>

#include "ldt_types.hpp"

namespace ldt {

// Resample.c bilinear_filter (support 1.0) and bicubic_filter (support 2.0,
// a = -0.5); x >= 0.
template <int FILT>
__host__ __device__ inline double resample_filter(double x) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  if (FILT == kFilterBicubic) {
    const double a = -0.5;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
  }
  return x < 1.0 ? 1.0 - x : 0.0;
}

// The weights of output index xx of (inSize -> outSize), box (0, in), as 22-bit
// fixed point in k[0 .. ksize), zero past the returned count; *xmin_out is the
// first source index. ksize >= resample_ksize_host(inSize, outSize, FILT).
template <int FILT>
__host__ __device__ inline int resample_coeffs(int inSize, int outSize, int xx, int ksize, int32_t *k,
                                               int *xmin_out) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double scale = (double)inSize / (double)outSize;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = (FILT == kFilterBicubic ? 2.0 : 1.0) * filterscale;
  const double center = (xx + 0.5) * scale;
  const double ss = 1.0 / filterscale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > inSize) xmax = inSize;
  xmax -= xmin;
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) {
    double t = ((double)(x + xmin) - center + 0.5) * ss;
    if (t < 0.0) t = -t;
    ww += resample_filter<FILT>(t);
  }
  for (int x = 0; x < ksize; ++x) {
    double wv = 0.0;
    if (x < xmax) {
      double t = ((double)(x + xmin) - center + 0.5) * ss;
      if (t < 0.0) t = -t;
      wv = resample_filter<FILT>(t);
      if (ww != 0.0) wv = wv / ww;
    }
    const double v = wv * (double)(1 << kPrecisionBits);
    k[x] = (int32_t)(wv < 0 ? (-0.5 + v) : (0.5 + v));
  }
  *xmin_out = xmin;
  return xmax;
}

// The taps (inSize -> outSize, BILINEAR) really has: the largest count
// resample_coeffs returns over the output indices. resample_ksize_host is only
// the length of Pillow's coefficient buffer, 2 * ceil(support) + 1; a window is
// the difference of two floors 2 * support apart, so it holds at most
// floor(2 * support) + 1 sources and a cached table row (k_fill_resample, the
// same arithmetic) is zero from this index on. Host only: a loop over the
// whole output, kept once per table entry (ldt_abi.cpp ResampFill).
inline int resample_taps_host(int inSize, int outSize) {
  int taps = 1;
  for (int xx = 0; xx < outSize; ++xx) {
    int xmin;
    const int n = resample_coeffs<kFilterBilinear>(inSize, outSize, xx, 0, nullptr, &xmin);
    if (n > taps) taps = n;
  }
  return taps;
}

// The k_resize4 instantiation that serves `taps` horizontal taps: 3 .. 11, a
// smaller count rounded up (the extra weights are the row's zeros).
inline int resize4_taps(int taps) { return taps < 3 ? 3 : taps; }

// Resample.c clip8 on a 22-bit fixed-point sum: signed, so a negative sum (a
// bicubic undershoot) is 0 and an overshoot 255.
__host__ __device__ __forceinline__ uint32_t clip8(int32_t in) {
  if (in >= (1 << kPrecisionBits << 8)) return 255;
  if (in <= 0) return 0;
  return (uint32_t)(in >> kPrecisionBits);
}

} // namespace ldt
