// ldt_pad.hpp — the index map of a padded window (ldt_set_pad): where index i
// of an axis of the padded image reads an axis of n resized pixels, in
// torchvision Pad's four modes. One source for the streaming resize
// (ldt_resize_stream.hpp), the planner and the CPU check against np.pad
// (tools/checks/pad_host.cpp, tests/test_pad_ops.py), so it is plain integer
// arithmetic with no HIP call.
//
// What is restated:
//   constant   ImageOps.expand(fill=): an index outside 0..n-1 is the fill colour
//   edge       np.pad(mode="edge"): clamp(i, 0, n - 1)
//   reflect    np.pad(mode="reflect"): periodic with period 2 (n - 1), the edge
//              not repeated; n == 1 reads pixel 0
//   symmetric  np.pad(mode="symmetric"): periodic with period 2 n, the edge repeated
// for any overhang: an index many periods away folds as often as it takes.
#pragma once
#include <stdint.h>

#include "../../include/ldt.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LDT_PAD_HD __host__ __device__ inline
#else
#define LDT_PAD_HD inline
#endif

namespace ldt {

constexpr int kPadConstant = 0, kPadEdge = 1, kPadReflect = 2, kPadSymmetric = 3;
static_assert(kPadConstant == LDT_PAD_CONSTANT && kPadEdge == LDT_PAD_EDGE && kPadReflect == LDT_PAD_REFLECT &&
                  kPadSymmetric == LDT_PAD_SYMMETRIC,
              "ldt.h and ldt_pad.hpp disagree");
constexpr int kPadFill = -1; // pad_index: the fill colour, no pixel

// A call's pad: the mode (one of the four, without the flag), the fill colour
// (RGB bytes, read in constant mode only) and which side it pads: 0 the window
// in the resized image, 1 the source ahead of the resize (LDT_PAD_SOURCE: the
// axis is then the decoded image's and i an index of the crop box).
struct PadSpec {
  int32_t mode;
  uint8_t fill[3];
  uint8_t source;
};
// The source pad as a kernel argument: a type of its own, so that a kernel's
// trailing pack tells the two pads apart (ldt_resize_stream.hip).
struct SrcPadSpec {
  PadSpec p;
};

// What ldt_set_pad takes: one of the four modes, LDT_PAD_SOURCE or'ed on or not.
LDT_PAD_HD bool pad_mode_ok(int mode) {
  return (mode & ~LDT_PAD_SOURCE) >= kPadConstant && (mode & ~LDT_PAD_SOURCE) <= kPadSymmetric;
}

// i mod p for p > 0, in 0..p-1 for a negative i too.
LDT_PAD_HD int pad_mod(int i, int p) {
  const int r = i % p;
  return r < 0 ? r + p : r;
}

// The pixel of 0..n-1 (n >= 1) that index i reads, or kPadFill. |i| and n stay
// below 2^30, so no sum here overflows.
LDT_PAD_HD int pad_index(int mode, int i, int n) {
  if (i >= 0 && i < n) return i;
  if (mode == kPadConstant) return kPadFill;
  if (mode == kPadEdge) return i < 0 ? 0 : n - 1;
  if (mode == kPadReflect) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1), r = pad_mod(i, p);
    return r < n ? r : p - r;
  }
  const int p = 2 * n, r = pad_mod(i, p);
  return r < n ? r : p - 1 - r;
}

// Whether any index of lo .. lo + count - 1 reads a pixel: false only in
// constant mode, for a run wholly outside 0..n-1.
LDT_PAD_HD bool pad_run_has_pixels(int mode, int lo, int count, int n) {
  return mode != kPadConstant || (lo < n && lo + count > 0);
}

} // namespace ldt
