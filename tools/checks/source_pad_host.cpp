// source_pad_host.cpp — the planner under a source pad (ldt_set_pad with
// LDT_PAD_SOURCE), compiled for the host with ldt_plan.cpp and reachable from
// Python through ctypes (tests/test_source_pad.py): the box check with and
// without the flag, and a batch's row statuses and LDS maxima.
#include <stdint.h>

#include "../../lance-distributed-training_amd/csrc/ldt_pad.hpp"
#include "../../lance-distributed-training_amd/csrc/ldt_plan.hpp"

extern "C" int source_pad_host_mode_ok(int mode) { return ldt::pad_mode_ok(mode); }

extern "C" int source_pad_host_check_crop(int top, int left, int h, int w, int flip, int width, int height, int out_h,
                                          int out_w, int filter, int src_padded) {
  return ldt::check_crop(ldt_crop{top, left, h, w, flip}, width, height, out_h, out_w, filter, src_padded != 0);
}

// Plans n cells (int64 offsets) with `crops` and, when not null, `windows`; src_padded: under a source pad.
// out: the n LDT_IMG_* codes, then max_w, max_h, max_ks_h, max_ks_v of the plan.
extern "C" void source_pad_host_plan(const uint8_t *data, const int64_t *offsets, int64_t n, const ldt_crop *crops,
                                     const ldt_window *windows, int out_h, int out_w, int src_padded, int32_t *out) {
  ldt::PlanOptions opt;
  opt.out_h = out_h;
  opt.out_w = out_w;
  opt.src_padded = src_padded != 0;
  opt.pad = ldt::PadSpec{ldt::kPadReflect, {1, 2, 3}, (uint8_t)(src_padded != 0)};
  ldt::HuffCache cache;
  ldt::BatchPlan B;
  ldt::plan_batch(data, offsets, 0, n, nullptr, opt, cache, B, crops, windows);
  for (int64_t i = 0; i < n; ++i) out[i] = B.status[(size_t)i];
  out[n] = B.max_w, out[n + 1] = B.max_h, out[n + 2] = B.max_ks_h, out[n + 3] = B.max_ks_v;
}
