// pad_host.cpp — csrc/ldt_pad.hpp compiled for the host: the index map the
// streaming resize runs under a pad (ldt_set_pad), reachable from Python
// through ctypes (tests/test_pad_ops.py holds it against np.pad). Built with
// ldt_plan.cpp and -DPAD_HOST_PLAN it also exports the planner's window check
// and a batch's row statuses with and without a pad (tests/test_pad.py).
#include <stdint.h>

#include "../../lance-distributed-training_amd/csrc/ldt_pad.hpp"

// out[k] = pad_index(mode, lo + k, n) for k in 0..count-1 (kPadFill = -1).
extern "C" void pad_host_indices(int mode, int lo, int count, int n, int32_t *out) {
  for (int k = 0; k < count; ++k) out[k] = ldt::pad_index(mode, lo + k, n);
}

#ifdef PAD_HOST_PLAN
#include "../../lance-distributed-training_amd/csrc/ldt_plan.hpp"

extern "C" int pad_host_check_window(int res_h, int res_w, int top, int left, int out_h, int out_w, int padded) {
  return ldt::check_window(ldt_window{res_h, res_w, top, left}, out_h, out_w, padded != 0);
}

// Plans n cells (int64 offsets) with `windows` and, when not null, `crops`; mode < 0: no pad.
// out: the n LDT_IMG_* codes, then max_w, max_ks_h, max_ks_v of the plan.
extern "C" void pad_host_plan(const uint8_t *data, const int64_t *offsets, int64_t n, const ldt_window *windows,
                              const ldt_crop *crops, int out_h, int out_w, int mode, int32_t *out) {
  ldt::PlanOptions opt;
  opt.out_h = out_h;
  opt.out_w = out_w;
  opt.padded = mode >= 0;
  opt.pad = ldt::PadSpec{mode, {1, 2, 3}, 0};
  ldt::HuffCache cache;
  ldt::BatchPlan B;
  ldt::plan_batch(data, offsets, 0, n, nullptr, opt, cache, B, crops, windows);
  for (int64_t i = 0; i < n; ++i) out[i] = B.status[(size_t)i];
  out[n] = B.max_w, out[n + 1] = B.max_ks_h, out[n + 2] = B.max_ks_v;
}
#endif
