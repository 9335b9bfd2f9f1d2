// native_sizes_host.cpp — the planner of a native call with per-row sizes
// (ldt_set_native_sizes) as a host library: built with ldt_plan.cpp by
// tests/test_native_sizes.py, no HIP call, no device.
#include <stdint.h>

#include "../../lance-distributed-training_amd/csrc/ldt_plan.hpp"

// Plans n cells (int64 offsets) as a native call with `native` offsets (n + 1)
// and `sizes` (n pairs (h, w)) under `filter`; crops may be null.
// out: the n LDT_IMG_* codes, the n + 1 entries of the tile prefix, then
// native_bad, max_ks_h, max_ks_v, rag.kh_words, rag.ks_v, rag.span, the LDS
// bytes of the launch and kRagTileRows.
extern "C" void native_sizes_host_plan(const uint8_t *data, const int64_t *offsets, int64_t n, const int64_t *native,
                                       const int32_t *sizes, const ldt_crop *crops, int filter, int32_t *out) {
  ldt::PlanOptions opt;
  opt.native = true;
  opt.filter = filter;
  ldt::HuffCache cache;
  ldt::BatchPlan B;
  ldt::plan_batch(data, offsets, 0, n, nullptr, opt, cache, B, crops, nullptr, 1, nullptr, nullptr, native, sizes);
  for (int64_t i = 0; i < n; ++i) out[i] = B.status[(size_t)i];
  for (int64_t i = 0; i <= n; ++i) out[n + i] = B.nat_tiles[(size_t)i];
  int32_t *m = out + 2 * n + 1;
  m[0] = B.native_bad, m[1] = B.max_ks_h, m[2] = B.max_ks_v, m[3] = B.rag.kh_words, m[4] = B.rag.ks_v, m[5] = B.rag.span;
  m[6] = ldt::ragged_lds(B.rag).bytes, m[7] = ldt::kRagTileRows;
}
