// Driver for the draft handling of libldt's host planner (csrc/ldt_plan.cpp),
// built for the CPU with -fsanitize=address,undefined by tests/test_draft.py
// and run directly. It calls the plan_batch that libldt.so calls, with draft
// scales (ldt_set_draft hands them to plan_batch unchanged).
//
// Arguments: out_h out_w, then one scale per cell. Input on stdin: records of
// [uint32 little-endian length][bytes], one JPEG cell each. The cells, their
// offsets and the scales live in heap buffers of exactly their size. Output:
// one line per row,
//   row i status S width W height H draft D nofancy F n_draft N max_w MW max_h MH box T L BH BW
//   and per component: comp k sc cdw cdh hf vf stride off
// then "plane_total P", and "draft_plan_ok".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/ldt.h"
#include "../../lance-distributed-training_amd/csrc/ldt_plan.hpp"

using namespace ldt;

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  std::vector<uint8_t> bytes;
  std::vector<int64_t> offs{0};
  for (;;) {
    uint32_t len;
    if (fread(&len, 4, 1, stdin) != 1) break;
    const size_t at = bytes.size();
    bytes.resize(at + len);
    if (len && fread(bytes.data() + at, 1, len, stdin) != len) return 2;
    offs.push_back((int64_t)bytes.size());
  }
  const int64_t n = (int64_t)offs.size() - 1;
  if (argc - 3 != n) return 2;
  uint8_t *data = (uint8_t *)malloc(bytes.size() ? bytes.size() : 1);
  memcpy(data, bytes.data(), bytes.size());
  int64_t *off = (int64_t *)malloc(sizeof(int64_t) * offs.size());
  memcpy(off, offs.data(), sizeof(int64_t) * offs.size());
  int32_t *scales = (int32_t *)malloc(sizeof(int32_t) * (n ? n : 1));
  for (int64_t i = 0; i < n; ++i) scales[i] = atoi(argv[3 + i]);
  PlanOptions opt;
  opt.out_h = atoi(argv[1]);
  opt.out_w = atoi(argv[2]);
  HuffCache cache;
  BatchPlan B;
  plan_batch(data, off, 0, n, nullptr, opt, cache, B, nullptr, nullptr, 1, nullptr, scales);
  // the blob is written from the descriptors: lay it out and write it too
  const PlanLayout L = plan_layout(B, false);
  uint8_t *blob = (uint8_t *)malloc((size_t)L.plan_bytes);
  write_plan(B, L, nullptr, nullptr, blob);
  const ImgDesc *descs = reinterpret_cast<const ImgDesc *>(blob + L.off_desc);
  for (int64_t i = 0; i < n; ++i) {
    const ImgDesc &d = descs[i];
    printf("row %lld status %d width %d height %d draft %d nofancy %d n_draft %d max_w %d max_h %d box %d %d %d %d\n",
           (long long)i, B.status[(size_t)i], d.width, d.height, d.draft, d.nofancy, B.n_draft, B.max_w, B.max_h,
           d.box_top, d.box_left, d.box_h, d.box_w);
    for (int k = 0; k < d.ncomp; ++k)
      printf("comp %d %d %d %d %d %d %d %lld\n", k, d.sc[k], d.cdw[k], d.cdh[k], d.hf[k], d.vf[k], d.plane_stride[k],
             (long long)d.plane_off[k]);
  }
  printf("plane_total %lld\n", (long long)B.plane_total);
  free(blob);
  free(scales);
  free(off);
  free(data);
  printf("draft_plan_ok\n");
  return 0;
}
