// Driver for libldt's host planner (csrc/ldt_plan.cpp), built for the CPU with
// -fsanitize=address,undefined by tests/test_plan_fuzz.py. It has no planning
// logic of its own: it calls the plan_batch / plan_layout / write_plan that
// libldt.so's decode_core calls.
// Input on stdin: records of [uint32 little-endian length][bytes].
//
// Default mode: every record is planned alone, as a one-cell batch whose cell
// lies in a heap buffer of exactly its length, so any read past the cell is an
// ASan report. Output: one line per cell, the row's LDT_IMG_* status; with
// PLAN_SCANS=1 preceded by the "offset:length" of each progressive scan.
//
// PLAN_BATCH=1: all records are the cells of one Arrow array in a single heap
// buffer of exactly their total length. Arguments (key=value, all optional):
//   arr_offset=K   the batch is rows K.. of the array (the first K records are not in it)
//   validity=HEX   the array's validity bitmap, hex bytes (bit r of byte r / 8: row r)
//   off64=1        int64 offsets           labels=1   labels (row index * 3) in the blob
//   serial=1       huff_mode serial        fuse=0     no fused destuff
//   win_cap=N      LDS window cap          sb=N       subseq_bits
//   twice=1        plan and write the batch again through the same Huffman cache
// Output: "row", "seg", "totals", "par_img", "chunk_img", "prog_img", "pscan",
// "layout", "sizes" (of the blob's structures) and "hash" (FNV-1a of the
// written blob) lines of key=value fields.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/ldt.h"
#include "../../lance-distributed-training_amd/csrc/ldt_plan.hpp"

using namespace ldt;

namespace {

// The blob as decode_core gets it: planned, laid out, written into a buffer of
// exactly plan_bytes.
struct Planned {
  BatchPlan B;
  PlanLayout L;
  uint64_t hash;
};

template <typename OffT>
void plan_and_write(const uint8_t *data, const std::vector<OffT> &off, int64_t arr_offset, const uint8_t *validity,
                    const PlanOptions &opt, HuffCache &cache, bool with_labels, Planned &P) {
  const int64_t n = (int64_t)off.size() - 1 - arr_offset;
  plan_batch(data, off.data(), arr_offset, n, validity, opt, cache, P.B);
  std::vector<int64_t> labels;
  for (int64_t i = 0; i < n; ++i) labels.push_back(3 * i);
  P.L = plan_layout(P.B, with_labels);
  uint8_t *blob = (uint8_t *)malloc(P.L.plan_bytes ? (size_t)P.L.plan_bytes : 1);
  memset(blob, 0xA5, (size_t)P.L.plan_bytes); // the sections' alignment gaps are not written
  write_plan(P.B, P.L, nullptr, with_labels ? labels.data() : nullptr, blob);
  P.hash = 1469598103934665603ull;
  for (int64_t k = 0; k < P.L.plan_bytes; ++k) P.hash = (P.hash ^ blob[k]) * 1099511628211ull;
  free(blob);
}

void print3(const char *key, const int32_t *v) { printf(" %s=%d,%d,%d", key, v[0], v[1], v[2]); }

void print_list(const char *key, const std::vector<int32_t> &v) {
  printf("%s", key);
  for (int32_t x : v) printf(" %d", x);
  printf("\n");
}

void print_plan(const Planned &P) {
  const BatchPlan &B = P.B;
  for (size_t i = 0; i < B.descs.size(); ++i) {
    const ImgDesc &d = B.descs[i];
    printf("row status=%d width=%d height=%d ncomp=%d color=%d mcux=%d mcuy=%d bpm=%d restart=%d nseg=%d seg_base=%d",
           B.status[i], d.width, d.height, d.ncomp, d.color, d.mcux, d.mcuy, d.bpm, d.restart, d.nseg, d.seg_base);
    printf(" src_off=%lld src_len=%lld dst_off=%lld coef_off=%lld pcoef_off=%lld plane_off=%lld,%lld,%lld",
           (long long)d.src_off, (long long)d.src_len, (long long)d.dst_off, (long long)d.coef_off,
           (long long)d.pcoef_off, (long long)d.plane_off[0], (long long)d.plane_off[1], (long long)d.plane_off[2]);
    print3("plane_stride", d.plane_stride);
    print3("cdw", d.cdw);
    print3("cdh", d.cdh);
    print3("hf", d.hf);
    print3("vf", d.vf);
    print3("ch", d.ch);
    print3("cv", d.cv);
    print3("qt", d.qt);
    print3("dct", d.dct);
    print3("act", d.act);
    printf(" ds_first=%d ds_count=%d sub_bits=%d prog_first=%d prog_count=%d\n", d.ds_first, d.ds_count, d.sub_bits,
           d.prog_first, d.prog_count);
  }
  for (const Segment &s : B.segs) printf("seg img=%d mcu_first=%d mcu_count=%d\n", s.img, s.mcu_first, s.mcu_count);
  printf("totals dst_total=%lld coef_blocks=%lld pcoef_blocks=%lld plane_total=%lld max_blocks=%lld max_window=%lld",
         (long long)B.dst_total, (long long)B.coef_blocks, (long long)B.pcoef_blocks, (long long)B.plane_total,
         (long long)B.max_blocks, (long long)B.max_window);
  printf(" win_bytes=%d n_serial=%d n_chunks=%d n_ds_img=%d max_w=%d max_h=%d max_ks_h=%d max_ks_v=%d max_tabs=%d"
         " n_fast420=%d any_bad=%d nhuff=%zu nquant=%zu nptab=%zu\n",
         B.win_bytes, B.n_serial, B.n_chunks, B.n_ds_img, B.max_w, B.max_h, B.max_ks_h, B.max_ks_v, B.max_tabs,
         B.n_fast420, (int)B.any_bad, B.htabs.size(), B.qtabs.size() / 64, B.ptabs.size());
  print_list("par_img", B.par_img);
  print_list("chunk_img", B.chunk_img);
  print_list("prog_img", B.prog_img);
  for (const ProgScan &sc : B.pscans)
    printf("pscan data_off=%lld data_len=%lld tab=%d,%d,%d,%d\n", (long long)sc.data_off, (long long)sc.data_len,
           sc.tab[0], sc.tab[1], sc.tab[2], sc.tab[3]);
  const PlanLayout &L = P.L;
  printf("layout off_desc=%lld off_seg=%lld off_huff=%lld off_quant=%lld off_lut=%lld off_labels=%lld off_status=%lld"
         " off_par=%lld off_chunk=%lld off_redo=%lld off_pscan=%lld off_ptab=%lld off_pimg=%lld plan_bytes=%lld\n",
         (long long)L.off_desc, (long long)L.off_seg, (long long)L.off_huff, (long long)L.off_quant,
         (long long)L.off_lut, (long long)L.off_labels, (long long)L.off_status, (long long)L.off_par,
         (long long)L.off_chunk, (long long)L.off_redo, (long long)L.off_pscan, (long long)L.off_ptab,
         (long long)L.off_pimg, (long long)L.plan_bytes);
  printf("sizes desc=%zu seg=%zu huff=%zu pscan=%zu ptab=%zu\n", sizeof(ImgDesc), sizeof(Segment), sizeof(HuffTab),
         sizeof(ProgScan), sizeof(ProgTab));
}

int batch_mode(int argc, char **argv, const std::vector<uint8_t> &all, const std::vector<int64_t> &off64) {
  PlanOptions opt;
  int64_t arr_offset = 0;
  bool use64 = false, labels = false, twice = false;
  std::vector<uint8_t> validity;
  for (int a = 1; a < argc; ++a) {
    const char *eq = strchr(argv[a], '=');
    if (!eq) return 2;
    const std::string key(argv[a], (size_t)(eq - argv[a]));
    const char *val = eq + 1;
    if (key == "arr_offset") arr_offset = atoll(val);
    else if (key == "off64") use64 = atoi(val) != 0;
    else if (key == "labels") labels = atoi(val) != 0;
    else if (key == "twice") twice = atoi(val) != 0;
    else if (key == "serial") opt.parallel = atoi(val) == 0;
    else if (key == "fuse") opt.fuse_destuff = atoi(val) != 0;
    else if (key == "win_cap") opt.win_cap = atoll(val);
    else if (key == "sb") opt.subseq_bits = atoi(val);
    else if (key == "validity") {
      for (size_t k = 0; k + 1 < strlen(val); k += 2) {
        const char byte[3] = {val[k], val[k + 1], 0};
        validity.push_back((uint8_t)strtoul(byte, nullptr, 16));
      }
    } else return 2;
  }
  const int64_t rows = (int64_t)off64.size() - 1;
  if (arr_offset < 0 || arr_offset > rows) return 2;
  if (!validity.empty() && (int64_t)validity.size() * 8 < rows) return 2;
  // exact-size heap copies, so ASan sees any read past the cells or the bitmap
  uint8_t *data = (uint8_t *)malloc(all.empty() ? 1 : all.size());
  if (!all.empty()) memcpy(data, all.data(), all.size());
  uint8_t *valid = nullptr;
  if (!validity.empty()) {
    valid = (uint8_t *)malloc(validity.size());
    memcpy(valid, validity.data(), validity.size());
  }
  const std::vector<int32_t> off32(off64.begin(), off64.end());
  HuffCache cache;
  for (int pass = 0; pass < (twice ? 2 : 1); ++pass) {
    Planned P;
    if (use64) plan_and_write(data, off64, arr_offset, valid, opt, cache, labels, P);
    else plan_and_write(data, off32, arr_offset, valid, opt, cache, labels, P);
    if (pass == 0) print_plan(P);
    printf("hash %016llx\n", (unsigned long long)P.hash);
  }
  free(valid);
  free(data);
  return 0;
}

} // namespace

int main(int argc, char **argv) {
  const bool print_scans = getenv("PLAN_SCANS") != nullptr; // also print each scan's (offset, length)
  const bool batch = getenv("PLAN_BATCH") != nullptr;
  std::vector<uint8_t> all;
  std::vector<int64_t> off(1, 0);
  HuffCache cache;
  uint32_t n;
  while (fread(&n, 4, 1, stdin) == 1) {
    uint8_t *cell = (uint8_t *)malloc(n ? n : 1);
    if (n && fread(cell, 1, n, stdin) != n) return 2;
    if (batch) {
      all.insert(all.end(), cell, cell + n);
      off.push_back((int64_t)all.size());
    } else {
      Planned P;
      plan_and_write(cell, std::vector<int64_t>{0, (int64_t)n}, 0, nullptr, PlanOptions(), cache, false, P);
      if (print_scans)
        for (const ProgScan &sc : P.B.pscans) printf("%lld:%lld ", (long long)sc.data_off, (long long)sc.data_len);
      printf("%d\n", P.B.status[0]);
    }
    free(cell);
  }
  return batch ? batch_mode(argc, argv, all, off) : 0;
}
