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
// Output: "row", "seg", "totals", "par_img", "chunk_img", "prog_img", "pscan"
// (every field of each ProgScan), "qtabs" (the device quantisation tables),
// "layout", "sizes" (of the blob's structures) and "hash" (FNV-1a of the
// written blob) lines of key=value fields.
//
// PLAN_HUFF=1 (with PLAN_BATCH=1): after planning, every device Huffman table
// of the batch (BatchPlan::htabs, through each baseline row's dct / act) is
// checked against a plain canonical decoder built here from the row's own DHT
// bytes (T.81 C.2): for all 65,536 16-bit words the entry reached the way the
// kernels reach it (l1 by the top kLookBits bits, then l2[(chunk << kL2Bits) +
// next kL2Bits bits], or the maxcode / valoff / vals search from kLookBits + 1
// bits when l1 says kHuffCanon) must be huff_entry(len, sym, dc) of the code
// the word starts with, or the invalid entry when it starts with none; and
// every count-mode half of lc must be the (T, PRE, ADV) that single-symbol
// steps over the same kLookBits bits give under the rules of ldt_types.hpp.
// Output: one "tab" line per (row, component, class), then "huff_ok"; the
// first mismatch is printed as a "MISMATCH" line and the exit status is 1.
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
    const uint8_t *tabs[3] = {d.bcomp, d.bdx, d.bdy}; // the MCU's blocks, in scan order
    const char *names[3] = {"bcomp", "bdx", "bdy"};
    for (int t = 0; t < 3 && d.bpm > 0; ++t) {
      printf(" %s=", names[t]);
      for (int b = 0; b < d.bpm; ++b) printf(b ? ",%d" : "%d", tabs[t][b]);
    }
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
    printf("pscan data_off=%lld data_len=%lld tab=%d,%d,%d,%d ns=%d comp=%d,%d,%d,%d ss=%d se=%d ah=%d al=%d restart=%d\n",
           (long long)sc.data_off, (long long)sc.data_len, sc.tab[0], sc.tab[1], sc.tab[2], sc.tab[3], sc.ns, sc.comp[0],
           sc.comp[1], sc.comp[2], sc.comp[3], sc.ss, sc.se, sc.ah, sc.al, sc.restart);
  printf("qtabs"); // the device quantisation tables (natural order), 64 values per index of a row's qt
  for (uint16_t q : B.qtabs) printf(" %d", (int)q);
  printf("\n");
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

// ---- PLAN_HUFF: the device tables against the file's own DHT bytes ---------
struct RefTab {
  bool present = false;
  int counts[16];
  std::vector<uint8_t> syms;
  std::string key; // counts + symbols: what makes two tables the same
};

// The DHT tables in force at a baseline file's SOS, its SOF component ids and
// the SOS selectors; a parser of its own (the planner's is the code under test).
struct RefHeader {
  RefTab tab[2][4];
  int ncomp = 0, cid[4], td[4], ta[4];
};

bool ref_header(const uint8_t *b, int64_t n, RefHeader &H) {
  int64_t i = 2;
  while (i + 4 <= n && b[i] == 0xFF) {
    const int m = b[i + 1];
    const int64_t len = (b[i + 2] << 8) | b[i + 3], e = i + 2 + len;
    if (e > n) return false;
    const uint8_t *s = b + i + 4;
    if (m == 0xC4) {
      int64_t p = i + 4;
      while (p + 17 <= e) {
        RefTab &t = H.tab[b[p] >> 4 & 1][b[p] & 3];
        int ns = 0;
        for (int l = 0; l < 16; ++l) ns += t.counts[l] = b[p + 1 + l];
        if (p + 17 + ns > e) return false;
        t.syms.assign(b + p + 17, b + p + 17 + ns);
        t.key.assign(reinterpret_cast<const char *>(b + p + 1), (size_t)(16 + ns));
        t.present = true;
        p += 17 + ns;
      }
    } else if (m == 0xC0 || m == 0xC1) {
      H.ncomp = s[5];
      for (int c = 0; c < H.ncomp && c < 4; ++c) H.cid[c] = s[6 + 3 * c];
    } else if (m == 0xDA) {
      if (s[0] != H.ncomp) return false;
      for (int k = 0; k < H.ncomp; ++k)
        for (int c = 0; c < H.ncomp; ++c)
          if (H.cid[c] == s[1 + 2 * k]) {
            H.td[c] = s[2 + 2 * k] >> 4;
            H.ta[c] = s[2 + 2 * k] & 15;
          }
      return true;
    }
    i = e;
  }
  return false;
}

// Plain canonical decoder: what every 16-bit word starts with.
struct RefDec {
  std::vector<uint8_t> len, sym; // len 0: no code
  explicit RefDec(const RefTab &t) : len(65536, 0), sym(65536, 0) {
    uint32_t code = 0;
    size_t k = 0;
    for (int l = 1; l <= 16; ++l) {
      for (int j = 0; j < t.counts[l - 1]; ++j, ++k, ++code)
        for (uint32_t w = code << (16 - l); w < (code + 1) << (16 - l) && w < 65536; ++w) {
          len[w] = (uint8_t)l;
          sym[w] = t.syms[k];
        }
      code <<= 1;
    }
  }
};

// The entry of the symbol a 16-bit word starts with, read as the kernels read it.
bool device_entry(const HuffTab &t, uint32_t w, bool dc, uint32_t &e, int &path) {
  const uint32_t e1 = t.lc[w >> kL2Bits] & 0xFFFFu;
  e = e1;
  path = 0;
  if ((e1 & 31) != 0) return true;
  if (e1 == kHuffCanon) {
    path = 2;
    for (int l = kLookBits + 1; l <= 16; ++l) {
      const int code = (int)(w >> (16 - l));
      if (code <= t.maxcode[l]) {
        e = huff_entry(l, t.vals[(t.valoff[l] + code) & 0xFF], dc);
        return true;
      }
    }
    e = huff_entry(16, 0, dc);
    return true;
  }
  path = 1;
  const uint32_t chunk = e1 >> 5;
  if (chunk >= (uint32_t)kL2Chunks) return false; // an indirect entry that names no chunk
  e = t.l2[(chunk << kL2Bits) + (w & ((1u << kL2Bits) - 1))];
  return true;
}

// The count-mode half of peek x (kLookBits bits), from single-symbol steps.
uint32_t ref_count_entry(const RefDec &R, uint32_t x, bool dc, uint32_t l1) {
  const uint32_t mask = (1u << kLookBits) - 1;
  const uint32_t w0 = x << kL2Bits;
  if (R.len[w0] == 0 || R.len[w0] > kLookBits) return l1; // no code, or a long one: l1's own entry
  const uint32_t first = huff_entry(R.len[w0], R.sym[w0], dc);
  uint32_t T = first & 31, adv = first >> 9, pre = 0;
  while (!dc && adv < 64 && adv <= 15 && T < (uint32_t)kLookBits) {
    const uint32_t w = ((x << T) & mask) << kL2Bits; // the peek's remaining bits, zero-filled
    const uint32_t l = R.len[w];
    if (l == 0 || T + l > (uint32_t)kLookBits) break; // no code, or one that runs past the peek
    const uint32_t e = huff_entry((int)l, R.sym[w], false);
    pre = adv;
    adv += e >> 9;
    T += e & 31;
  }
  return T | (pre << 5) | (adv << 9);
}

int check_tables(const BatchPlan &B, const uint8_t *data, const std::vector<int64_t> &off, int64_t arr_offset) {
  std::vector<std::string> seen(B.htabs.size()); // key of the DHT table an index was checked against
  int checked = 0;
  for (size_t i = 0; i < B.descs.size(); ++i) {
    const ImgDesc &d = B.descs[i];
    if (B.status[i] != LDT_IMG_OK || d.prog_count > 0) continue;
    RefHeader H;
    const int64_t c0 = off[(size_t)arr_offset + i] - off[(size_t)arr_offset];
    if (!ref_header(data + off[(size_t)arr_offset + i], off[(size_t)arr_offset + i + 1] - off[(size_t)arr_offset + i], H) ||
        H.ncomp != d.ncomp) {
      printf("MISMATCH row=%zu: headers not understood (cell at %lld)\n", i, (long long)c0);
      return 1;
    }
    for (int c = 0; c < d.ncomp; ++c)
      for (int ac = 0; ac < 2; ++ac) {
        const int idx = ac ? d.act[c] : d.dct[c];
        const RefTab &rt = H.tab[ac][ac ? H.ta[c] : H.td[c]];
        const bool dc = !ac;
        if (idx < 0 || idx >= (int)B.htabs.size() || !rt.present) {
          printf("MISMATCH row=%zu comp=%d ac=%d: table index %d\n", i, c, ac, idx);
          return 1;
        }
        const std::string key = (dc ? "D" : "A") + rt.key;
        if (seen[(size_t)idx] == key) continue;
        const HuffTab &t = B.htabs[(size_t)idx];
        const RefDec R(rt);
        const uint32_t invalid = huff_entry(16, 0, dc);
        int npath[3] = {0, 0, 0};
        for (uint32_t w = 0; w < 65536; ++w) {
          uint32_t e;
          int path;
          const bool ok = device_entry(t, w, dc, e, path);
          const uint32_t want = R.len[w] ? huff_entry(R.len[w], R.sym[w], dc) : invalid;
          if (!ok || e != want) {
            printf("MISMATCH row=%zu comp=%d ac=%d idx=%d word=%04x path=%d: entry %04x, canonical decoder %04x\n", i, c,
                   ac, idx, w, path, e, want);
            return 1;
          }
          if (R.len[w]) ++npath[path];
        }
        for (uint32_t x = 0; x < (1u << kLookBits); ++x) {
          const uint32_t l1 = t.lc[x] & 0xFFFFu, got = t.lc[x] >> 16;
          const uint32_t want = ref_count_entry(R, x, dc, l1);
          if (got != want) {
            printf("MISMATCH row=%zu comp=%d ac=%d idx=%d peek=%03x: count entry %04x, single steps give %04x\n", i, c,
                   ac, idx, x, got, want);
            return 1;
          }
        }
        int prefixes = 0, chunks = 0;
        for (uint32_t x = 0; x < (1u << kLookBits); ++x) {
          const uint32_t l1 = t.lc[x] & 0xFFFFu;
          if ((l1 & 31) == 0) {
            ++prefixes;
            if (l1 != kHuffCanon && (int)(l1 >> 5) + 1 > chunks) chunks = (int)(l1 >> 5) + 1;
          }
        }
        printf("tab row=%zu comp=%d ac=%d idx=%d nsym=%zu prefixes=%d chunks=%d words_l1=%d words_l2=%d words_canon=%d\n", i,
               c, ac, idx, rt.syms.size(), prefixes, chunks, npath[0], npath[1], npath[2]);
        seen[(size_t)idx] = key;
        ++checked;
      }
  }
  printf("huff_ok tables=%d\n", checked);
  return 0;
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
  int rc = 0;
  for (int pass = 0; pass < (twice ? 2 : 1); ++pass) {
    Planned P;
    if (use64) plan_and_write(data, off64, arr_offset, valid, opt, cache, labels, P);
    else plan_and_write(data, off32, arr_offset, valid, opt, cache, labels, P);
    if (pass == 0) print_plan(P);
    printf("hash %016llx\n", (unsigned long long)P.hash);
    if (pass == 0 && getenv("PLAN_HUFF") != nullptr) rc = check_tables(P.B, data, off64, arr_offset);
  }
  free(valid);
  free(data);
  return rc;
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
