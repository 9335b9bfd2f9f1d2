// ldt_plan.cpp — host planner (see ldt_plan.hpp). Restates libjpeg-turbo
// jdmarker.c (marker parsing), jdhuff.c jpeg_make_d_derived_tbl and
// jdphuff.c's progression checks for the subset the device kernels decode,
// then plans the batch from those headers (plan_batch) and writes the plan
// blob (plan_layout, write_plan). No HIP calls: built into libldt.so and, for
// the planner tests, alone with -fsanitize=address,undefined.
#include "ldt_plan.hpp"

#include <stdint.h>
#include <string.h>
#include <emmintrin.h>

#include <algorithm>

namespace ldt {

namespace {

const uint8_t kZigzagToNatural[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

inline int be16(const uint8_t *p) { return (p[0] << 8) | p[1]; }

} // namespace

// Returns an LDT_IMG_* code.
int walk_markers(const uint8_t *cell, int64_t len, Header &H) {
  for (int i = 0; i < 4; ++i) H.dc[i].present = H.ac[i].present = false;
  if (len < 4 || cell[0] != 0xFF || cell[1] != 0xD8) return LDT_IMG_NOT_JPEG;
  int64_t i = 2;
  bool sof = false;
  while (true) {
    if (i + 1 >= len) return LDT_IMG_NOT_JPEG;
    if (cell[i] != 0xFF) return LDT_IMG_NOT_JPEG;
    while (i + 1 < len && cell[i + 1] == 0xFF) ++i; // fill bytes
    if (i + 1 >= len) return LDT_IMG_NOT_JPEG;
    const int m = cell[i + 1];
    i += 2;
    if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
    if (m == 0xD9) return LDT_IMG_NOT_JPEG;
    if (i + 2 > len) return LDT_IMG_NOT_JPEG;
    const int seglen = be16(cell + i);
    if (seglen < 2 || i + seglen > len) return LDT_IMG_NOT_JPEG;
    const uint8_t *s = cell + i + 2;
    const uint8_t *e = cell + i + seglen;
    switch (m) {
    case 0xC0:
    case 0xC1:
    case 0xC2: {
      if (sof) return LDT_IMG_NOT_JPEG; // two SOF markers
      H.progressive = m == 0xC2;
      if (e - s < 6) return LDT_IMG_NOT_JPEG;
      if (s[0] != 8) return LDT_IMG_UNSUPPORTED;
      H.height = be16(s + 1);
      H.width = be16(s + 3);
      H.ncomp = s[5];
      if (H.width == 0 || H.height == 0) return LDT_IMG_NOT_JPEG;
      if (H.ncomp != 1 && H.ncomp != 3) return LDT_IMG_UNSUPPORTED;
      if (e - s < 6 + 3 * H.ncomp) return LDT_IMG_NOT_JPEG;
      for (int c = 0; c < H.ncomp; ++c) {
        H.cid[c] = s[6 + 3 * c];
        H.h[c] = s[7 + 3 * c] >> 4;
        H.v[c] = s[7 + 3 * c] & 15;
        H.tq[c] = s[8 + 3 * c];
        if (H.h[c] < 1 || H.h[c] > 4 || H.v[c] < 1 || H.v[c] > 4 || H.tq[c] > 3)
          return LDT_IMG_NOT_JPEG;
      }
      sof = true;
      break;
    }
    case 0xC3: case 0xC5: case 0xC6: case 0xC7: case 0xC9: case 0xCA:
    case 0xCB: case 0xCD: case 0xCE: case 0xCF:
      return LDT_IMG_UNSUPPORTED;
    case 0xC4: {
      while (s < e) {
        const int tc = s[0] >> 4, th = s[0] & 15;
        if (tc > 1 || th > 3 || e - s < 17) return LDT_IMG_NOT_JPEG;
        RawHuff &t = tc ? H.ac[th] : H.dc[th];
        int n = 0;
        for (int l = 0; l < 16; ++l) {
          t.counts[l] = s[1 + l];
          n += s[1 + l];
        }
        if (n > 256 || e - s < 17 + n) return LDT_IMG_NOT_JPEG;
        memcpy(t.syms, s + 17, n);
        t.nsym = n;
        t.present = true;
        s += 17 + n;
      }
      break;
    }
    case 0xDB: {
      while (s < e) {
        const int pq = s[0] >> 4, tq = s[0] & 15;
        if (tq > 3 || pq > 1) return LDT_IMG_NOT_JPEG;
        const int need = pq ? 129 : 65;
        if (e - s < need) return LDT_IMG_NOT_JPEG;
        for (int k = 0; k < 64; ++k)
          H.q[tq][kZigzagToNatural[k]] = pq ? (uint16_t)be16(s + 1 + 2 * k) : s[1 + k];
        H.qpresent[tq] = true;
        s += need;
      }
      break;
    }
    case 0xDD:
      if (seglen != 4) return LDT_IMG_NOT_JPEG;
      H.restart = be16(s);
      break;
    case 0xE0:
      if (e - s >= 5 && memcmp(s, "JFIF\0", 5) == 0) H.jfif = true;
      break;
    case 0xEE:
      if (e - s >= 12 && memcmp(s, "Adobe", 5) == 0) {
        H.adobe = true;
        H.adobe_transform = s[11];
      }
      break;
    case 0xDA: {
      if (!sof) return LDT_IMG_NOT_JPEG;
      if (H.progressive) { // every scan is walked by plan_progressive
        H.scan_pos = i - 2;
        return LDT_IMG_OK;
      }
      if (e - s < 1) return LDT_IMG_NOT_JPEG;
      const int ns = s[0];
      if (ns < 1 || ns > 4 || e - s < 4 + 2 * ns) return LDT_IMG_NOT_JPEG;
      if (ns != H.ncomp) return LDT_IMG_UNSUPPORTED; // multi-scan sequential
      bool seen[4] = {false, false, false, false};
      for (int k = 0; k < ns; ++k) {
        int idx = -1;
        for (int c = 0; c < H.ncomp; ++c)
          if (H.cid[c] == s[1 + 2 * k]) idx = c;
        // jdmarker.c get_sos: unknown or repeated component -> JERR_BAD_COMPONENT_ID
        if (idx < 0 || seen[idx]) return LDT_IMG_NOT_JPEG;
        seen[idx] = true;
        H.td[idx] = s[2 + 2 * k] >> 4;
        H.ta[idx] = s[2 + 2 * k] & 15;
        if (H.td[idx] > 3 || H.ta[idx] > 3) return LDT_IMG_NOT_JPEG;
      }
      if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0)
        return LDT_IMG_UNSUPPORTED;
      H.scan_pos = i + seglen;
      return LDT_IMG_OK;
    }
    default:
      break;
    }
    i += seglen;
  }
}

// jdhuff.c jpeg_make_d_derived_tbl restated into the device table layout
// (canonical code assignment, then the two-level lookup of ldt_types.hpp).
bool build_huff(const RawHuff &r, bool is_dc, HuffTab &t) {
  memset(&t, 0, sizeof(t));
  int code = 0, k = 0;
  int lens[256];
  int codes[256];
  for (int l = 1; l <= 16; ++l) {
    const int cnt = r.counts[l - 1];
    if (cnt) {
      t.valoff[l] = k - code;
      for (int j = 0; j < cnt; ++j) {
        lens[k] = l;
        codes[k] = code;
        ++k;
        ++code;
      }
      t.maxcode[l] = code - 1;
    } else {
      t.maxcode[l] = -1;
    }
    if (cnt && code >= (1 << l)) return false; // all-ones code: JERR_BAD_HUFF_TABLE
    code <<= 1;
  }
  t.maxcode[17] = 0x7FFFFFFF;
  for (int j = 0; j < r.nsym; ++j) {
    t.vals[j] = r.syms[j];
    if (is_dc && r.syms[j] > 15) return false;
  }
  // level 1 (unused codes: the invalid entry)
  const uint16_t invalid = huff_entry(16, 0, is_dc);
  static thread_local uint16_t l1[1 << kLookBits];
  for (int q = 0; q < (1 << kLookBits); ++q) l1[q] = invalid;
  for (int q = 0; q < (kL2Chunks << kL2Bits); ++q) t.l2[q] = invalid;
  for (int j = 0; j < r.nsym; ++j) {
    if (lens[j] <= kLookBits) {
      const int shift = kLookBits - lens[j];
      const int base = codes[j] << shift;
      for (int q = 0; q < (1 << shift); ++q) l1[base + q] = huff_entry(lens[j], r.syms[j], is_dc);
    }
  }
  // level 2: one chunk per distinct kLookBits-bit prefix of a longer code
  int prefix_chunk[1 << kLookBits];
  for (int q = 0; q < (1 << kLookBits); ++q) prefix_chunk[q] = -1;
  int nchunks = 0;
  bool overflow = false;
  for (int j = 0; j < r.nsym; ++j) {
    if (lens[j] <= kLookBits) continue;
    const int pre = codes[j] >> (lens[j] - kLookBits);
    if (prefix_chunk[pre] < 0) {
      if (nchunks < kL2Chunks) prefix_chunk[pre] = nchunks++;
      else overflow = true;
    }
  }
  for (int j = 0; j < r.nsym && !overflow; ++j) {
    if (lens[j] <= kLookBits) continue;
    const int pre = codes[j] >> (lens[j] - kLookBits);
    const int rest = lens[j] - kLookBits; // 1..kL2Bits bits after the prefix
    const int sub = (codes[j] & ((1 << rest) - 1)) << (kL2Bits - rest);
    for (int q = 0; q < (1 << (kL2Bits - rest)); ++q)
      t.l2[(prefix_chunk[pre] << kL2Bits) + sub + q] = huff_entry(lens[j], r.syms[j], is_dc);
  }
  for (int q = 0; q < (1 << kLookBits); ++q)
    if (prefix_chunk[q] >= 0) l1[q] = overflow ? (uint16_t)kHuffCanon : (uint16_t)(prefix_chunk[q] << 5);
  if (overflow) // every long-code prefix takes the canonical search
    for (int j = 0; j < r.nsym; ++j)
      if (lens[j] > kLookBits) l1[codes[j] >> (lens[j] - kLookBits)] = (uint16_t)kHuffCanon;
  // count-mode entries (ldt_types.hpp HuffTab): runs of AC symbols whose
  // codes all lie in the kLookBits peeked bits
  const uint32_t mask = (1u << kLookBits) - 1;
  for (uint32_t x = 0; x <= mask; ++x) {
    const uint32_t e = l1[x];
    uint32_t T = e & 31;
    if (T == 0) {
      t.lc[x] = e | (e << 16); // long code: the count entry is l1's indirect entry
      continue;
    }
    uint32_t adv = e >> 9, pre = 0;
    while (!is_dc && adv < 64 && adv <= 15 && T < (uint32_t)kLookBits) {
      const uint32_t e2 = l1[(x << T) & mask];
      const uint32_t t2 = e2 & 31;
      if (t2 == 0 || T + (t2 - ((e2 >> 5) & 15)) > (uint32_t)kLookBits) break; // code past the peek
      pre = adv;
      adv += e2 >> 9;
      T += t2;
    }
    t.lc[x] = e | ((T | (pre << 5) | (adv << 9)) << 16);
  }
  return true;
}

std::string huff_key(const RawHuff &r, bool dc) {
  std::string k(1, dc ? 'D' : 'A');
  k.append(reinterpret_cast<const char *>(r.counts), 16);
  k.append(reinterpret_cast<const char *>(r.syms), r.nsym);
  return k;
}

// ---- progressive (SOF2) planning ----------------------------------------
// The end of a scan's entropy-coded data: the first j >= start (j + 1 < len)
// with cell[j] == 0xFF and cell[j + 1] not 0x00 (stuffing), 0xFF (fill) or
// RSTn; len when there is none. 16 positions per step with SSE2 (the host
// planner cost 5.8 ms per 256-image c2p batch with a byte loop, ~1.5 ms with
// memchr hopping from one stuffed 0xFF to the next).
static int64_t scan_end(const uint8_t *cell, int64_t start, int64_t len) {
  int64_t j = start;
  const __m128i ff = _mm_set1_epi8((char)0xFF), zero = _mm_setzero_si128();
  const __m128i f8 = _mm_set1_epi8((char)0xF8), d0 = _mm_set1_epi8((char)0xD0);
  for (; j + 17 <= len; j += 16) {
    const __m128i x = _mm_loadu_si128(reinterpret_cast<const __m128i *>(cell + j));
    const __m128i y = _mm_loadu_si128(reinterpret_cast<const __m128i *>(cell + j + 1));
    const __m128i keep = _mm_or_si128(_mm_or_si128(_mm_cmpeq_epi8(y, zero), _mm_cmpeq_epi8(y, ff)),
                                      _mm_cmpeq_epi8(_mm_and_si128(y, f8), d0));
    const int m = _mm_movemask_epi8(_mm_andnot_si128(keep, _mm_cmpeq_epi8(x, ff)));
    if (m) return j + __builtin_ctz((unsigned)m);
  }
  for (; j + 1 < len; ++j) {
    const int nx = cell[j + 1];
    if (cell[j] == 0xFF && nx != 0x00 && nx != 0xFF && !(nx >= 0xD0 && nx <= 0xD7)) return j;
  }
  return len;
}

// Table for k_prog: canonical codes as jdhuff.c jpeg_make_d_derived_tbl
// (same validity checks as build_huff), plus the 8-bit lookahead.
bool build_prog_tab(const RawHuff &r, bool is_dc, ProgTab &t) {
  memset(&t, 0, sizeof(t));
  int code = 0, k = 0;
  int lens[256], codes[256];
  for (int l = 1; l <= 16; ++l) {
    const int cnt = r.counts[l - 1];
    if (cnt) {
      t.valoff[l] = k - code;
      for (int j = 0; j < cnt; ++j, ++k, ++code) {
        lens[k] = l;
        codes[k] = code;
      }
      t.maxcode[l] = code - 1;
    } else {
      t.maxcode[l] = -1;
    }
    if (cnt && code >= (1 << l)) return false; // all-ones code: JERR_BAD_HUFF_TABLE
    code <<= 1;
  }
  t.maxcode[17] = 0x7FFFFFFF;
  for (int j = 0; j < r.nsym; ++j) {
    t.vals[j] = r.syms[j];
    if (is_dc && r.syms[j] > 15) return false;
    if (lens[j] <= 8) {
      const int base = codes[j] << (8 - lens[j]);
      for (int x = 0; x < (1 << (8 - lens[j])); ++x)
        t.look[base + x] = (uint16_t)((lens[j] << 8) | r.syms[j]);
    }
  }
  return true;
}



// Walks every scan of a progressive image from its first SOS (H.scan_pos):
// jdmarker.c between scans (DHT / DQT / DRI), jdphuff.c
// start_pass_phuff_decoder's progression checks, jdinput.c's quant table
// latch at a component's first scan, and the byte range of each scan's
// entropy-coded data (up to the first marker that is not RSTn). Files whose
// coefficients 0..9 are not fully refined after the last scan would take
// libjpeg's block-smoothing path (jdcoefct.c smoothing_ok): unsupported.
// Returns an LDT_IMG_* code.
int plan_progressive(const uint8_t *cell, int64_t len, const Header &H0, ProgPlan &P) {
  Header H = H0;
  int coef_bits[4][10];
  bool latched[4] = {false, false, false, false};
  for (int c = 0; c < 4; ++c)
    for (int k = 0; k < 10; ++k) coef_bits[c][k] = -1;
  int64_t i = H0.scan_pos;
  while (true) {
    if (i + 1 >= len || cell[i] != 0xFF) return LDT_IMG_CORRUPT; // data ended before EOI
    while (i + 1 < len && cell[i + 1] == 0xFF) ++i;
    if (i + 1 >= len) return LDT_IMG_CORRUPT;
    const int m = cell[i + 1];
    i += 2;
    if (m == 0xD9) break;
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
    if (i + 2 > len) return LDT_IMG_CORRUPT;
    const int seglen = be16(cell + i);
    if (seglen < 2 || i + seglen > len) return LDT_IMG_CORRUPT;
    const uint8_t *s = cell + i + 2;
    const uint8_t *e = cell + i + seglen;
    if (m == 0xC4) {
      while (s < e) {
        const int tc = s[0] >> 4, th = s[0] & 15;
        if (tc > 1 || th > 3 || e - s < 17) return LDT_IMG_NOT_JPEG;
        RawHuff &t = tc ? H.ac[th] : H.dc[th];
        int n = 0;
        for (int l = 0; l < 16; ++l) {
          t.counts[l] = s[1 + l];
          n += s[1 + l];
        }
        if (n > 256 || e - s < 17 + n) return LDT_IMG_NOT_JPEG;
        memcpy(t.syms, s + 17, n);
        t.nsym = n;
        t.present = true;
        s += 17 + n;
      }
    } else if (m == 0xDB) {
      while (s < e) {
        const int pq = s[0] >> 4, tq = s[0] & 15;
        if (tq > 3 || pq > 1) return LDT_IMG_NOT_JPEG;
        const int need = pq ? 129 : 65;
        if (e - s < need) return LDT_IMG_NOT_JPEG;
        for (int k = 0; k < 64; ++k)
          H.q[tq][kZigzagToNatural[k]] = pq ? (uint16_t)be16(s + 1 + 2 * k) : s[1 + k];
        H.qpresent[tq] = true;
        s += need;
      }
    } else if (m == 0xDD) {
      if (seglen != 4) return LDT_IMG_NOT_JPEG;
      H.restart = be16(s);
    } else if (m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
      return LDT_IMG_NOT_JPEG; // a second frame header
    } else if (m == 0xDA) {
      if (e - s < 1) return LDT_IMG_NOT_JPEG;
      const int ns = s[0];
      if (ns < 1 || ns > 4 || e - s < 4 + 2 * ns) return LDT_IMG_NOT_JPEG;
      ProgScan sc;
      memset(&sc, 0, sizeof(sc));
      sc.ns = ns;
      sc.ss = s[1 + 2 * ns];
      sc.se = s[2 + 2 * ns];
      sc.ah = s[3 + 2 * ns] >> 4;
      sc.al = s[3 + 2 * ns] & 15;
      sc.restart = H.restart;
      const bool dcband = sc.ss == 0;
      bool bad = dcband ? sc.se != 0 : (sc.ss > sc.se || sc.se > 63 || ns != 1);
      if (sc.ah != 0 && sc.al != sc.ah - 1) bad = true;
      if (sc.al > 13) bad = true;
      if (bad) return LDT_IMG_CORRUPT; // JERR_BAD_PROGRESSION
      for (int k = 0; k < 4; ++k) sc.tab[k] = -1;
      bool seen[4] = {false, false, false, false};
      for (int k = 0; k < ns; ++k) {
        int idx = -1;
        for (int c = 0; c < H.ncomp; ++c)
          if (H.cid[c] == s[1 + 2 * k]) idx = c;
        if (idx < 0 || seen[idx]) return LDT_IMG_NOT_JPEG; // JERR_BAD_COMPONENT_ID
        seen[idx] = true;
        sc.comp[k] = idx;
        const int td = s[2 + 2 * k] >> 4, ta = s[2 + 2 * k] & 15;
        if (td > 3 || ta > 3) return LDT_IMG_NOT_JPEG;
        if (!latched[idx]) {
          if (!H.qpresent[H.tq[idx]]) return LDT_IMG_NOT_JPEG;
          memcpy(P.q[idx], H.q[H.tq[idx]], sizeof(P.q[idx]));
          latched[idx] = true;
        }
        const RawHuff *t = nullptr;
        bool is_dc = false;
        if (dcband && sc.ah == 0) {
          t = &H.dc[td];
          is_dc = true;
        } else if (!dcband && k == 0) {
          t = &H.ac[ta];
        }
        if (t) {
          if (!t->present) return LDT_IMG_NOT_JPEG;
          sc.tab[k] = (int32_t)P.tabs.size();
          P.tabs.emplace_back(*t, is_dc);
        }
        for (int q = sc.ss; q <= sc.se && q < 10; ++q) coef_bits[idx][q] = sc.al;
      }
      const int64_t start = i + seglen;
      const int64_t j = scan_end(cell, start, len);
      if (j + 1 >= len) return LDT_IMG_CORRUPT; // truncated inside the scan
      if (j - start > (int64_t)INT32_MAX - 64) return LDT_IMG_UNSUPPORTED; // k_prog's offsets are int32
      sc.data_off = start;
      sc.data_len = j - start;
      P.scans.push_back(sc);
      if ((int)P.scans.size() > kMaxProgScans) return LDT_IMG_UNSUPPORTED;
      i = j;
      continue;
    }
    i += seglen;
  }
  for (int c = 0; c < H.ncomp; ++c) {
    if (!latched[c]) return LDT_IMG_NOT_JPEG;
    for (int k = 0; k < 10; ++k)
      if (coef_bits[c][k] != 0) return LDT_IMG_UNSUPPORTED; // would be block-smoothed
  }
  return LDT_IMG_OK;
}

// ---- per-batch planning --------------------------------------------------
namespace {

inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

inline int32_t destuff_chunks(const ImgDesc &d) {
  // over the scan bytes from the 4-aligned word before them
  return (int32_t)((d.src_len + 3 + kDsChunkBytes - 1) / kDsChunkBytes);
}

bool same_huff(const RawHuff &a, const RawHuff &b) {
  return a.nsym == b.nsym && memcmp(a.counts, b.counts, 16) == 0 && memcmp(a.syms, b.syms, (size_t)a.nsym) == 0;
}

// State of one plan_batch call: the plan being built and the batch's dedupe maps.
struct Planner {
  const PlanOptions &opt;
  HuffCache &cache;
  BatchPlan &B;
  std::unordered_map<std::string, int> qmap;
  std::unordered_map<int, int> hid_to_batch; // cache table id -> index in this batch
  std::unordered_map<std::string, int> ptab_map;
  // The tables of the previous image (per component): images of one dataset
  // mostly share their DQT/DHT bytes, so a byte compare against the last
  // match skips the key strings and hash lookups of the dedupe below.
  struct LastQ {
    uint16_t q[64];
    int idx = -1;
  } last_q[3];
  struct LastH {
    RawHuff r;
    int bidx = -1;
  } last_h[3][2];

  int quant_index(const uint16_t *qsrc, int k);
  int huff_index(const RawHuff &rh, bool is_dc, LastH &lh);
  int plan_image(int64_t i, const uint8_t *cell, int64_t cell_off, int64_t cell_len, ImgDesc &d,
                 const ldt_crop *crop, const ldt_window *win, int views, const int32_t *vsz, int scale);
  void plan_destuff();
};

int Planner::quant_index(const uint16_t *qsrc, int k) {
  if (last_q[k].idx >= 0 && memcmp(last_q[k].q, qsrc, 128) == 0) return last_q[k].idx;
  std::string qk(reinterpret_cast<const char *>(qsrc), 128);
  auto qi = qmap.find(qk);
  if (qi == qmap.end()) {
    qi = qmap.emplace(qk, (int)(B.qtabs.size() / 64)).first;
    B.qtabs.insert(B.qtabs.end(), qsrc, qsrc + 64);
  }
  memcpy(last_q[k].q, qsrc, 128);
  return last_q[k].idx = qi->second;
}

// Index of a baseline table in the batch (deduped across the cache's
// lifetime); -1 for a table libjpeg rejects.
int Planner::huff_index(const RawHuff &rh, bool is_dc, LastH &lh) {
  if (lh.bidx >= 0 && same_huff(lh.r, rh)) return lh.bidx;
  std::string key = huff_key(rh, is_dc);
  auto it = cache.map.find(key);
  int cid;
  if (it == cache.map.end()) {
    HuffTab t;
    if (!build_huff(rh, is_dc, t)) return -1;
    cid = (int)cache.tabs.size();
    cache.tabs.push_back(t);
    cache.map.emplace(std::move(key), cid);
  } else {
    cid = it->second;
  }
  auto bi = hid_to_batch.find(cid);
  if (bi == hid_to_batch.end()) {
    bi = hid_to_batch.emplace(cid, (int)B.htabs.size()).first;
    B.htabs.push_back(cache.tabs[(size_t)cid]);
  }
  lh.r = rh;
  return lh.bidx = bi->second;
}

// Plans row i (a non-null cell) into d (zeroed but for seg_base) and the
// batch totals. Returns an LDT_IMG_* code; on failure the caller resets d, so
// only what was added to the shared tables stays.
int Planner::plan_image(int64_t i, const uint8_t *cell, int64_t cell_off, int64_t cell_len, ImgDesc &d,
                        const ldt_crop *crop, const ldt_window *win, int views, const int32_t *vsz, int scale) {
  if (cell_len < 0) return LDT_IMG_NOT_JPEG;
  Header H;
  int status = walk_markers(cell, cell_len, H);
  if (status != LDT_IMG_OK) return status;
  if (H.width > LDT_MAX_DIM || H.height > LDT_MAX_DIM) return LDT_IMG_TOO_LARGE; // the file's own size, drafted or not
  // a drafted row (ldt_set_draft) decodes to ceil(W / scale) x ceil(H / scale)
  // (jdmaster.c jpeg_calc_output_dimensions): that is the decoded image for
  // everything below: the default box, check_crop, the limits, the taps
  const int img_w = (H.width + scale - 1) / scale, img_h = (H.height + scale - 1) / scale;
  // ... or reduced by more than kMaxReduce on an axis (the streaming resize
  // kernel's tap limit): never at the default 224 x 224, where LDT_MAX_DIM
  // reduces by exactly that; a small output size makes it the tighter bound,
  // and so does BICUBIC, whose support of 2 doubles the taps (4144 px at 224)
  // the limit is on what the resize reads: the row's box when it has one
  // a window (ldt_set_windows): the box is resized to res, so the limit is
  // that of (box -> res); the window is checked first, which also makes res a
  // divisor check_crop can take
  // several views (ldt_set_views): crop and win point at the row's `views`
  // entries, checked in order; the first bad view gives the row its status
  // per-view sizes (ldt_set_view_sizes): view v against its own (h_v, w_v)
  for (int v = 0; v < views; ++v) {
    const int oh = vsz ? vsz[2 * v] : opt.out_h, ow = vsz ? vsz[2 * v + 1] : opt.out_w;
    const ldt_crop box = crop ? crop[v] : ldt_crop{0, 0, img_h, img_w, 0};
    const ldt_window wnd = win ? win[v] : ldt_window{oh, ow, 0, 0};
    if (win && (status = check_window(wnd, oh, ow)) != LDT_IMG_OK) return status;
    if ((status = check_crop(box, img_w, img_h, wnd.res_h, wnd.res_w, opt.filter)) != LDT_IMG_OK) return status;
  }
  int hmax = 1, vmax = 1;
  for (int k = 0; k < H.ncomp; ++k) {
    if (!H.progressive && (!H.qpresent[H.tq[k]] || !H.dc[H.td[k]].present || !H.ac[H.ta[k]].present))
      return LDT_IMG_NOT_JPEG;
    hmax = H.h[k] > hmax ? H.h[k] : hmax;
    vmax = H.v[k] > vmax ? H.v[k] : vmax;
  }
  if (H.ncomp == 3) {
    // supported sampling: luma at full size, every factor (1..4) divides the
    // max, at most 10 blocks per MCU; chroma_at upsamples any such ratio
    int bpm = 0;
    if (H.h[0] != hmax || H.v[0] != vmax) return LDT_IMG_UNSUPPORTED; // subsampled luma
    for (int k = 0; k < 3; ++k) {
      if (hmax % H.h[k] || vmax % H.v[k]) return LDT_IMG_UNSUPPORTED;
      bpm += H.h[k] * H.v[k];
    }
    if (bpm > kMaxBlocksPerMcu) return LDT_IMG_UNSUPPORTED;
  }
  d.width = img_w;
  d.height = img_h;
  d.ncomp = H.ncomp;
  d.draft = (uint8_t)scale;
  d.file_w = (uint16_t)H.width;
  d.file_h = (uint16_t)H.height;
  if (H.ncomp == 1) {
    d.color = 2;
    d.mcux = (H.width + 7) / 8;
    d.mcuy = (H.height + 7) / 8;
    d.bpm = 1;
    d.bcomp[0] = 0;
    d.ch[0] = d.cv[0] = 1;
    d.hf[0] = d.vf[0] = 1;
  } else {
    // jdapimin.c default_decompress_parms: JFIF -> YCbCr; Adobe transform 0 -> RGB;
    // otherwise component ids 'R','G','B' -> RGB; else YCbCr.
    bool rgb;
    if (H.jfif) rgb = false;
    else if (H.adobe) rgb = (H.adobe_transform == 0);
    else rgb = (H.cid[0] == 82 && H.cid[1] == 71 && H.cid[2] == 66);
    d.color = rgb ? 1 : 0;
    d.mcux = (H.width + 8 * hmax - 1) / (8 * hmax);
    d.mcuy = (H.height + 8 * vmax - 1) / (8 * vmax);
    int b = 0;
    for (int k = 0; k < 3; ++k) {
      d.ch[k] = H.h[k];
      d.cv[k] = H.v[k];
      d.hf[k] = hmax / H.h[k];
      d.vf[k] = vmax / H.v[k];
      for (int yy = 0; yy < H.v[k]; ++yy)
        for (int xx = 0; xx < H.h[k]; ++xx) {
          d.bcomp[b] = (uint8_t)k;
          d.bdx[b] = (uint8_t)xx;
          d.bdy[b] = (uint8_t)yy;
          ++b;
        }
    }
    d.bpm = b;
  }
  ProgPlan PP;
  if (H.progressive && (status = plan_progressive(cell, cell_len, H, PP)) != LDT_IMG_OK) return status;
  int64_t pl = B.plane_total;
  // libjpeg under scaling (jdmaster.c jpeg_calc_output_dimensions, jdinput.c,
  // jdsample.c): luma's DCT_scaled_size is min_s = 8 / scale; a component's
  // starts there and doubles while it stays below 8 and the component's
  // upsampling factor stays whole, so subsampled chroma takes a larger IDCT
  // instead of being upsampled (4:2:0 never upsamples under a draft); at
  // min_s == 1 fancy upsampling is off. A grey file is one component at full
  // sampling whatever its SOF says.
  const int min_s = 8 / scale;
  const int gh = H.ncomp == 1 ? 1 : hmax, gv = H.ncomp == 1 ? 1 : vmax;
  d.nofancy = scale > 1 && min_s == 1;
  for (int k = 0; k < H.ncomp; ++k) {
    const int bw = d.mcux * d.ch[k], bh = d.mcuy * d.cv[k];
    int sc = min_s;
    while (sc < 8 && (gh * min_s) % (d.ch[k] * sc * 2) == 0 && (gv * min_s) % (d.cv[k] * sc * 2) == 0) sc *= 2;
    d.sc[k] = (uint8_t)sc;
    // scale 1: sc == 8, the stride bw * 8 and the factors hmax / h, vmax / v
    // as ever. A drafted plane is bw * sc wide; its stride is rounded up
    // (kPlaneStrideAlign) and the padding is never written or selected
    d.plane_stride[k] = (int32_t)align_up((int64_t)bw * sc, kPlaneStrideAlign);
    d.plane_off[k] = pl;
    pl += align_up((int64_t)d.plane_stride[k] * bh * sc, 256);
    d.hf[k] = gh * min_s / (d.ch[k] * sc);
    d.vf[k] = gv * min_s / (d.cv[k] * sc);
    d.cdw[k] = (int)(((int64_t)H.width * d.ch[k] * sc + gh * 8 - 1) / (gh * 8));
    d.cdh[k] = (int)(((int64_t)H.height * d.cv[k] * sc + gv * 8 - 1) / (gv * 8));
    // quant table (progressive: latched at the component's first scan)
    d.qt[k] = quant_index(H.progressive ? PP.q[k] : H.q[H.tq[k]], k);
    // Huffman tables; after a bad one the other components' tables still
    // join the batch, so the indices later rows get do not depend on it
    if (H.progressive) continue;
    if ((d.dct[k] = huff_index(H.dc[H.td[k]], true, last_h[k][0])) < 0 ||
        (d.act[k] = huff_index(H.ac[H.ta[k]], false, last_h[k][1])) < 0)
      status = LDT_IMG_NOT_JPEG;
  }
  if (status != LDT_IMG_OK) return status;
  B.plane_total = pl;
  const int64_t nmcu = (int64_t)d.mcux * d.mcuy;
  if (H.progressive) {
    // k_prog decodes it: no baseline segments, destuff chunks or decoder
    // workgroups; its scans join the batch's scan table
    d.dst_off = B.dst_total;
    d.prog_first = (int32_t)B.pscans.size();
    d.prog_count = (int32_t)PP.scans.size();
    for (ProgScan sc : PP.scans) {
      sc.data_off += cell_off;
      for (int k = 0; k < 4; ++k) {
        if (sc.tab[k] < 0) continue;
        const auto &rt = PP.tabs[(size_t)sc.tab[k]];
        std::string key = huff_key(rt.first, rt.second);
        auto it = ptab_map.find(key);
        if (it == ptab_map.end()) {
          ProgTab t;
          if (!build_prog_tab(rt.first, rt.second, t)) {
            status = LDT_IMG_NOT_JPEG; // the other scans' tables still join the batch
            break;
          }
          it = ptab_map.emplace(std::move(key), (int)B.ptabs.size()).first;
          B.ptabs.push_back(t);
        }
        sc.tab[k] = it->second;
      }
      B.pscans.push_back(sc);
    }
    if (status != LDT_IMG_OK) {
      B.pscans.resize((size_t)d.prog_first);
      return status;
    }
    B.prog_img.push_back((int32_t)i);
  } else {
    // distinct tables over the image's (component, DC/AC) contexts
    int ids[6], nd = 0;
    for (int x = 0; x < 6; ++x) {
      const int cc = (x >> 1) < d.ncomp ? (x >> 1) : 0;
      const int tix = (x & 1) ? d.act[cc] : d.dct[cc];
      bool seen = false;
      for (int q = 0; q < nd; ++q) seen = seen || ids[q] == tix;
      if (!seen) ids[nd++] = tix;
    }
    if (nd > B.max_tabs) B.max_tabs = nd;
    d.restart = H.restart;
    d.nseg = H.restart ? (int32_t)((nmcu + H.restart - 1) / H.restart) : 1;
    for (int sidx = 0; sidx < d.nseg; ++sidx) {
      Segment sg;
      memset(&sg, 0, sizeof(sg));
      sg.img = (int32_t)i;
      sg.mcu_first = H.restart ? sidx * H.restart : 0;
      sg.mcu_count = H.restart ? (int32_t)std::min<int64_t>(H.restart, nmcu - sg.mcu_first) : (int32_t)nmcu;
      B.segs.push_back(sg);
    }
    d.src_off = cell_off + H.scan_pos;
    d.src_len = cell_len - H.scan_pos;
    // k_huff_image: all of the image's slots in one workgroup. Slots are
    // sum over segments of ceil(bits_s / S) <= bits / S + nseg, so
    // S >= bits / (kHuffThreads - nseg) fits; the option is a lower bound.
    const int64_t room = std::max<int64_t>(kHuffThreads - (int64_t)d.nseg, 1);
    const int64_t min_s = (d.src_len * 8 + room - 1) / room;
    if (opt.parallel && d.nseg <= kMaxParSegs && min_s <= kMaxParS - 64) {
      int64_t sbits = std::max<int64_t>(min_s, std::max(opt.subseq_bits, 64));
      sbits = (sbits + 31) & ~(int64_t)31;
      // an odd number of 32-bit words per range: lanes' LDS window reads start
      // in distinct banks
      if (((sbits >> 5) & 1) == 0) sbits += 32;
      d.sub_bits = (int32_t)sbits;
      B.par_img.push_back((int32_t)i);
      B.max_window = std::max<int64_t>(B.max_window, destuff_region_bytes(d.src_len, d.nseg) + 16);
    } else {
      d.sub_bits = 0;
      ++B.n_serial;
    }
    d.dst_off = B.dst_total;
    B.dst_total += destuff_region_bytes(d.src_len, d.nseg);
  }
  // each image's coefficients: room for 8 packed units per block (baseline),
  // and for progressive images also eight dense group planes of npad blocks
  // (coef_piece) in the progressive buffer (ldt_kernels.hpp)
  d.coef_off = B.coef_blocks;
  const int64_t nblk = nmcu * d.bpm;
  const int64_t npad = (nblk + kCoefAlign - 1) & ~(int64_t)(kCoefAlign - 1);
  B.coef_blocks += npad;
  d.pcoef_off = B.pcoef_blocks;
  if (H.progressive) B.pcoef_blocks += npad;
  if (nblk > B.max_blocks) B.max_blocks = nblk;
  if (resize_fast420(d)) ++B.n_fast420;
  if (scale > 1) ++B.n_draft;
  // the descriptor carries view 0 (the only one without ldt_set_views); the
  // batch's staged row and taps cover every view of the row
  const int64_t n = (int64_t)B.descs.size();
  for (int v = 0; v < views; ++v) {
    const int oh = vsz ? vsz[2 * v] : opt.out_h, ow = vsz ? vsz[2 * v + 1] : opt.out_w;
    const ldt_crop box = crop ? crop[v] : ldt_crop{0, 0, img_h, img_w, 0};
    const ldt_window wnd = win ? win[v] : ldt_window{oh, ow, 0, 0};
    if (v == 0) {
      d.box_top = box.top;
      d.box_left = box.left;
      d.box_h = box.height;
      d.box_w = box.width;
      d.flip = box.flip;
      d.res_h = wnd.res_h;
      d.res_w = wnd.res_w;
      d.win_top = wnd.top;
      d.win_left = wnd.left;
    }
    if (!B.views.empty())
      B.views[(size_t)(v * n + i)] = ViewDesc{box.top,   box.left,  box.height, box.width, box.flip,
                                             wnd.res_h, wnd.res_w, wnd.top,    wnd.left,  {vsz ? oh : 0, vsz ? ow : 0, 0}};
    if (box.width > B.max_w) B.max_w = box.width;
    if (box.height > B.max_h) B.max_h = box.height;
    // the taps are those of (box -> res): out without windows
    const int kh = resample_ksize_host(box.width, wnd.res_w, opt.filter),
              kv = resample_ksize_host(box.height, wnd.res_h, opt.filter);
    if (kh > B.max_ks_h) B.max_ks_h = kh;
    if (kv > B.max_ks_v) B.max_ks_v = kv;
  }
  return LDT_IMG_OK;
}

// The LDS window, then the destuff chunks. Fused destuff: a k_huff_image
// workgroup whose image's destuffed stream fits the window destuffs the scan
// bytes itself (ldt_huffman.hip destuff_into_window); those images get no
// destuff chunks (ds_count 0).
void Planner::plan_destuff() {
  int64_t cap = kHuffLdsMax - kHuffStaticLds - huff_tab_lds_image(B.max_tabs);
  if (opt.win_cap >= 0) cap = std::min<int64_t>(cap, opt.win_cap);
  B.win_bytes = (int)(std::min<int64_t>(B.max_window, cap) & ~(int64_t)15);
  for (size_t i = 0; i < B.descs.size(); ++i) {
    ImgDesc &d = B.descs[i];
    d.ds_first = B.n_chunks;
    if (d.nseg == 0) continue; // failed or progressive: ds_count 0
    const bool fused = opt.fuse_destuff && d.sub_bits > 0 &&
                       destuff_region_bytes(d.src_len, d.nseg) + 16 <= B.win_bytes;
    if (fused) continue;
    d.ds_count = destuff_chunks(d);
    B.chunk_img.insert(B.chunk_img.end(), (size_t)d.ds_count, (int32_t)i);
    B.n_chunks += d.ds_count;
    ++B.n_ds_img;
  }
}

} // namespace

int check_crop(const ldt_crop &c, int width, int height, int out_h, int out_w, int filter) {
  // top + height and left + width are never formed: a hostile box cannot overflow
  if (c.top < 0 || c.left < 0 || c.height < 1 || c.width < 1 || c.top > height || c.left > width ||
      c.height > height - c.top || c.width > width - c.left || (c.flip != 0 && c.flip != 1))
    return LDT_IMG_BAD_CROP;
  // the box is inside the image here: support * size cannot overflow
  if (resample_reduce(c.width, out_w, filter) > kMaxReduce || resample_reduce(c.height, out_h, filter) > kMaxReduce)
    return LDT_IMG_TOO_LARGE;
  return LDT_IMG_OK;
}

int check_window(const ldt_window &w, int out_h, int out_w) {
  // top + out_h and left + out_w are never formed: res - top cannot overflow
  // once res is in 1..LDT_MAX_RES and top is not negative
  if (w.res_h < 1 || w.res_h > LDT_MAX_RES || w.res_w < 1 || w.res_w > LDT_MAX_RES || w.top < 0 || w.left < 0 ||
      w.top > w.res_h || w.left > w.res_w || out_h > w.res_h - w.top || out_w > w.res_w - w.left)
    return LDT_IMG_BAD_WINDOW;
  return LDT_IMG_OK;
}

template <typename OffT>
void plan_batch(const uint8_t *data, const OffT *offsets, int64_t arr_offset, int64_t n,
                const uint8_t *validity, const PlanOptions &opt, HuffCache &cache, BatchPlan &B,
                const ldt_crop *crops, const ldt_window *windows, int views, const int32_t *view_sizes,
                const int32_t *drafts) {
  B = BatchPlan();
  if (views < 1) views = 1;
  B.n_views = views;
  if (view_sizes && !view_geom_build(n, views, view_sizes, kMaxOut, B.geom)) {
    // refused sizes: no table of n * views entries is formed, every row fails
    B.geom_bad = true;
    B.n_views = views = 1;
    view_sizes = nullptr;
  }
  if (views > 1 || view_sizes) B.views.resize((size_t)n * (size_t)views); // all zero
  B.descs.resize((size_t)n);
  B.status.assign((size_t)n, LDT_IMG_OK);
  Planner P{opt, cache, B};
  const int64_t base = (int64_t)offsets[arr_offset];
  for (int64_t i = 0; i < n; ++i) {
    ImgDesc &d = B.descs[(size_t)i]; // all zero
    d.seg_base = (int32_t)B.segs.size();
    const int64_t r = arr_offset + i;
    const int64_t cell_off = (int64_t)offsets[r] - base;
    int status = LDT_IMG_NULL;
    if (B.geom_bad)
      status = LDT_IMG_BAD_WINDOW;
    else if (!validity || ((validity[r >> 3] >> (r & 7)) & 1))
      status = P.plan_image(i, data + base + cell_off, cell_off, (int64_t)offsets[r + 1] - (int64_t)offsets[r], d,
                            crops ? crops + i * views : nullptr, windows ? windows + i * views : nullptr, views,
                            view_sizes, drafts ? (int)drafts[i] : 1);
    if (status != LDT_IMG_OK) {
      // a failed row: a 1x1 image with nothing to decode
      const int32_t seg_base = d.seg_base;
      memset(&d, 0, sizeof(d));
      d.seg_base = seg_base;
      d.width = d.height = 1;
      d.box_h = d.box_w = 1;
      d.res_h = opt.out_h;
      d.res_w = opt.out_w;
      if (view_sizes) {
        d.res_h = view_sizes[0];
        d.res_w = view_sizes[1];
      }
      for (int v = 0; !B.views.empty() && v < views; ++v) {
        const int oh = view_sizes ? view_sizes[2 * v] : opt.out_h, ow = view_sizes ? view_sizes[2 * v + 1] : opt.out_w;
        B.views[(size_t)(v * n + i)] = ViewDesc{0, 0, 1, 1, 0, oh, ow, 0, 0, {view_sizes ? oh : 0, view_sizes ? ow : 0, 0}};
      }
      B.status[(size_t)i] = status;
      B.any_bad = true;
    }
  }
  P.plan_destuff();
}

template void plan_batch<int32_t>(const uint8_t *, const int32_t *, int64_t, int64_t, const uint8_t *,
                                  const PlanOptions &, HuffCache &, BatchPlan &, const ldt_crop *,
                                  const ldt_window *, int, const int32_t *, const int32_t *);
template void plan_batch<int64_t>(const uint8_t *, const int64_t *, int64_t, int64_t, const uint8_t *,
                                  const PlanOptions &, HuffCache &, BatchPlan &, const ldt_crop *,
                                  const ldt_window *, int, const int32_t *, const int32_t *);

namespace {
template <typename OffT>
void image_sizes(const uint8_t *data, const OffT *offsets, int64_t arr_offset, int64_t n, const uint8_t *validity,
                 int32_t *wh, int32_t *status) {
  for (int64_t i = 0; i < n; ++i) {
    const int64_t r = arr_offset + i;
    const int64_t len = (int64_t)offsets[r + 1] - (int64_t)offsets[r];
    int st = LDT_IMG_NULL;
    Header H;
    if (!validity || ((validity[r >> 3] >> (r & 7)) & 1))
      st = len < 0 ? LDT_IMG_NOT_JPEG : walk_markers(data + (int64_t)offsets[r], len, H);
    status[i] = st;
    wh[2 * i] = st == LDT_IMG_OK ? H.width : 0;
    wh[2 * i + 1] = st == LDT_IMG_OK ? H.height : 0;
  }
}
} // namespace

// ---- plan blob -----------------------------------------------------------
PlanLayout plan_layout(const BatchPlan &B, bool has_labels) {
  const int64_t n = (int64_t)B.descs.size();
  PlanLayout L;
  int64_t off = 0;
  auto section = [&off](int64_t bytes) {
    const int64_t at = off;
    off = align_up(off + bytes, 64);
    return at;
  };
  L.off_desc = section((int64_t)sizeof(ImgDesc) * n);
  L.off_seg = section((int64_t)sizeof(Segment) * (int64_t)B.segs.size());
  L.off_huff = section((int64_t)sizeof(HuffTab) * (int64_t)B.htabs.size());
  L.off_quant = section(2 * (int64_t)B.qtabs.size());
  L.off_lut = section(3 * 256 * 4);
  L.off_labels = section(has_labels ? 8 * n : 0);
  L.off_status = section(4 * n);
  L.off_par = section(4 * (int64_t)B.par_img.size());
  L.off_chunk = section(4 * (int64_t)B.chunk_img.size());
  L.off_redo = section(64);
  L.off_pscan = section((int64_t)sizeof(ProgScan) * (int64_t)B.pscans.size());
  L.off_ptab = section((int64_t)sizeof(ProgTab) * (int64_t)B.ptabs.size());
  L.off_pimg = section(4 * (int64_t)B.prog_img.size());
  L.off_view = section((int64_t)sizeof(ViewDesc) * (int64_t)B.views.size());
  L.plan_bytes = off;
  return L;
}

void build_lut(const ldt_norm *norm, float *lut) {
  // torchvision to_tensor: float32(v) / 255 (IEEE single), then Normalize:
  // (x - mean) / std in float32 (tensor.sub_(mean).div_(std)).
  for (int c = 0; c < 3; ++c)
    for (int v = 0; v < 256; ++v) {
      volatile float x = (float)v / 255.0f;
      if (norm) {
        volatile float t = x - norm->mean[c];
        x = t / norm->std[c];
      }
      lut[c * 256 + v] = x;
    }
}

uint16_t f32_to_f16_bits(float f) {
  uint32_t x;
  memcpy(&x, &f, 4);
  const uint32_t sign = (x >> 16) & 0x8000u;
  x &= 0x7FFFFFFFu;
  if (x > 0x7F800000u) return (uint16_t)(sign | 0x7E00u); // NaN
  // 65520 = the tie between the largest finite value 65504 (odd mantissa) and 2^16: inf from there on
  if (x >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);
  if (x < 0x38800000u) {
    // below 2^-14: a subnormal result, in units of 2^-24
    const int shift = 126 - (int)(x >> 23);
    if (shift > 24) return (uint16_t)sign; // below 2^-25: zero (the tie at 2^-25 goes to the even 0 below)
    const uint32_t mant = (x & 0x7FFFFFu) | 0x800000u;
    uint32_t r = mant >> shift;
    const uint32_t rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (r & 1u))) ++r; // 0x400 is the smallest normal: the carry is right
    return (uint16_t)(sign | r);
  }
  const uint32_t r = x - 0x38000000u; // exponent rebiased 127 -> 15; a mantissa carry moves into it
  return (uint16_t)(sign | ((r + 0xFFFu + ((r >> 13) & 1u)) >> 13));
}

uint16_t f32_to_bf16_bits(float f) {
  uint32_t x;
  memcpy(&x, &f, 4);
  if ((x & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC0u; // NaN, as c10::BFloat16 gives it
  return (uint16_t)((x + 0x7FFFu + ((x >> 16) & 1u)) >> 16);
}

void build_lut16(const ldt_norm *norm, int dtype, uint16_t *lut) {
  float f[768];
  build_lut(norm, f);
  for (int i = 0; i < 768; ++i) lut[i] = dtype == kDtypeBF16 ? f32_to_bf16_bits(f[i]) : f32_to_f16_bits(f[i]);
}

void write_plan(const BatchPlan &B, const PlanLayout &L, const ldt_norm *norm, const int64_t *labels,
                uint8_t *dst, int dtype) {
  auto put = [dst](int64_t off, const auto &v) {
    if (!v.empty()) memcpy(dst + off, v.data(), sizeof(v[0]) * v.size());
  };
  put(L.off_desc, B.descs);
  put(L.off_seg, B.segs);
  put(L.off_huff, B.htabs);
  put(L.off_quant, B.qtabs);
  if (dtype == kDtypeF16 || dtype == kDtypeBF16) {
    build_lut16(norm, dtype, reinterpret_cast<uint16_t *>(dst + L.off_lut));
    memset(dst + L.off_lut + 768 * 2, 0, 768 * 2);
  } else {
    build_lut(norm, reinterpret_cast<float *>(dst + L.off_lut));
  }
  if (labels) memcpy(dst + L.off_labels, labels, 8 * B.descs.size());
  put(L.off_status, B.status);
  put(L.off_par, B.par_img);
  put(L.off_chunk, B.chunk_img);
  memset(dst + L.off_redo, 0, 64);
  put(L.off_pscan, B.pscans);
  put(L.off_ptab, B.ptabs);
  put(L.off_pimg, B.prog_img);
  put(L.off_view, B.views);
}

} // namespace ldt

// The sizes plan_batch's marker walk reads, for callers that sample crop boxes
// before the decode (include/ldt.h). Host memory only.
extern "C" int ldt_image_sizes(const uint8_t *data, const void *offsets, int offsets64, int64_t arr_offset, int64_t n,
                               const uint8_t *validity, int32_t *wh, int32_t *status) {
  if (n < 0 || arr_offset < 0 || (n > 0 && (!data || !offsets || !wh || !status))) return LDT_ERR_ARG;
  if (offsets64)
    ldt::image_sizes(data, static_cast<const int64_t *>(offsets), arr_offset, n, validity, wh, status);
  else
    ldt::image_sizes(data, static_cast<const int32_t *>(offsets), arr_offset, n, validity, wh, status);
  return LDT_OK;
}
