// ldt_sync_cache.hpp — the converged slot states of k_huff_image, kept per
// image on the device (HIP-free: layout, index and validation only).
//
// Phase 1 and the rounds of the parallel Huffman decoder compute a function
// of the compressed bytes alone: per slot the exit (ex_p, ex_bk) and the
// blocks started (nblk). The write pass reads nothing else. The table keeps
// those triples, keyed by a fingerprint of the scan bytes, so that a later
// decode of the same cell goes from setup to the write pass. Nothing here is
// trusted: a hinted write pass proves its hints or the image is redone
// (ldt_huffman.hip, image_decode). This header only keeps a
// hint from moving an access outside what the full path can touch.
//
// One allocation per device:
//   [stats: kScStats int64][headers: sets x kScWays x 16 B][payloads]
// A set's kScWays headers share one 64-byte line. Entry e = set * kScWays +
// way owns payload e: kScSlots x 8 B. There is no eviction: a full set
// refuses the insert.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LDT_SC_HD __host__ __device__ inline
#else
#define LDT_SC_HD inline
#endif

namespace ldt {

constexpr int kScWays = 4;
constexpr int kScSlots = 1024; // slots per payload (kHuffThreads)
constexpr int kScStats = 8;    // hits, misses, inserts, refused, rejected, fallbacks, 2 spare
constexpr uint32_t kScEmpty = 0, kScWriting = 1, kScReady = 2;

// key, then meta = geometry word | (state | blocks << 2) << 32: two 8-byte
// words, each read and written whole.
struct ScHeader {
  uint64_t key;
  uint64_t meta;
};
// One slot's triple: ex_p, then ex_bk | nblk << 16.
struct ScSlot {
  int32_t ex_p;
  uint32_t bk_n;
};
static_assert(sizeof(ScHeader) == 16 && sizeof(ScSlot) == 8, "table layout");
constexpr int64_t kScPayloadBytes = (int64_t)kScSlots * (int64_t)sizeof(ScSlot);
constexpr int64_t kScSetBytes = kScWays * kScPayloadBytes; // the budget counts payloads
constexpr int64_t kScMaxSets = (int64_t)1 << 24;

// Sets a budget of `bytes` buys (0: too small for one set; no table).
LDT_SC_HD int64_t sc_sets(int64_t bytes) {
  if (bytes < kScSetBytes) return 0;
  const int64_t s = bytes / kScSetBytes;
  return s > kScMaxSets ? kScMaxSets : s;
}
LDT_SC_HD int64_t sc_entries(int64_t sets) { return sets * kScWays; }
LDT_SC_HD int64_t sc_off_headers() { return (int64_t)kScStats * 8; }
LDT_SC_HD int64_t sc_off_payloads(int64_t sets) { return sc_off_headers() + sets * kScWays * (int64_t)sizeof(ScHeader); }
LDT_SC_HD int64_t sc_table_bytes(int64_t sets) { return sc_off_payloads(sets) + sets * kScSetBytes; }

// Geometry word: S / 32 (S <= 32768, a multiple of 32), slots - 1, nseg - 1.
LDT_SC_HD uint32_t sc_geom(int sub_bits, int slots, int nseg) {
  return (uint32_t)(sub_bits >> 5) | ((uint32_t)(slots - 1) << 12) | ((uint32_t)(nseg - 1) << 22);
}
LDT_SC_HD uint64_t sc_meta(uint32_t geom, uint32_t state, int64_t blocks) {
  return (uint64_t)geom | ((uint64_t)(state | ((uint32_t)blocks << 2)) << 32);
}
LDT_SC_HD uint32_t sc_meta_state(uint64_t meta) { return (uint32_t)(meta >> 32) & 3u; }
// Images of more blocks do not use the table (8192 x 8192 4:4:4 has 3 << 20).
constexpr int64_t kScMaxBlocks = ((int64_t)1 << 30) - 1;

// The key: the scan bytes' fingerprint with the cell length and the geometry
// folded in (splitmix64 finaliser).
LDT_SC_HD uint64_t sc_key(uint64_t fp, int64_t src_len, uint32_t geom) {
  uint64_t z = fp ^ ((uint64_t)src_len * 0x9E3779B97F4A7C15ull) ^ ((uint64_t)geom << 32 | geom);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
LDT_SC_HD int64_t sc_set_index(uint64_t key, int64_t sets) {
  return (int64_t)(((key >> 32) * (uint64_t)sets) >> 32); // < sets (sets <= 2^24)
}

// One slot's hint against the image's geometry: slot j of a segment of
// sub_count slots and seg_bits bits, S bits per slot, b3end = 3 * blocks per
// MCU. A converged exit is the first count-step boundary at or after the
// range end min((j + 1) S, seg_bits), and a step consumes at most 31 bits;
// its state is a block of the MCU (b3 a multiple of 3 below b3end) and a
// coefficient index <= 63. The last slot's exit position is never used (its
// write pass ends at the segment's end), so any value passes there.
LDT_SC_HD bool hints_plausible(int32_t ex_p, uint32_t ex_bk, int j, int sub_count, int S, int32_t seg_bits,
                               int b3end) {
  if (j < 0 || j >= sub_count || S <= 0 || seg_bits < 0) return false;
  const uint32_t b3 = ex_bk >> 8, k = ex_bk & 255u;
  if (b3 >= (uint32_t)b3end || b3 % 3u != 0u || k > 63u) return false;
  if (j == sub_count - 1) return true;
  const int64_t end = (int64_t)(j + 1) * S;
  const int64_t stop = end < seg_bits ? end : seg_bits;
  return ex_p >= stop && ex_p <= stop + 31;
}

// A segment's hinted block counts, summed over all its slots but the last,
// must not exceed its blocks (mcu_count * bpm): then every slot's first block
// lies inside the segment and its limit is not negative, as on the full path.
// (The last slot's count is read by nothing: its first block is the sum
// before it. It is also no function of the block count alone: the count
// steps run to the segment's end and take its pad bits for one more block.)
LDT_SC_HD bool hints_sum_ok(int64_t sum_before_last, int64_t mcu_count, int bpm) {
  return sum_before_last >= 0 && sum_before_last <= mcu_count * bpm;
}

} // namespace ldt
