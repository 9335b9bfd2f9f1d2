// ldt_kernels.hpp — host-callable launchers for the gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ldt.h"
#include "ldt_types.hpp"

namespace ldt {

struct RawSrc {
  const uint8_t *base;
  int64_t cell_stride;
  int h, w;
};

// The output size of a resize launch and the cached coefficient tables for it
// (ldt_types.hpp kResamp*): tab_h holds rows of out_w entries for input widths
// up to max_in_h, tab_v rows of out_h entries for input heights up to
// max_in_v. At 224 x 224 both are the context's kOut table.
struct ResizeOut {
  int oh = kOut, ow = kOut;
  const int32_t *tab_h = nullptr, *tab_v = nullptr;
  int max_in_h = 0, max_in_v = 0;
  // the most taps any width / height of the batch really has (resample_taps_host,
  // kept per table entry; a height without an entry counts Pillow's capacity,
  // resample_ksize_host): k_resize4's KS, ring and rows are sized by these. 0: not known
  int taps_h = 0, taps_v = 0;
  bool generic = false; // the generic-width band kernel even at kOut x kOut (LDT_OPT_RESIZE_IMPL 3)
  // the call's output format (ldt_set_output_format). The default takes the
  // float32 CHW kernels; any other their FMT instantiations, whose table
  // (DevPlan::lut, the raw launchers' lut) is the form write_plan emits for
  // fmt.dtype and whose `out` is the base of n * 3 * oh * ow such elements
  OutFmt fmt;
};

// The device's table of converged slot states (ldt_sync_cache.hpp) as
// k_huff_image sees it. sets 0: off (no lookups, no inserts).
struct ScView {
  uint8_t *base = nullptr;
  int32_t sets = 0;
  int32_t stats = 0; // 1: count into the table's statistics (LDT_OPT_SYNC_CACHE 2)
};

struct DevPlan {
  ScView sc;
  const ImgDesc *descs;
  Segment *segs;
  const HuffTab *htabs;
  const uint16_t *qtabs;
  const float *lut;
  ResizeOut ro;          // output size and the context's cached resample coefficient tables for it
  const int64_t *labels; // may be null
  int n, nseg;
  int max_ks_h, max_ks_v, max_w, max_h;
  int64_t max_blocks;
  // Huffman decode: k_huff_image (one workgroup per image) and k_huff_serial
  int n_par;              // images on the parallel decoder
  const int32_t *par_img; // its workgroup -> image
  int n_serial;           // images on the serial decoder (sub_bits == 0)
  int win_bytes;          // LDS window of k_huff_image (images needing more read global memory)
  int warm_pct;           // phase-1 warm-up before each range, % of S
  int resize_waves_pct;   // k_resize4 band count, % of one full wave of resize waves
  int resize_wpg;         // k_resize4 waves per workgroup for JPEG sources (0: default 2)
  int resize420;          // 4:2:0 images <= 512 px: 3 k_resize4<5> (packed 16-bit staging), 0 k_resize4<0>
  int32_t *redo;          // debug counters of the parallel decoder (16 ints)
  int max_tabs;           // max distinct Huffman tables of one image (LDS slots)
  int n_fast420;         // images on k_resize4's fast staging path (resize_fast420)
  int n_draft = 0;       // good rows drafted to 1/2, 1/4 or 1/8 (ldt_set_draft): not 0 -> k_idct_scaled, not k_idct
  // progressive images (k_prog, one workgroup each)
  int n_prog;
  const int32_t *prog_img; // -> image index
  const ProgScan *pscans;
  const ProgTab *ptabs;
  // destuff chunks (4 KB of entropy-coded bytes each)
  int n_chunks;
  int n_ds_img;           // baseline images destuffed by k_destuff_* (the others: k_huff_image)
  const int32_t *chunk_img; // chunk -> image
  // a call with several views per image (ldt_set_views): the view table, one
  // entry per output image v * n + i; null and 1 otherwise
  const ViewDesc *views = nullptr;
  int n_views = 1;
  // a call with per-view output sizes (ldt_set_view_sizes): the plan's geometry
  // table, in host memory (the launches pass it by value); null otherwise.
  // `views` is then set for n_views = 1 too, and ro.oh / ro.ow are not read.
  const struct ViewGeomTab *geom = nullptr;
};

// Coefficients of baseline images (the Huffman decoders' output), packed:
// a block's nonzero 16-byte groups (zigzag slots 8g..8g+7, slot 0 unused) in
// increasing g, one 16-byte unit each, in the image's region of `coef`
// (starting at coef_off * 64 int16s, room for 8 units per block). A run (the
// blocks one decoder lane owns, consecutive) writes its blocks' units
// contiguously from unit 8 * (its first block), so its first unit is
// 64-byte aligned and it writes whole 64-byte segments. Per block a 4-byte
// record brec[coef_off + ib] = nonzero-group mask (bits 0-7) | run start
// (bit 8) | DC (bits 16-31: the difference from the decoder, the absolute
// value after the predictor scan), and per 64 blocks a carry
// bcarry[coef_off / 64 + c] = the first unit of block 64c. A block's first
// unit is then 8 * ib at a run start, else its predecessor's first unit plus
// the predecessor's group count: k_idct, whose waves own 64 consecutive
// blocks, gets it with one segmented wave scan from the chunk's carry.
// Nothing is read that was not written in the same batch, so the buffer needs
// no clearing.
//
// Progressive images (k_prog) refine coefficients over many scans, so they
// keep dense per-image group planes in `pcoef`: zigzag slots 8g..8g+7 of block
// ib at piece g * npad + ib of the region at pcoef_off * 64 int16s (npad = the
// block count rounded up to 64), so the 64 lanes of a wave owning 64
// consecutive blocks read group g with one contiguous 1 KB access. That buffer
// is all zero between batches (k_idct clears the groups it read).
__host__ __device__ __forceinline__ int coef_npad(const ImgDesc &d) {
  return (int)(((int64_t)d.mcux * d.mcuy * d.bpm + kCoefAlign - 1) & ~(int64_t)(kCoefAlign - 1));
}
// Index of the 16-byte piece (block ib, group g) from the image's dense region.
// npad < 2^24 (LDT_MAX_DIM 8192, 4:4:4), so this is one 24-bit multiply-add.
__host__ __device__ __forceinline__ uint32_t coef_piece(int ib, int g, int npad) {
  return __umul24((unsigned)g, (unsigned)npad) + (unsigned)ib;
}

struct DevWork {
  const uint8_t *data;  // compressed cells
  uint8_t *dstuf;       // destuffed entropy data
  int16_t *coef;        // baseline images: packed nonzero coefficient groups (above)
  uint32_t *brec;       // baseline images: per block group mask | run start << 8 | DC << 16
  uint32_t *bcarry;     // baseline images: per 64 blocks the first unit of the chunk's first block
  int16_t *pcoef;       // progressive images: dense group planes, all zero between batches
  int16_t *dcv;         // progressive images, per block (coef_off): absolute DC (k_prog)
  uint8_t *planes;      // component planes
  int32_t *status;      // per image
  int4 *ds_cnt;         // per destuff chunk: kept bytes, RSTn markers, end marker seen
};

hipError_t launch_destuff(const DevPlan &p, const DevWork &w, hipStream_t s);
hipError_t launch_huff_serial(const DevPlan &p, const DevWork &w, hipStream_t s);
hipError_t launch_huff_parallel(const DevPlan &p, const DevWork &w, hipStream_t s);
hipError_t launch_dc_scan(const DevPlan &p, const DevWork &w, hipStream_t s);
// *scaled (when given and a kernel is launched): 1 k_idct_scaled, 0 k_idct.
hipError_t launch_idct(const DevPlan &p, const DevWork &w, hipStream_t s, int *scaled = nullptr);
// Progressive (SOF2) images: serial per-scan decode into coef/dcv (ldt_prog.hip).
hipError_t launch_prog(const DevPlan &p, const DevWork &w, hipStream_t s);
// Failed rows: zero image, label -100 (after the resize kernels).
hipError_t launch_fill_failed(const DevPlan &p, const DevWork &w, float *out, int64_t *out_labels,
                              hipStream_t s);
// box 1: the batch has crops (ImgDesc box_* / flip): k_resize's BOX variant;
// box 2: the batch has windows (ImgDesc res_* / win_*, the box fields hold the
// crops or the whole image): the BOX == 2 variant. filter: kFilterBilinear or
// kFilterBicubic, the one p.max_ks_h / p.max_ks_v were planned with.
hipError_t launch_resize_jpeg(const DevPlan &p, const DevWork &w, float *out, int64_t *out_labels,
                              hipStream_t s, int box = 0, int filter = kFilterBilinear);
// A call with views > 1 (ldt_resize_stream.hip): the streaming resize over
// (image, view, band, tile), geometry from p.views, output image v * n + i of
// p.n_views * p.n; p.max_w and the tap counts cover every view. order: 0 an
// image's views adjacent in launch order, 1 view-major (LDT_OPT_VIEW_ORDER).
// The only launch of a call with views > 1, and of no other call.
hipError_t launch_resize_views(const DevPlan &p, const DevWork &w, float *out, int64_t *out_labels,
                               hipStream_t s, int filter, int order);
// Its workgroups; the launch needs them to fit an int.
int64_t resize_views_groups(int n, int views, int oh, int ow);
// Its failed rows: all p.n_views outputs zero bytes, label -100.
hipError_t launch_fill_failed_views(const DevPlan &p, const DevWork &w, float *out, int64_t *out_labels,
                                    hipStream_t s);
// The photometric stage of a call with colours (ldt_set_colors, ldt_color.hip).
// The resize has written the call's Pillow-exact bytes into `ws`, laid out as
// a uint8 NCHW output of the call (view-major, dense); the two kernels read
// them and store the call's real output. Their geometry, by value: the output
// size of each view, the first row tile of each view among an image's tiles
// (kColorRows rows each) and the first element of each view's dense block,
// which is the same in `ws` (bytes) and in the output (elements). A call
// without views is one view.
constexpr int kColorRows = 16;
struct ColorGeom {
  int32_t views = 0;
  int32_t tiles = 0; // row tiles of one image over all its views
  int32_t oh[kMaxViews], ow[kMaxViews];
  int32_t tile0[kMaxViews];
  int64_t base[kMaxViews];
};
// hw: [views][2] as (h, w), each in 1..kMaxOut. False when the grid (n * tiles
// workgroups) does not fit an int.
inline bool color_geom_build(int64_t n, int views, const int32_t *hw, ColorGeom &g) {
  g = ColorGeom();
  if (views < 1 || views > kMaxViews || n < 0 || n > 0x7FFFFFFF) return false;
  int64_t tiles = 0, base = 0;
  for (int v = 0; v < kMaxViews; ++v) {
    const bool in = v < views;
    g.oh[v] = in ? hw[2 * v] : 1;
    g.ow[v] = in ? hw[2 * v + 1] : 1;
    g.tile0[v] = (int32_t)tiles;
    g.base[v] = base;
    if (!in) continue;
    if (g.oh[v] < 1 || g.oh[v] > kMaxOut || g.ow[v] < 1 || g.ow[v] > kMaxOut) return false;
    tiles += (g.oh[v] + kColorRows - 1) / kColorRows; // at most 16 * 64
    base += n * 3 * g.oh[v] * g.ow[v];
  }
  if (n * tiles > 0x7FFFFFFF) return false;
  g.views = views;
  g.tiles = (int32_t)tiles;
  return true;
}
// colors: n * views entries on the device, image-major (row i, view v at
// i * views + v). sums: one zeroed counter per entry. k_color_mean adds the L
// of every pixel of the entries that have contrast, in the state the image has
// when contrast's turn comes; k_color_apply runs each entry's chain and stores
// through the 768-entry table `lut` (the form write_plan emits for fmt.dtype)
// in the call's format. Rows whose status is not 0 are skipped by both.
hipError_t launch_color_mean(const ldt_color *colors, const uint8_t *ws, uint32_t *sums, const int32_t *status,
                             int n, const ColorGeom &g, hipStream_t s);
hipError_t launch_color_apply(const ldt_color *colors, const uint8_t *ws, const uint32_t *sums,
                              const int32_t *status, const float *lut, float *out, OutFmt fmt, int n,
                              const ColorGeom &g, hipStream_t s);
// The blur of the entries that have one (blur_ww != 0; k_color_blur, after
// k_color_apply, which leaves those entries alone). One workgroup per (output
// image, tile of kBlurTileH x kBlurTileW pixels): it loads the tile and a halo
// of 3 * (r + 1) pixels per side, clipped to the image, from `ws`, applies the
// chain up to grayscale while loading, runs the six passes in LDS, then
// solarize, the table and the formatted store. Its geometry: an image's tiles
// over all its views, view after view, row-major inside a view.
constexpr int kBlurTileH = 32, kBlurTileW = 64;
struct BlurGeom {
  int32_t views = 0;
  int32_t tiles = 0; // tiles of one image over all its views
  int32_t oh[kMaxViews], ow[kMaxViews];
  int32_t tile0[kMaxViews]; // first tile of the view
  int32_t tiles_x[kMaxViews];
  int64_t base[kMaxViews];
};
// From the call's ColorGeom. False when the grid does not fit an int.
inline bool blur_geom_build(int64_t n, const ColorGeom &cg, BlurGeom &g) {
  g = BlurGeom();
  int64_t tiles = 0;
  for (int v = 0; v < kMaxViews; ++v) {
    g.oh[v] = cg.oh[v];
    g.ow[v] = cg.ow[v];
    g.base[v] = cg.base[v];
    g.tile0[v] = (int32_t)tiles;
    g.tiles_x[v] = (cg.ow[v] + kBlurTileW - 1) / kBlurTileW;
    if (v < cg.views) tiles += (int64_t)g.tiles_x[v] * ((cg.oh[v] + kBlurTileH - 1) / kBlurTileH); // at most 16 * 32
  }
  if (cg.views < 1 || n * tiles > 0x7FFFFFFF) return false;
  g.views = cg.views;
  g.tiles = (int32_t)tiles;
  return true;
}
// max_r: the largest blur_r among the entries (0..7); it sizes the launch's LDS.
hipError_t launch_color_blur(const ldt_color *colors, const uint8_t *ws, const uint32_t *sums,
                             const int32_t *status, const float *lut, float *out, OutFmt fmt, int n,
                             const BlurGeom &g, int max_r, hipStream_t s);
// The auto-augment stage of a call with augments (ldt_set_augments,
// ldt_augment.hip). The resize has written the call's bytes into `wsa` as it
// does for a call with colours; `wsb` is a second workspace of the same size.
// augs: n * views entries on the device, image-major. K: the largest count of
// the call; the stage is slots 0 .. max(K, 1) - 1, an entry with k ops running
// op j in slot K - k + j, reading wsa when j is even and wsb when it is odd
// and writing the other one, or the call's output in the last slot (through
// `lut`, in `fmt`, with the entry's erase box). stats: kAugStatBytes per entry,
// the 768-byte table of an autocontrast / equalize op, then the int32 rounded L
// mean of a contrast op: launch_aug_stats fills them for the entries whose op
// in `slot` needs them, ahead of that slot's launch_aug_apply. Rows whose
// status is not 0 are skipped by both.
// to_ws (a call with a mix): the last slot too writes uint8 planes to the other
// workspace, without the erase box or the table, so after the stage an entry
// with k ops has its final bytes in wsb when k is odd and in wsa when it is
// even (k = 0: the resize's own), and a stage with K = 0 needs no launch.
constexpr int kAugStatBytes = 784;
hipError_t launch_aug_stats(const ldt_aug *augs, const uint8_t *wsa, const uint8_t *wsb, uint8_t *stats,
                            const int32_t *status, int n, const ColorGeom &g, int slot, int K, hipStream_t s);
hipError_t launch_aug_apply(const ldt_aug *augs, uint8_t *wsa, uint8_t *wsb, const uint8_t *stats,
                            const int32_t *status, const float *lut, float *out, OutFmt fmt, int n,
                            const ColorGeom &g, int slot, int K, hipStream_t s, bool to_ws = false);
// The mix stage of a call with a mix (ldt_set_mix, ldt_mix.hip), the last
// before the store; one view. mix: n records on the device. src: where a row's
// final uint8 planes are: wsa (no colours or augments: the resize's workspace),
// wsb (colours: the photometric stage's uint8 output), or by the parity of the
// row's augment count (above). augs: the call's augment entries, whose erase
// boxes the kernel applies as the value 0 to a row and to its partner, or
// null. lut: the float32 table whatever the dtype. Rows whose status is not 0
// are skipped; a row whose partner's is not 0 is stored unmixed.
constexpr int kMixSrcA = 0, kMixSrcB = 1, kMixSrcByCount = 2;
hipError_t launch_mix_apply(const ldt_mix *mix, const ldt_aug *augs, const uint8_t *wsa, const uint8_t *wsb, int src,
                            const int32_t *status, const float *lut, float *out, OutFmt fmt, int n,
                            const ColorGeom &g, hipStream_t s);
// soft: float32 [n][num_classes], every element written (zero rows for failed
// rows, 1.0f at its label for a row whose partner failed). labels: the plan's.
hipError_t launch_mix_labels(const ldt_mix *mix, const int64_t *labels, const int32_t *status, float *soft, int n,
                             int num_classes, hipStream_t s);
// One-wave-per-band resize (ldt_resize4.hip); false when unsupported (taps
// > 11, i.e. sources wider than 5 x out_w, outputs wider than kTileCols, a
// width without a table entry, or LDS), then the streaming
// workgroup kernel (launch_resize_jpeg / launch_resize_raw) is used.
// *wpg_used: the waves per workgroup the launch took (a tall batch may need
// fewer than the default to fit the LDS) and *bands_used the bands per image;
// untouched when it returns false
bool launch_resize4_jpeg(const DevPlan &p, const DevWork &w, float *out, int64_t *out_labels,
                         hipStream_t s, hipError_t *err, int *wpg_used = nullptr, int *bands_used = nullptr);
// k_resize4 loads its coefficients from the cached tables (ResizeOut): the
// entries of every width in the batch, and of every height that has one
// (resamp_cached), must have been filled on `s` (launch_fill_resample). Other
// heights' vertical coefficients are computed in the kernel.
bool launch_resize4_raw(const uint8_t *hwc, int64_t cell_stride, int n, int h, int wd,
                        const float *lut, const ResizeOut &ro, float *out, hipStream_t s,
                        hipError_t *err);
// Fills the entries of sz.n <= kResampFill input sizes in a table whose rows
// have `out` entries (each size cached for that table: resamp_cached).
constexpr int kResampFill = 120;
struct ResampSizes {
  int32_t n;
  uint16_t size[kResampFill];
};
hipError_t launch_fill_resample(const ResampSizes &sz, int32_t *tab, int out, hipStream_t s);
// boxes: null, or n crops on the device, each inside h x w, none wider than
// box_w or taller than box_h: k_resize's BOX variant. wins: null, or n windows
// on the device, each inside its res and no row's source (box, or the cell
// when boxes is null) reduced by more than kMaxReduce against its res; win_ks_h
// and win_ks_v are the most taps of any row's (source -> res): the BOX == 2
// variant. filter: the call's filter; the taps (win_ks_* too) and the limit
// are that filter's (resample_ksize_host, resample_reduce). fmt: the output
// format, with `lut` in its dtype's form (ResizeOut::fmt).
hipError_t launch_resize_raw(const uint8_t *hwc, int64_t cell_stride, int n, int h, int w,
                             const float *lut, int oh, int ow, float *out, hipStream_t s,
                             const ldt_crop *boxes = nullptr, int box_w = 0, int box_h = 0,
                             const ldt_window *wins = nullptr, int win_ks_h = 0, int win_ks_v = 0,
                             int filter = kFilterBilinear, OutFmt fmt = OutFmt());
hipError_t launch_resample_coeffs(int in_size, int out_size, int ksize, int32_t *bounds,
                                  int32_t *kk, hipStream_t s);
hipError_t launch_shard_ranges(int64_t num_rows, int64_t bsz, int rank, int world, int64_t *out,
                               int64_t capacity, int64_t *count, hipStream_t s);
hipError_t launch_shard_fragments(const int64_t *frag_rows, int nfrag, int64_t bsz, int rank,
                                  int world, int64_t pad_to, int64_t *out, int64_t capacity,
                                  int64_t *count, int64_t *local_count, hipStream_t s);
// DistributedSampler indices (ldt_sampler.hip). Shuffled: the rank's
// num_samples entries of torch.randperm(n) strided from rank (H, head, nxt: n
// int32 each of scratch). launch_dist_select: the unshuffled identity.
hipError_t launch_dist_shuffled(uint32_t seed, int64_t n, int rank, int world,
                                int64_t num_samples, int32_t *H, int32_t *head, int32_t *nxt,
                                int64_t *out, hipStream_t s);
hipError_t launch_dist_select(const int32_t *perm, int64_t n, int rank, int world,
                              int64_t num_samples, int64_t *out, hipStream_t s);

} // namespace ldt
