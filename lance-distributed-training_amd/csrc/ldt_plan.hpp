// ldt_plan.hpp — the host-side planner of libldt.so. plan_batch turns a
// batch of untrusted JPEG cells into row statuses, image descriptors, tables
// and every size and offset of the device workspace (marker walk SOI..SOS,
// Huffman table derivation, the progressive scan walk, decoder routing,
// destuff chunks); plan_layout / write_plan lay that out as the plan blob.
// Everything here works on plain host memory and makes no HIP call, so
// tests/test_plan_fuzz.py also builds ldt_plan.cpp for the CPU with
// AddressSanitizer + UBSan and drives the same functions
// (tests/fuzz/plan_fuzz.cpp). ldt_abi.cpp only consumes the results.
#pragma once
#include <stdint.h>

#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/ldt.h"
#include "ldt_types.hpp"
#include "ldt_view_index.hpp"

namespace ldt {

// ---------------------------------------------------------------------------
// Marker walk (ITU T.81 B.2; libjpeg jdmarker.c semantics for the subset).
// ---------------------------------------------------------------------------
struct RawHuff {
  uint8_t counts[16];
  uint8_t syms[256];
  int nsym;
  bool present;
};

struct Header {
  int width = 0, height = 0, ncomp = 0;
  int cid[4], h[4], v[4], tq[4], td[4], ta[4];
  uint16_t q[4][64]; // natural order
  bool qpresent[4] = {false, false, false, false};
  RawHuff dc[4], ac[4];
  int restart = 0;
  bool jfif = false, adobe = false;
  int adobe_transform = -1;
  int64_t scan_pos = 0; // offset of entropy-coded data within the cell
                        // (progressive: of the first SOS marker)
  bool progressive = false;
};

struct ProgPlan {
  std::vector<ProgScan> scans;                // tab[]: indices into tabs
  std::vector<std::pair<RawHuff, bool>> tabs; // (table, is_dc)
  uint16_t q[4][64];                          // latched quant tables, natural order
};

// Returns an LDT_IMG_* code (include/ldt.h).
int walk_markers(const uint8_t *cell, int64_t len, Header &H);
// jdhuff.c jpeg_make_d_derived_tbl into the device layout; false = bad table.
bool build_huff(const RawHuff &r, bool is_dc, HuffTab &t);
std::string huff_key(const RawHuff &r, bool dc);
bool build_prog_tab(const RawHuff &r, bool is_dc, ProgTab &t);
// Returns an LDT_IMG_* code.
int plan_progressive(const uint8_t *cell, int64_t len, const Header &H0, ProgPlan &P);


// ---------------------------------------------------------------------------
// Per-batch planning.
// ---------------------------------------------------------------------------
// The context settings planning reads.
struct PlanOptions {
  bool parallel = true;     // huff_mode != 1: images may take k_huff_image
  int subseq_bits = 256;    // minimum S of the parallel decoder
  bool fuse_destuff = true; // LDT_OPT_FUSED_DESTUFF
  int64_t win_cap = -1;     // LDT_OPT_HUFF_WINDOW (bytes; -1 none)
  int out_h = kOut, out_w = kOut; // the context's output size (ldt_set_output_size)
  int filter = kFilterBilinear;   // the call's filter (ldt_set_filter): the reduction limit and the taps are its
};

// Baseline Huffman tables derived so far, deduped over a context's lifetime.
struct HuffCache {
  std::unordered_map<std::string, int> map; // huff_key -> index in tabs
  std::vector<HuffTab> tabs;
};

struct BatchPlan {
  std::vector<ImgDesc> descs;   // one per row
  std::vector<Segment> segs;    // baseline images' restart intervals, row order
  std::vector<int32_t> status;  // LDT_IMG_* per row
  std::vector<HuffTab> htabs;   // this batch's baseline tables (ImgDesc::dct/act)
  std::vector<uint16_t> qtabs;  // 64 per table, natural order (ImgDesc::qt)
  std::vector<int32_t> par_img; // images on the parallel decoder (one workgroup each)
  std::vector<int32_t> chunk_img; // destuff chunk -> image
  std::vector<int32_t> prog_img;  // progressive images (k_prog)
  std::vector<ProgScan> pscans;   // their scans
  std::vector<ProgTab> ptabs;
  int64_t dst_total = 0, coef_blocks = 0, pcoef_blocks = 0, plane_total = 0, max_blocks = 0;
  int64_t max_window = 0; // largest LDS window a parallel image needs
  // LDS window of k_huff_image: the largest image's stream, capped by what is
  // left of the CU's LDS after the tables (bigger streams read global)
  int win_bytes = 0;
  int n_serial = 0;
  int32_t n_chunks = 0; // destuff chunks (kDsChunkBytes of scan data each)
  int n_ds_img = 0;     // baseline images left to k_destuff_*
  int max_w = 1, max_h = 1, max_ks_h = 3, max_ks_v = 3, max_tabs = 1, n_fast420 = 0;
  int n_draft = 0; // good rows with a draft scale above 1: k_idct_scaled runs when there is one
  bool any_bad = false;
  // a call with views > 1 (ldt_set_views): the view table, n_views * n entries
  // indexed by output image v * n + i; empty for a single view
  std::vector<ViewDesc> views;
  int n_views = 1;
  // a call with per-view output sizes (ldt_set_view_sizes): the geometry table
  // (ldt_view_index.hpp); geom.views == 0 otherwise. The view table then exists
  // for one view too, and its entries' spare words carry the view's size.
  ViewGeomTab geom;
  bool geom_bad = false; // sizes were given and refused (range, or more workgroups than a launch takes)
};

// Plans rows [arr_offset, arr_offset + n) of an Arrow binary array: cell r is
// data[offsets[r] .. offsets[r + 1]), validity is the array's bitmap or null.
// Offsets in the plan are relative to offsets[arr_offset]. OffT: int32_t or
// int64_t. A bad row gets its status and a 1x1 descriptor; it never fails the batch.
// crops: null, or n boxes (ldt_set_crops), each checked against its row's
// header (LDT_IMG_BAD_CROP; LDT_IMG_TOO_LARGE on the box's reduction). The
// descriptors carry the box and flip (the whole image without crops), and
// max_w, max_h, max_ks_h, max_ks_v of a cropped batch are those of its boxes.
// windows: null, or n windows (ldt_set_windows), each checked against the
// output size (LDT_IMG_BAD_WINDOW); the row's source (box or whole image) is
// then held to the reduction limit against res (LDT_IMG_TOO_LARGE), the
// descriptors carry res and the window's origin (out_h, out_w, 0, 0 without
// windows), and max_ks_h / max_ks_v are those of (source -> res).
// opt.filter: the reduction limit and the taps are that filter's
// (resample_reduce, resample_ksize_host); the order of a row's errors stays
// window, crop, too large.
// views (ldt_set_views, 1..kMaxViews): crops and windows then hold n * views
// rows, image-major (row i, view v at i * views + v). A row's views are checked
// in order v = 0..views-1, each as above, and the first that fails gives the
// row its status; max_w, max_h, max_ks_h and max_ks_v cover every view of every
// good row; with views > 1 B.views holds the view table (ViewDesc, view-major)
// and the descriptors carry view 0. views = 1 is the call without it.
// view_sizes (ldt_set_view_sizes): null, or `views` pairs (h, w): view v is
// then checked (check_window, check_crop's reduction limit) against its own
// size, a missing window defaults to (h_v, w_v, 0, 0), max_ks_* cover every
// view's (box -> res), the view table exists for views = 1 too and every entry
// (a failed row's included) carries its view's size in pad_[0], pad_[1], and
// B.geom holds the geometry table. Sizes that view_geom_build refuses set
// B.geom_bad and fail every row with LDT_IMG_BAD_WINDOW: nothing of such a
// plan may be launched. opt.out_h / out_w are not read for a view then.
// drafts (ldt_set_draft): null, or n scales, each 1, 2, 4 or 8 (the caller has
// checked them). Row i decodes to ceil(W / s) x ceil(H / s), the image libjpeg
// gives at scale 1 / s, and every word above about the decoded image, its
// boxes, limits and taps then means that image; LDT_MAX_DIM alone stays a
// bound on the file's own size. The descriptor carries the scale, each
// component's DCT_scaled_size and whether fancy upsampling is off (ImgDesc
// draft, sc, nofancy); planes are blocks_w * sc wide with the stride rounded up
// to kPlaneStrideAlign. A row without a draft is planned exactly as before.
template <typename OffT>
void plan_batch(const uint8_t *data, const OffT *offsets, int64_t arr_offset, int64_t n,
                const uint8_t *validity, const PlanOptions &opt, HuffCache &cache, BatchPlan &B,
                const ldt_crop *crops = nullptr, const ldt_window *windows = nullptr, int views = 1,
                const int32_t *view_sizes = nullptr, const int32_t *drafts = nullptr);
// The LDT_IMG_* code of a crop against a width x height image resized to
// out_h x out_w with `filter`: LDT_IMG_BAD_CROP, LDT_IMG_TOO_LARGE
// (ceil(support * box / out) > kMaxReduce on an axis: support 1 for BILINEAR,
// 2 for BICUBIC) or LDT_IMG_OK.
int check_crop(const ldt_crop &c, int width, int height, int out_h, int out_w, int filter = kFilterBilinear);
// The LDT_IMG_* code of a window against the output size: LDT_IMG_BAD_WINDOW
// (res outside 1..LDT_MAX_RES, a negative origin, or the out_h x out_w window
// at (top, left) not inside res_h x res_w) or LDT_IMG_OK. The reduction limit
// of a row with a window is check_crop's with res_h, res_w in place of the
// output size.
int check_window(const ldt_window &w, int out_h, int out_w);

// Byte offsets of the plan blob's sections (each 64-byte aligned, in this order).
struct PlanLayout {
  int64_t off_desc, off_seg, off_huff, off_quant, off_lut, off_labels, off_status, off_par,
      off_chunk, off_redo /* 64 bytes of debug counters */, off_pscan, off_ptab, off_pimg;
  int64_t plan_bytes;
  int64_t off_view; // the view table (BatchPlan::views), the last section; empty for a single view
};
PlanLayout plan_layout(const BatchPlan &B, bool has_labels);
// Writes the blob (L.plan_bytes at dst); labels: the batch's n labels, or null.
// dtype (kDtype*): the form of the table at off_lut: 768 float32 entries
// (kDtypeF32, and kDtypeU8, whose kernels do not read it) or 768 16-bit ones
// (build_lut16) in the section's first half.
void write_plan(const BatchPlan &B, const PlanLayout &L, const ldt_norm *norm, const int64_t *labels,
                uint8_t *dst, int dtype = kDtypeF32);
// ToTensor + Normalize as a table: lut[c * 256 + v], bit-exact with torchvision.
void build_lut(const ldt_norm *norm, float *lut);
// float32 -> IEEE binary16 / bfloat16 bits, round-to-nearest-even, as
// torch's Tensor.to(dtype) computes them on the CPU: fp16 overflow is +-inf,
// fp16 subnormals are kept, a NaN stays a (quiet) NaN.
uint16_t f32_to_f16_bits(float f);
uint16_t f32_to_bf16_bits(float f);
// build_lut's 768 entries converted to kDtypeF16 or kDtypeBF16.
void build_lut16(const ldt_norm *norm, int dtype, uint16_t *lut);

} // namespace ldt
