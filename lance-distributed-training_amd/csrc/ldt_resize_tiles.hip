// ldt_resize_tiles.hip — the store of a tile call (ldt_decode_tiles): every
// good row's source rectangle resized to its own res_h x res_w (Pillow's
// BILINEAR or BICUBIC bit for bit), pasted at (top, left) of a canvas of
// rows x cols square tiles of S pixels whose rest is the call's fill, and
// stored as those tiles in row-major order, each a dense [3, S, S] (or
// [S, S, 3]) block of the row's region; where the call asks for thumbnails and
// the canvas has more than one tile, the rectangle resized to S x S follows.
// That is what the tiled vision-language towers take (InternVL's
// dynamic_preprocess, Llama 3.2 Vision's fit, pad and split). It is launched
// in place of k_resize_ragged, whose plan it shares (prefix, int64 offsets, the
// uniform binary search); the per-row section holds kTileRowWords words.
//
// k_resize_tiles<FILT>. The unit of work is an output tile, not a piece of the
// resized image: one workgroup of 256 lanes serves kTileRows output rows by one
// column chunk of one output tile, so it has a single destination block and no
// store straddles two tiles. A tile's S columns are ceil(S / 256) chunks, of 256
// columns and a remainder (448: 256 and 192; the even split, two of 224,
// measured a little slower), see tile_chunk_cols. All tiles of
// all rows, thumbnails included, sit in one grid (the prefix is over
// workgroups): workgroup t of a row is output tile k = t / tile_groups(S),
// then band and chunk; k < rows * cols is canvas tile (a, b) = (k / cols,
// k % cols), k == rows * cols the thumbnail.
//
// Index map, before any load. Pixel (y, x) of canvas tile (a, b) is canvas
// (a * S + y, b * S + x), which is resized pixel (i, j) = (Y - top, X - left);
// a thumbnail's (y, x) is pixel (y, x) of the S x S resize. A lane owns its
// output column. When the row is flipped the lane computes the coefficients of
// the mirrored resized column res_w - 1 - j: the mirror is on the tap side,
// since a mirrored store would leave the chunk grid once a placement is
// involved. Lanes with j outside [0, res_w) and rows with i outside [0, res_h)
// are fill; the live lanes and rows are one interval each. The staged source
// span is the union of the live lanes' windows: from the window of the first
// live lane to that of the last, the other way round when flipped.
//
// A workgroup whose chunk holds no live pixel (a uniform branch) computes no
// coefficient, stages nothing, runs no tap and stores table entries of the
// fill. Every other runs resize_rows (ldt_resize_rows.hpp), the body
// k_resize_ragged has: the span's bytes in aligned 8-byte loads, chroma_at /
// ycc_to_rgb once per staged pixel, horizontal taps to a clip8 byte, the
// vertical accumulators of the kTileRows rows in registers.
//
// Store. By destination address, as k_resize_ragged does: in steps of four
// rows every lane puts its column's element bits (the call's 768-entry table in
// LDS; a fill pixel is the table's entry for the fill byte, the byte itself
// under uint8, as the padded streaming resize stores it) into the four waves'
// row buffers, and each wave stores its row's runs with store_run. The label is
// written once per image. A failed row is not touched: k_native_fill does it.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ldt_device.hpp"
#include "ldt_kernels.hpp"
#include "ldt_resize_rows.hpp"

#pragma clang fp contract(off)

namespace ldt {
namespace {

constexpr int kTilThreads = 256, TR = kTileRows;
static_assert(kRagTileCols == kTilThreads, "one lane per column of a chunk; ragged_span_bound bounds its span");
static_assert(3072 + 4 * 3 * kRagTileCols * 4 >= LDT_MAX_DIM, "a chroma region's base minus its first column stays in LDS");

template <int FILT>
__global__ void __launch_bounds__(kTilThreads)
    k_resize_tiles(const ImgDesc *__restrict__ descs, const uint8_t *__restrict__ planes,
                   const int32_t *__restrict__ status, const int32_t *__restrict__ group_pref,
                   const int64_t *__restrict__ nat_off, const int32_t *__restrict__ tile_rows, int n,
                   const float *__restrict__ lut, const int64_t *__restrict__ labels, uint8_t *__restrict__ out,
                   int64_t *__restrict__ out_labels, OutFmt fmt, TilesCap cap) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x, group = blockIdx.x;
  // the image whose workgroups hold this one, as k_emit_rgb finds it
  int img = 0;
  for (int hi = n; hi - img > 1;) {
    const int mid = (img + hi) >> 1;
    if (group_pref[mid] <= group) img = mid;
    else hi = mid;
  }
  if (status[img] != 0) return;
  const ImgDesc &d = descs[img];
  const int32_t *g = tile_rows + kTileRowWords * img;
  const int S = cap.s.tile, cols = g[3], ncanvas = g[2] * cols;
  const int chunks = tile_chunks(S), CW = tile_chunk_cols(S);
  // ---- which output tile, and which rows and columns of it ----
  const int t = group - group_pref[img];
  const int k = t / tile_groups(S), rest = t - k * tile_groups(S);
  const int band = rest / chunks, chunk = rest - band * chunks;
  const bool thumb = k >= ncanvas;
  const int a = thumb ? 0 : k / cols, b = thumb ? 0 : k - a * cols;
  const int rh = thumb ? S : g[0], rw = thumb ? S : g[1];
  const int x0 = chunk * CW, y0 = band * TR;
  const int ncols = min(CW, S - x0), nrows = min(TR, S - y0);
  // the resized pixel of the chunk's first lane and row, and the live intervals
  const int j0 = b * S + x0 - (thumb ? 0 : g[5]), i0 = a * S + y0 - (thumb ? 0 : g[4]);
  const int l0 = max(0, -j0), l1 = min(ncols, rw - j0);
  const int r0 = max(0, -i0), r1 = min(nrows, rh - i0);
  const bool any = l0 < l1 && r0 < r1; // uniform
  const int W = d.box_w, H = d.box_h;
  const int ks_h = resample_ksize_host(W, rw, FILT), ks_v = resample_ksize_host(H, rh, FILT);
  // what the planner checked and sized the LDS by holds this chunk (uniform; never taken)
  if (ncols < 1 || nrows < 1 || k > ncanvas || CW * ks_h > cap.kh_words || ks_v > cap.ks_v) return;
  if (t == 0 && tid == 0 && labels != nullptr) out_labels[img] = labels[img];

  const RaggedLds L = tiles_lds(cap);
  uint32_t *s_lut = reinterpret_cast<uint32_t *>(smem);
  uint32_t *s_out = s_lut + 768; // [4][3 * kRagTileCols]
  int32_t *s_hb = reinterpret_cast<int32_t *>(smem + L.hb);
  int32_t *s_vb = reinterpret_cast<int32_t *>(smem + L.vb);
  int32_t *s_kv = reinterpret_cast<int32_t *>(smem + L.kv);
  int32_t *s_kh = reinterpret_cast<int32_t *>(smem + L.kh);

  const int es = dtype_bytes(fmt.dtype);
  for (int i = tid; i < 768; i += kTilThreads)
    s_lut[i] = es == 4   ? reinterpret_cast<const uint32_t *>(lut)[i]
               : es == 2 ? (uint32_t) reinterpret_cast<const uint16_t *>(lut)[i]
                         : (uint32_t)(i & 255);

  const bool live = any && tid >= l0 && tid < l1;
  int32_t acc[TR][3];
#pragma unroll
  for (int j = 0; j < TR; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 1 << (kPrecisionBits - 1);
  if (any) {
    // ---- coefficients: a live lane its (mirrored) column, the last TR lanes a row each ----
    if (live) {
      const int j = j0 + tid;
      int xmin;
      const int cnt = resample_coeffs<FILT>(W, rw, d.flip ? rw - 1 - j : j, ks_h, s_kh + tid * ks_h, &xmin);
      s_hb[2 * tid] = xmin;
      s_hb[2 * tid + 1] = cnt;
    }
    if (tid >= kTilThreads - TR) {
      const int j = tid - (kTilThreads - TR);
      int ymin = 0, cnt = 0; // a fill row, or one past the tile: an empty window
      if (j >= r0 && j < r1) cnt = resample_coeffs<FILT>(H, rh, i0 + j, ks_v, s_kv + j * ks_v, &ymin);
      s_vb[2 * j] = ymin;
      s_vb[2 * j + 1] = cnt;
    }
    __syncthreads();
    // the union of the live lanes' windows: they move left with the lane when the row is flipped
    const int lo = d.flip ? l1 - 1 : l0, hi = d.flip ? l0 : l1 - 1;
    const int xa = s_hb[2 * lo], span = s_hb[2 * hi] + s_hb[2 * hi + 1] - xa;
    const int ya = s_vb[2 * r0], yb = s_vb[2 * (r1 - 1)] + s_vb[2 * (r1 - 1) + 1];
    if (span > cap.span || span < 1 || xa < 0 || xa + span > W || ya < 0 || yb > H) return; // uniform; never taken
    int hoff = 0, hcnt = 0;
    if (live) {
      hoff = s_hb[2 * tid] - xa;
      hcnt = s_hb[2 * tid + 1];
    }
    resize_rows<TR, kTilThreads>(d, planes, smem, L, ragged_pitch(cap.span), xa, span, ya, yb, live, hoff, hcnt,
                                 s_kh + tid * ks_h, ks_v, acc);
  } else {
    __syncthreads(); // the table is in
  }

  // ---- store: steps of four rows, a wave a row, by destination address ----
  const int wave = tid >> 6, lane = tid & 63;
  const bool nhwc = fmt.layout == kLayoutNHWC;
  uint8_t *ob = out + (nat_off[img] + (int64_t)k * 3 * S * S) * es; // the output tile's block
#pragma unroll
  for (int step = 0; step < TR / 4; ++step) {
    if (4 * step >= nrows) break; // uniform
    if (tid < ncols) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool pix = live && 4 * step + r >= r0 && 4 * step + r < r1;
#pragma unroll
        for (int c = 0; c < 3; ++c)
          s_out[r * 3 * kRagTileCols + (nhwc ? tid * 3 + c : c * kRagTileCols + tid)] =
              s_lut[c * 256 + (pix ? clip8(acc[4 * step + r][c]) : (uint32_t)cap.s.fill[c])];
      }
    }
    __syncthreads();
    const int oy = y0 + 4 * step + wave;
    if (4 * step + wave < nrows) {
      const uint32_t *orow = s_out + wave * 3 * kRagTileCols;
      if (nhwc) {
        store_run(ob + (((int64_t)oy * S + x0) * 3) * es, orow, 3 * ncols, es, lane);
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
          store_run(ob + (((int64_t)c * S + oy) * S + x0) * es, orow + c * kRagTileCols, ncols, es, lane);
      }
    }
    __syncthreads(); // the next step overwrites the row buffers
  }
}

} // namespace

hipError_t launch_resize_tiles(const DevPlan &p, const DevWork &w, float *out, int64_t *out_labels, hipStream_t s,
                               int filter) {
  if (p.nat_tiles_total == 0) return hipSuccess;
  const int lds = tiles_lds(p.til).bytes;
  if (!tile_spec_ok(p.til.s.tile, p.til.s.thumbnail, p.til.s.reserved) || lds > kRaggedLdsMax)
    return hipErrorInvalidValue;
  const auto kern = filter == kFilterBicubic ? &k_resize_tiles<kFilterBicubic> : &k_resize_tiles<kFilterBilinear>;
  // up to the full 160 KiB of LDS (wide boxes under a large reduction), once per kernel
  static hipError_t attr[2] = {
      hipFuncSetAttribute(reinterpret_cast<const void *>(&k_resize_tiles<kFilterBilinear>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, kRaggedLdsMax),
      hipFuncSetAttribute(reinterpret_cast<const void *>(&k_resize_tiles<kFilterBicubic>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, kRaggedLdsMax)};
  if (attr[filter == kFilterBicubic] != hipSuccess) return attr[filter == kFilterBicubic];
  hipLaunchKernelGGL(kern, dim3(p.nat_tiles_total), dim3(kTilThreads), lds, s, p.descs, w.planes, w.status,
                     p.nat_tiles, p.nat_off, p.nat_res, p.n, p.lut, p.labels, reinterpret_cast<uint8_t *>(out),
                     out_labels, p.ro.fmt, p.til);
  return hipGetLastError();
}

} // namespace ldt
