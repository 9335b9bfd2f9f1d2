// ldt_resize_ragged.hip — the store of a native call with per-row sizes
// (ldt_set_native_sizes): every good row's source rectangle (its box, else the
// whole decoded image) resized to the row's own res_h x res_w with Pillow's
// BILINEAR or BICUBIC, Image.resize((w_i, h_i), filter) bit for bit, in the
// call's dtype and layout, at the row's own offset of a ragged output. It is
// launched in place of k_emit_rgb (ldt_native.hip), whose ragged plan it
// shares (tile prefix, int64 offsets, the uniform binary search), and joins it
// to the two passes of the streaming resize (ldt_resize_stream.hpp).
//
// k_resize_ragged<FILT>. One workgroup of 256 lanes serves one tile of
// kRagTileRows x kRagTileCols (TR x 256) output pixels of one image; the
// tiles of all images sit in one grid. Everything about the tile comes from
// the row's own geometry: the box from the descriptor, (res_h, res_w) from the
// plan's size section, the tap capacities from resample_ksize_host on those.
//
// Column-span staging. A lane below the tile's width computes its output
// column's coefficients first; the tile then reads source columns
// [xmin(first column), xmin(last column) + count(last column)) and nothing
// else of the box, since the windows move right with the output column. The
// span is at most ragged_span_bound (ldt_types.hpp) columns, which the
// planner took the launch's maximum of: the dynamic LDS is laid out by that
// maximum (ragged_lds), and a tile that found a wider span would return
// without touching memory (it cannot: the bound is proved there).
//
// Per source row of the band (ymin(first row) .. ymin(last row) + count(last
// row)), two stages and two barriers:
//   raw   the span's luma bytes and, per chroma component, the one or two
//         chroma rows this luma row's upsampling reads, over the span's chroma
//         columns and a halo sample on each side, in aligned 8-byte loads
//         (planes start 256-aligned, strides are multiples of 8);
//   rgb   one lane per staged column: chroma_at (ldt_device.hpp) on a
//         descriptor whose plane stride is the LDS pitch, whose rows count
//         from the region's first and whose base is moved back by the
//         region's first column, as k_emit_rgb hands it its regions: the
//         fancy-upsampling edge rules, the cdw <= 2 exceptions and nofancy
//         stay that helper's code on the image's absolute coordinates. Then
//         ycc_to_rgb, RGB passthrough or grey replicated, once per pixel.
// The raw buffers are the ring: row y + 1 is loaded into them while the taps
// of row y still read the RGB row, which is rewritten only after the barrier
// that ends the loads.
//
// Taps. Pillow's order, the streaming body's split: a lane owns one output
// column, takes the horizontal tap sum of each staged row to a uint8 value
// (clip8) and accumulates the vertical taps of its TR output rows in
// registers (3 * TR int32), so the image between the passes never leaves the
// lane. resample_coeffs<FILT> and clip8 are ldt_resample.hpp's, with
// floating-point contraction off in this file.
//
// Store. By destination address, as k_emit_rgb does: in steps of four rows
// every lane puts its column's element bits (the call's 768-entry table, in
// LDS) into the four waves' row buffers in output order (planar under NCHW,
// interleaved under NHWC, mirrored when the row is flipped), and each wave
// stores its row's runs with store_run: element stores up to the first
// 4-element boundary and after the last, vectors between. The label is
// written once per image. A failed row is not touched: k_native_fill does it.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ldt_device.hpp"
#include "ldt_kernels.hpp"

#pragma clang fp contract(off)

namespace ldt {
namespace {

constexpr int kRagThreads = 256, TR = kRagTileRows;
static_assert(kRagTileCols == kRagThreads, "one lane per column of a tile");
static_assert(3072 + 4 * 3 * kRagTileCols * 4 >= LDT_MAX_DIM, "a chroma region's base minus its first column stays in LDS");

__device__ __forceinline__ uint2 load8(const uint8_t *p) { return *reinterpret_cast<const uint2 *>(p); }

template <int FILT>
__global__ void __launch_bounds__(kRagThreads)
    k_resize_ragged(const ImgDesc *__restrict__ descs, const uint8_t *__restrict__ planes,
                    const int32_t *__restrict__ status, const int32_t *__restrict__ tile_pref,
                    const int64_t *__restrict__ nat_off, const int32_t *__restrict__ nat_res, int n,
                    const float *__restrict__ lut, const int64_t *__restrict__ labels, uint8_t *__restrict__ out,
                    int64_t *__restrict__ out_labels, OutFmt fmt, RaggedCap cap) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x, tile = blockIdx.x;
  // the image whose tiles hold this one, as k_emit_rgb finds it
  int img = 0;
  for (int hi = n; hi - img > 1;) {
    const int mid = (img + hi) >> 1;
    if (tile_pref[mid] <= tile) img = mid;
    else hi = mid;
  }
  if (status[img] != 0) return;
  const ImgDesc &d = descs[img];
  const int W = d.box_w, H = d.box_h, rh = nat_res[2 * img], rw = nat_res[2 * img + 1];
  const int t = tile - tile_pref[img];
  const int tiles_x = (rw + kRagTileCols - 1) / kRagTileCols;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int ox0 = tx * kRagTileCols, oy0 = ty * TR;
  const int ncols = min(kRagTileCols, rw - ox0), nrows = min(TR, rh - oy0);
  const int ks_h = resample_ksize_host(W, rw, FILT), ks_v = resample_ksize_host(H, rh, FILT);
  // what the planner sized the LDS by holds this tile (uniform; never taken)
  if (ncols * ks_h > cap.kh_words || ks_v > cap.ks_v) return;
  if (t == 0 && tid == 0 && labels != nullptr) out_labels[img] = labels[img];

  const RaggedLds L = ragged_lds(cap);
  const int pitch = ragged_pitch(cap.span);
  uint32_t *s_lut = reinterpret_cast<uint32_t *>(smem);
  uint32_t *s_out = s_lut + 768; // [4][3 * kRagTileCols]
  int32_t *s_hb = reinterpret_cast<int32_t *>(smem + L.hb);
  int32_t *s_vb = reinterpret_cast<int32_t *>(smem + L.vb);
  int32_t *s_kv = reinterpret_cast<int32_t *>(smem + L.kv);
  int32_t *s_kh = reinterpret_cast<int32_t *>(smem + L.kh);
  uint8_t *s_y = smem + L.y;
  uint8_t *s_rgb = smem + L.rgb;

  const int es = dtype_bytes(fmt.dtype);
  for (int i = tid; i < 768; i += kRagThreads)
    s_lut[i] = es == 4   ? reinterpret_cast<const uint32_t *>(lut)[i]
               : es == 2 ? (uint32_t) reinterpret_cast<const uint16_t *>(lut)[i]
                         : (uint32_t)(i & 255);
  // ---- coefficients: a lane a column, the last TR lanes a row each ----
  if (tid < ncols) {
    int xmin;
    const int cnt = resample_coeffs<FILT>(W, rw, ox0 + tid, ks_h, s_kh + tid * ks_h, &xmin);
    s_hb[2 * tid] = xmin;
    s_hb[2 * tid + 1] = cnt;
  }
  if (tid >= kRagThreads - TR) {
    const int j = tid - (kRagThreads - TR);
    int ymin = 0, cnt = 0; // a row past the image: an empty window
    if (j < nrows) cnt = resample_coeffs<FILT>(H, rh, oy0 + j, ks_v, s_kv + j * ks_v, &ymin);
    s_vb[2 * j] = ymin;
    s_vb[2 * j + 1] = cnt;
  }
  __syncthreads();
  const int xa = s_hb[0], span = s_hb[2 * (ncols - 1)] + s_hb[2 * (ncols - 1) + 1] - xa;
  const int ya = s_vb[0], yb = s_vb[2 * (nrows - 1)] + s_vb[2 * (nrows - 1) + 1];
  if (span > cap.span) return; // uniform; the planner's bound says never

  // ---- the span in the image, and what of each plane holds it ----
  const int X0 = d.box_left + xa, xa8 = X0 & ~7;
  const int ychunks = (X0 + span - xa8 + 7) >> 3; // 8 * ychunks <= span + 14 <= pitch; ends inside the stride
  const uint8_t *py = planes + d.plane_off[0] + xa8;
  const int color = d.color;
  // chroma_at's view of a component's staged rows: the fields it reads, the
  // LDS pitch as the stride, rows counted from the region's first (cdh, and
  // the y handed to it, move by a whole number of chroma rows per source row)
  ImgDesc ld;
  ld.nofancy = d.nofancy;
  ld.vf[1] = ld.vf[2] = 1;
  int ca[2] = {0, 0}, cchunks[2] = {0, 0};
  if (color != 2) {
#pragma unroll
    for (int c = 1; c <= 2; ++c) {
      const int hf = d.hf[c], dw = d.cdw[c];
      ld.hf[c] = hf, ld.vf[c] = d.vf[c], ld.cdw[c] = dw;
      ld.plane_stride[c] = pitch;
      const int cx0 = max(X0 / hf - 1, 0), cx1 = min((X0 + span - 1) / hf + 1, dw - 1);
      ca[c - 1] = cx0 & ~7;
      cchunks[c - 1] = (cx1 - ca[c - 1] + 8) >> 3; // 8 * cchunks <= span + 16 <= pitch; cx1 < cdw <= the stride
    }
  }
  // the regions moved back by their first column, so that the image's chroma
  // columns index them: a byte offset into smem that is never negative
  const uint8_t *vb[2] = {smem + (L.c - ca[0]), smem + (L.c + 2 * pitch - ca[1])};

  int32_t acc[TR][3];
#pragma unroll
  for (int j = 0; j < TR; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 1 << (kPrecisionBits - 1);
  int hoff = 0, hcnt = 0;
  if (tid < ncols) {
    hoff = s_hb[2 * tid] - xa;
    hcnt = s_hb[2 * tid + 1];
  }

  for (int y = ya; y < yb; ++y) {
    const int Y = d.box_top + y;
    // ---- raw: this row's luma and the chroma rows its upsampling reads ----
#pragma unroll 1
    for (int k = tid; k < ychunks; k += kRagThreads)
      *reinterpret_cast<uint2 *>(s_y + 8 * k) = load8(py + (int64_t)Y * d.plane_stride[0] + 8 * k);
    int lo[2] = {0, 0};
    if (color != 2) {
#pragma unroll
      for (int c = 1; c <= 2; ++c) {
        const int vf = d.vf[c], dh = d.cdh[c], cy = Y / vf;
        // h2v2 and h1v2 fancy take the row above an even y and below an odd
        // one; every other ratio reads row cy alone
        const int l = vf == 2 && !(Y & 1) ? max(cy - 1, 0) : cy;
        const int h = vf == 2 && (Y & 1) ? min(cy + 1, dh - 1) : cy;
        lo[c - 1] = l;
        ld.cdh[c] = dh - l;
        const int r = tid >> 7; // 128 lanes a row
        const uint8_t *pc = planes + d.plane_off[c] + ca[c - 1] + (int64_t)(l + r) * d.plane_stride[c];
        uint8_t *dst = smem + L.c + (2 * (c - 1) + r) * pitch;
        if (l + r <= h)
#pragma unroll 1
          for (int k = tid & 127; k < cchunks[c - 1]; k += 128) *reinterpret_cast<uint2 *>(dst + 8 * k) = load8(pc + 8 * k);
      }
    }
    __syncthreads(); // the loads are in; every lane is past the taps of the row before
    // ---- rgb: one lane per staged column ----
#pragma unroll 1
    for (int x = tid; x < span; x += kRagThreads) {
      const int Yv = s_y[X0 - xa8 + x];
      uint8_t *o = s_rgb + 3 * x;
      if (color == 2) {
        o[0] = o[1] = o[2] = (uint8_t)Yv;
      } else {
        const int cb = chroma_at(ld, vb[0], 1, X0 + x, Y - lo[0] * ld.vf[1]);
        const int cr = chroma_at(ld, vb[1], 2, X0 + x, Y - lo[1] * ld.vf[2]);
        if (color == 1) o[0] = (uint8_t)Yv, o[1] = (uint8_t)cb, o[2] = (uint8_t)cr;
        else ycc_to_rgb(Yv, cb, cr, o);
      }
    }
    __syncthreads();
    // ---- horizontal taps of this lane's column, then the vertical accumulate ----
    if (tid < ncols) {
      int32_t s0 = 1 << (kPrecisionBits - 1), s1 = s0, s2 = s0;
      const int32_t *k = s_kh + tid * ks_h;
      const uint8_t *p = s_rgb + 3 * hoff;
      for (int c = 0; c < hcnt; ++c) {
        const int32_t kw = k[c];
        s0 += (int32_t)p[3 * c] * kw;
        s1 += (int32_t)p[3 * c + 1] * kw;
        s2 += (int32_t)p[3 * c + 2] * kw;
      }
      const int32_t h0 = (int32_t)clip8(s0), h1 = (int32_t)clip8(s1), h2 = (int32_t)clip8(s2);
#pragma unroll
      for (int j = 0; j < TR; ++j) {
        const int jj = y - s_vb[2 * j];
        if (jj >= 0 && jj < s_vb[2 * j + 1]) {
          const int32_t kw = s_kv[j * ks_v + jj];
          acc[j][0] += h0 * kw;
          acc[j][1] += h1 * kw;
          acc[j][2] += h2 * kw;
        }
      }
    }
  }

  // ---- store: steps of four rows, a wave a row, by destination address ----
  const int wave = tid >> 6, lane = tid & 63;
  const bool nhwc = fmt.layout == kLayoutNHWC;
  const int flip = d.flip;
  uint8_t *ob = out + nat_off[img] * es;
  const int ocol0 = flip ? rw - ox0 - ncols : ox0; // the tile's first output column
  const int li = flip ? ncols - 1 - tid : tid;     // this lane's place in the tile's row segment
#pragma unroll
  for (int step = 0; step < TR / 4; ++step) {
    if (4 * step >= nrows) break; // uniform
    if (tid < ncols) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
          s_out[r * 3 * kRagTileCols + (nhwc ? li * 3 + c : c * kRagTileCols + li)] =
              s_lut[c * 256 + clip8(acc[4 * step + r][c])];
    }
    __syncthreads();
    const int oy = oy0 + 4 * step + wave;
    if (4 * step + wave < nrows) {
      const uint32_t *orow = s_out + wave * 3 * kRagTileCols;
      if (nhwc) {
        store_run(ob + (((int64_t)oy * rw + ocol0) * 3) * es, orow, 3 * ncols, es, lane);
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
          store_run(ob + (((int64_t)c * rh + oy) * rw + ocol0) * es, orow + c * kRagTileCols, ncols, es, lane);
      }
    }
    __syncthreads(); // the next step overwrites the row buffers
  }
}

} // namespace

hipError_t launch_resize_ragged(const DevPlan &p, const DevWork &w, float *out, int64_t *out_labels, hipStream_t s,
                                int filter) {
  if (p.nat_tiles_total == 0) return hipSuccess;
  const auto kern = filter == kFilterBicubic ? &k_resize_ragged<kFilterBicubic> : &k_resize_ragged<kFilterBilinear>;
  // up to the full 160 KiB of LDS (wide boxes under a large reduction), once per kernel
  static hipError_t attr[2] = {
      hipFuncSetAttribute(reinterpret_cast<const void *>(&k_resize_ragged<kFilterBilinear>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, kRaggedLdsMax),
      hipFuncSetAttribute(reinterpret_cast<const void *>(&k_resize_ragged<kFilterBicubic>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, kRaggedLdsMax)};
  if (attr[filter == kFilterBicubic] != hipSuccess) return attr[filter == kFilterBicubic];
  const int lds = ragged_lds(p.rag).bytes;
  if (lds > kRaggedLdsMax) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kern, dim3(p.nat_tiles_total), dim3(kRagThreads), lds, s, p.descs, w.planes, w.status,
                     p.nat_tiles, p.nat_off, p.nat_res, p.n, p.lut, p.labels, reinterpret_cast<uint8_t *>(out),
                     out_labels, p.ro.fmt, p.rag);
  return hipGetLastError();
}

} // namespace ldt
