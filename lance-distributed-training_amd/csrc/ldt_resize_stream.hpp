// ldt_resize_stream.hpp — what one workgroup of the streaming resize does once
// it knows its tile: the one device body of k_resize and k_resize_views
// (ldt_resize_stream.hip, which says how each kernel finds the tile and what
// the BOX, FILT, FMT and SIZED variants mean). Device code only.
//
// Each thread below the tile's width owns one output column: it computes the
// horizontal tap sum of every needed source row and accumulates the vertical
// taps in registers, so the uint8 value between the passes (Pillow's
// intermediate image) never leaves the thread. The tap sums are signed int32
// and both passes clamp with the signed clip8, so BICUBIC's negative weights
// and its overshoot need no other code: FILT only chooses the coefficients.
//
// Nothing here asks which kernel called it. What differs between the callers
// is a template parameter (SRC, FILT, FMT) or a field of StreamTile; a field
// the caller sets to a constant (a call without boxes: top, left and flip 0,
// without windows: res = the output size, origin 0) is that constant after
// inlining, so such a call compiles no box or window code in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ldt_device.hpp"

namespace ldt {

// The format a kernel's trailing argument pack carries: only the FMT
// instantiations have one (F = OutFmt; the pack is empty otherwise).
__device__ __forceinline__ OutFmt fmt_arg() { return OutFmt(); }
__device__ __forceinline__ OutFmt fmt_arg(OutFmt f) { return f; }

// One workgroup's work: kBandRows output rows (the last band of an image may
// hold fewer) by one tile of up to kTileCols output columns of one output image.
struct StreamTile {
  int img;                 // the source image: the row of the batch
  // SRC 0: the image's descriptor and the batch's planes. SRC 1: the batch's
  // raw HWC cells, the bytes from one cell to the next and a cell's width in
  // pixels; the body forms cell `img`'s address where it stages a row (formed
  // once ahead of the row loop it costs the raw FMT kernels 24 VGPRs and a
  // wave of occupancy)
  const ImgDesc *desc;
  const uint8_t *src;
  int64_t src_stride;
  int src_w;
  int W, H;                // the source of the resize: the box, or the whole image
  int top, left, flip;     // the box's origin in the image; the output row is mirrored
  int rh, rw, wtop, wleft; // the size the source is resized to, the output window's origin in it
  int oh, ow;              // the output image's size
  int band, tile;
  // the batch's labels, or null when this workgroup's kernel or view writes
  // none: the workgroup of band 0, tile 0 copies labels[img] to out_labels[img]
  const int64_t *labels;
  int64_t *out_labels;
  int64_t oimg, obase;     // the output image's index in the dense block that starts at element obase
};

// ---- stage one source row as interleaved RGB in LDS ----
// From planes: row top + y of the image, columns left .. left + W. Gray is
// replicated, RGB passes through, YCbCr is converted; chroma_at gets the
// image's absolute coordinates, so the fancy upsampling's edge rules stay
// those of the whole image whatever the box.
__device__ __forceinline__ void stage_row_planes(const ImgDesc &d, const uint8_t *planes, int top, int left, int W,
                                                 int y, uint8_t *row, int tid) {
  const uint8_t *py = planes + d.plane_off[0] + (int64_t)(top + y) * d.plane_stride[0] + left;
  if (d.color == 2) {
    for (int x = tid; x < W; x += kResizeThreads) {
      const uint8_t v = py[x];
      row[3 * x] = v;
      row[3 * x + 1] = v;
      row[3 * x + 2] = v;
    }
  } else {
    const uint8_t *pcb = planes + d.plane_off[1];
    const uint8_t *pcr = planes + d.plane_off[2];
    for (int x = tid; x < W; x += kResizeThreads) {
      const int Y = py[x];
      const int cb = chroma_at(d, pcb, 1, left + x, top + y);
      const int cr = chroma_at(d, pcr, 2, left + x, top + y);
      if (d.color == 1) {
        row[3 * x] = (uint8_t)Y;
        row[3 * x + 1] = (uint8_t)cb;
        row[3 * x + 2] = (uint8_t)cr;
      } else {
        ycc_to_rgb(Y, cb, cr, row + 3 * x);
      }
    }
  }
}

// From raw HWC: the W columns from `left` of row top + y of a cell src_w pixels
// wide. A start or a length that breaks the 4-byte alignment (an odd box)
// takes the byte copy.
__device__ __forceinline__ void stage_row_hwc(const uint8_t *cell, int src_w, int top, int left, int W, int y,
                                              uint8_t *row, int tid) {
  const uint8_t *src = cell + ((int64_t)(top + y) * src_w + left) * 3;
  const int nbytes = W * 3;
  if ((((uintptr_t)src) & 3) == 0 && (nbytes & 3) == 0) {
    const uint32_t *s4 = reinterpret_cast<const uint32_t *>(src);
    uint32_t *r4 = reinterpret_cast<uint32_t *>(row);
    for (int i = tid; i < nbytes / 4; i += kResizeThreads) r4[i] = s4[i];
  } else {
    for (int i = tid; i < nbytes; i += kResizeThreads) row[i] = src[i];
  }
}

// The tile. lut: the launch's 768-entry table, float32, or in the form
// write_plan emits for fmt.dtype (FMT). ks_h / ks_v: the tap capacity of the
// LDS coefficient rows, at least that of any (W -> rw) / (H -> rh) of the
// launch; row_bytes: one staged row, at least 3 * W rounded up to 16. The LDS
// layout (stream_lds_bytes on the host) is sized by min(ow, kTileCols) columns.
template <int SRC, int FILT, bool FMT>
__device__ __forceinline__ void resize_stream_tile(const StreamTile &t, const float *__restrict__ lut,
                                                   float *__restrict__ out, OutFmt fmt, int ks_h, int ks_v,
                                                   int row_bytes) {
  static_assert(kResizeThreads == kTileCols, "one thread per column of a tile");
  const int tid = threadIdx.x;
  const int W = t.W, H = t.H, oh = t.oh, ow = t.ow;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  float *s_lut = reinterpret_cast<float *>(smem);                 // 768 floats
  const int tcols = min(ow, kTileCols);                           // columns of a full tile
  int32_t *s_kh = reinterpret_cast<int32_t *>(smem + 3072);       // tcols * ks_h
  int32_t *s_kv = s_kh + tcols * ks_h;                            // kBandRows * ks_v
  int32_t *s_hb = s_kv + kBandRows * ks_v;                        // tcols * 2
  int32_t *s_vb = s_hb + 2 * tcols;                               // kBandRows * 2
  uint8_t *s_row = reinterpret_cast<uint8_t *>(s_vb + 2 * kBandRows); // 2 * row_bytes

  // FMT: the table holds the output element's bits (float32, the host-rounded
  // 16-bit table widened to dwords, or the byte itself for uint8)
  const int es = FMT ? dtype_bytes(fmt.dtype) : 4; // bytes per element
  if constexpr (FMT) {
    uint32_t *sb = reinterpret_cast<uint32_t *>(smem);
    for (int i = tid; i < 768; i += kResizeThreads)
      sb[i] = es == 4   ? reinterpret_cast<const uint32_t *>(lut)[i]
              : es == 2 ? (uint32_t) reinterpret_cast<const uint16_t *>(lut)[i]
                        : (uint32_t)(i & 255);
  } else {
    for (int i = tid; i < 768; i += kResizeThreads) s_lut[i] = lut[i];
  }
  const int oy0 = t.band * kBandRows, ox0 = t.tile * kTileCols;
  const int nrows = min(kBandRows, oh - oy0); // rows of this band (the last one may be short)
  const int ncols = min(kTileCols, ow - ox0); // columns of this tile
  // Pillow's passes are separable with a uint8 image between them, so output
  // column x takes the coefficients of (W -> rw) at index wleft + x and output
  // row y those of (H -> rh) at wtop + y; the band's source rows follow from
  // the shifted vertical windows.
  if (tid < ncols) {
    int xmin;
    const int cnt = resample_coeffs<FILT>(W, t.rw, t.wleft + ox0 + tid, ks_h, s_kh + tid * ks_h, &xmin);
    s_hb[2 * tid] = xmin;
    s_hb[2 * tid + 1] = cnt;
  }
  // the vertical rows by the last kBandRows threads: idle ones unless the tile
  // is nearly full. Rows past the image get an empty window.
  if (tid >= kResizeThreads - kBandRows) {
    const int j = tid - (kResizeThreads - kBandRows);
    int ymin = 0, cnt = 0;
    if (j < nrows) cnt = resample_coeffs<FILT>(H, t.rh, t.wtop + oy0 + j, ks_v, s_kv + j * ks_v, &ymin);
    s_vb[2 * j] = ymin;
    s_vb[2 * j + 1] = cnt;
  }
  // the label, between the coefficients and the barrier (ahead of the table
  // load the raw FMT kernels take 138 VGPRs instead of 114)
  if (t.band == 0 && t.tile == 0 && tid == 0 && t.labels != nullptr) t.out_labels[t.img] = t.labels[t.img];
  __syncthreads();
  const int ya = s_vb[0];
  const int yb = s_vb[2 * (nrows - 1)] + s_vb[2 * (nrows - 1) + 1];

  int32_t acc[kBandRows][3];
#pragma unroll
  for (int j = 0; j < kBandRows; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 1 << (kPrecisionBits - 1);
  int hxmin = 0, hcnt = 0;
  if (tid < ncols) {
    hxmin = s_hb[2 * tid];
    hcnt = s_hb[2 * tid + 1];
  }

  for (int y = ya; y < yb; ++y) {
    uint8_t *row = s_row + ((y - ya) & 1) * row_bytes;
    if constexpr (SRC == 0) stage_row_planes(*t.desc, t.src, t.top, t.left, W, y, row, tid);
    else stage_row_hwc(t.src + (int64_t)t.img * t.src_stride, t.src_w, t.top, t.left, W, y, row, tid);
    __syncthreads();
    // ---- horizontal taps for column ox0 + tid, then vertical accumulate ----
    if (tid < ncols) {
      int32_t s0 = 1 << (kPrecisionBits - 1), s1 = s0, s2 = s0;
      const int32_t *k = s_kh + tid * ks_h;
      const uint8_t *p = row + 3 * hxmin;
      for (int c = 0; c < hcnt; ++c) {
        const int32_t kw = k[c];
        s0 += (int32_t)p[3 * c] * kw;
        s1 += (int32_t)p[3 * c + 1] * kw;
        s2 += (int32_t)p[3 * c + 2] * kw;
      }
      const int32_t h0 = (int32_t)clip8(s0), h1 = (int32_t)clip8(s1), h2 = (int32_t)clip8(s2);
#pragma unroll
      for (int j = 0; j < kBandRows; ++j) {
        const int jj = y - s_vb[2 * j];
        if (jj >= 0 && jj < s_vb[2 * j + 1]) {
          const int32_t kw = s_kv[j * ks_v + jj];
          acc[j][0] += h0 * kw;
          acc[j][1] += h1 * kw;
          acc[j][2] += h2 * kw;
        }
      }
    }
    // the next iteration writes the other row buffer; one barrier per row suffices
  }
  if (tid >= ncols) return;
  const int ox = t.flip ? ow - 1 - (ox0 + tid) : ox0 + tid; // a flipped image stores column x at ow - 1 - x
  if constexpr (FMT) {
    // fmt.dtype / fmt.layout are uniform over the launch: one element per
    // channel at the CHW address, or the pixel's three consecutive elements in
    // HWC, mirrored per pixel when flipped
    const uint32_t *s_bits = reinterpret_cast<const uint32_t *>(smem);
    uint8_t *ob = reinterpret_cast<uint8_t *>(out) + t.obase * es;
#pragma unroll
    for (int j = 0; j < kBandRows; ++j) {
      const int oy = oy0 + j;
      if (j < nrows) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int64_t e = fmt.layout == kLayoutNHWC ? ((t.oimg * oh + oy) * ow + ox) * 3 + c
                                                      : ((t.oimg * 3 + c) * oh + oy) * ow + ox;
          fmt_store1(ob + e * es, es, s_bits[c * 256 + clip8(acc[j][c])]);
        }
      }
    }
  } else {
    float *o = out + t.obase + t.oimg * 3 * oh * ow;
#pragma unroll
    for (int j = 0; j < kBandRows; ++j) {
      const int oy = oy0 + j;
      if (j < nrows) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[((int64_t)c * oh + oy) * ow + ox] = s_lut[c * 256 + clip8(acc[j][c])];
      }
    }
  }
}

} // namespace ldt
