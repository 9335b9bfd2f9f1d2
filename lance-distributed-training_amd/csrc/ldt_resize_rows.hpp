// ldt_resize_rows.hpp — the per-source-row body of the ragged resizes as a
// device function: k_resize_ragged's loop (ldt_resize_ragged.hip has the
// account of it), taken out so that a kernel with another index map can run
// it. k_resize_tiles (ldt_resize_tiles.hip) does; k_resize_ragged and
// k_resize_patches still carry their own copies.
//
// The caller has, in the LDS laid out by L (RaggedLds): every lane's horizontal
// coefficients at `kh` with its window (hoff columns into the span, hcnt taps;
// hcnt == 0 and live == false for a lane with no column), rows' windows in
// s_vb (ymin, count; count 0 for a row that takes nothing) and coefficients in
// s_kv (ks_v apart), and the staged span [xa, xa + span) of the box's columns,
// span <= the span L was laid out for. resize_rows walks source rows
// [ya, yb) of the box: per row the span's luma and chroma bytes in aligned
// 8-byte loads, chroma_at / ycc_to_rgb once per staged pixel, this lane's
// horizontal taps to a clip8 byte, and the vertical taps of its TR output rows
// into acc (which the caller initialised to the rounding term). Two barriers
// per source row; every lane of the workgroup must call it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ldt_device.hpp"
#include "ldt_kernels.hpp"

namespace ldt {

template <int TR, int THREADS>
__device__ __forceinline__ void resize_rows(const ImgDesc &d, const uint8_t *__restrict__ planes, uint8_t *smem,
                                            const RaggedLds &L, int pitch, int xa, int span, int ya, int yb, bool live,
                                            int hoff, int hcnt, const int32_t *kh, int ks_v, int32_t (&acc)[TR][3]) {
  const int tid = threadIdx.x;
  const int32_t *s_vb = reinterpret_cast<const int32_t *>(smem + L.vb);
  const int32_t *s_kv = reinterpret_cast<const int32_t *>(smem + L.kv);
  uint8_t *s_y = smem + L.y;
  uint8_t *s_rgb = smem + L.rgb;
  // ---- the span in the image, and what of each plane holds it ----
  const int X0 = d.box_left + xa, xa8 = X0 & ~7;
  const int ychunks = (X0 + span - xa8 + 7) >> 3; // 8 * ychunks <= span + 14 <= pitch; ends inside the stride
  const uint8_t *py = planes + d.plane_off[0] + xa8;
  const int color = d.color;
  // chroma_at's view of a component's staged rows: the fields it reads, the
  // LDS pitch as the stride, rows counted from the region's first
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
  // the regions moved back by their first column (below LDT_MAX_DIM <= L.c)
  const uint8_t *vb[2] = {smem + (L.c - ca[0]), smem + (L.c + 2 * pitch - ca[1])};

  for (int y = ya; y < yb; ++y) {
    const int Y = d.box_top + y;
    // ---- raw: this row's luma and the chroma rows its upsampling reads ----
#pragma unroll 1
    for (int k = tid; k < ychunks; k += THREADS)
      *reinterpret_cast<uint2 *>(s_y + 8 * k) =
          *reinterpret_cast<const uint2 *>(py + (int64_t)Y * d.plane_stride[0] + 8 * k);
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
        const int r = tid / (THREADS / 2); // half the lanes a row
        const uint8_t *pc = planes + d.plane_off[c] + ca[c - 1] + (int64_t)(l + r) * d.plane_stride[c];
        uint8_t *dst = smem + L.c + (2 * (c - 1) + r) * pitch;
        if (l + r <= h)
#pragma unroll 1
          for (int k = tid % (THREADS / 2); k < cchunks[c - 1]; k += THREADS / 2)
            *reinterpret_cast<uint2 *>(dst + 8 * k) = *reinterpret_cast<const uint2 *>(pc + 8 * k);
      }
    }
    __syncthreads(); // the loads are in; every lane is past the taps of the row before
    // ---- rgb: one lane per staged column ----
#pragma unroll 1
    for (int x = tid; x < span; x += THREADS) {
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
    if (live) {
      int32_t s0 = 1 << (kPrecisionBits - 1), s1 = s0, s2 = s0;
      const uint8_t *p = s_rgb + 3 * hoff;
      for (int c = 0; c < hcnt; ++c) {
        const int32_t kw = kh[c];
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
}

} // namespace ldt
