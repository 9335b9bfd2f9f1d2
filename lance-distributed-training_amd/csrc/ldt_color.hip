// ldt_color.hip — the photometric stage of a call with colours
// (ldt_set_colors): ColorJitter, RandomGrayscale and RandomSolarize per output
// image, on the resized uint8 image, then ToTensor / Normalize and the store in
// the call's dtype and layout. The arithmetic is ldt_color.hpp's, which the CPU
// check holds against Pillow itself.
//
// The resize of such a call runs as it does for a uint8 contiguous output and
// writes its Pillow-exact bytes into a workspace laid out like that output
// (view-major, dense planes whose rows are `w` bytes, not padded). Two
// streaming kernels with no reuse follow on the same stream:
//
//   k_color_mean   launched only when some entry has contrast. For those output
//                  images it applies the ops that precede contrast in the
//                  entry's order and sums L over the image: per lane, then a
//                  wave reduction, then one 32-bit atomic add per wave into the
//                  image's counter (zeroed on the stream beforehand). The sum
//                  is at most 255 * 2^20 and integer adds commute, so the
//                  result does not depend on the order of arrival.
//   k_color_apply  runs every entry's chain with the mean from the first pass
//                  and stores through the 768-entry ToTensor / Normalize table
//                  and the formatted-store helpers of the resize kernels, so
//                  every dtype, channels_last, Normalize, views and size lists
//                  work as they do there. An entry with nothing present is a
//                  plain table store.
//
//   k_color_blur   launched only when some entry has a blur (blur_ww != 0),
//                  Pillow's GaussianBlur between grayscale and solarize; it
//                  serves those entries and k_color_apply leaves them alone.
//                  One workgroup per (output image, tile of kBlurTileH x
//                  kBlurTileW pixels): the tile and a halo of 3 * (r + 1)
//                  pixels go from the workspace through the chain up to
//                  grayscale into LDS, the three row passes and three column
//                  passes (ldt_blur.hpp) ping-pong between two LDS buffers, and
//                  the tile goes through solarize, the table and the same
//                  formatted store. No pass touches device memory.
//
// The first two: one workgroup per (output image, tile of kColorRows rows); a lane takes
// four consecutive pixels of a row, one dword from each of the three planes
// when the row's address allows it (w a multiple of 4, or a row that happens to
// start aligned), single bytes at a tail or an unaligned row. The geometry of
// a workgroup's view comes from ColorGeom, a kernel argument: finding the view
// is a walk over at most 16 scalars, uniform over the workgroup. Rows whose
// status is not 0 are skipped: launch_fill_failed* zeroes them afterwards.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ldt_blur.hpp"
#include "ldt_color.hpp"
#include "ldt_color_dev.hpp"
#include "ldt_device.hpp"
#include "ldt_kernels.hpp"

#pragma clang fp contract(off)

namespace ldt {

namespace {

__global__ void __launch_bounds__(kColorThreads)
    k_color_mean(const ldt_color *__restrict__ colors, const uint8_t *__restrict__ ws, uint32_t *__restrict__ sums,
                 const int32_t *__restrict__ status, int n, const ColorGeom g) {
  const ColorWork k = color_work(g, blockIdx.x, n);
  if (k.img >= n || status[k.img] != 0) return;
  const int entry = k.img * g.views + k.view;
  const ldt_color c = colors[entry];
  if (!color_has_contrast(c)) return;
  const int Q = (k.ow + 3) >> 2; // quads per row
  const int64_t plane = (int64_t)k.oh * k.ow;
  uint32_t sum = 0;
  for (int idx = threadIdx.x; idx < k.rows * Q; idx += kColorThreads) {
    const int row = idx / Q, x = (idx - row * Q) * 4;
    const int cnt = min(4, k.ow - x);
    const uint8_t *p = ws + k.base + (int64_t)(k.y0 + row) * k.ow + x;
    const uint32_t qr = load_quad(p, cnt), qg = load_quad(p + plane, cnt), qb = load_quad(p + 2 * plane, cnt);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < cnt) {
        int r = (qr >> (8 * e)) & 255, gg = (qg >> (8 * e)) & 255, b = (qb >> (8 * e)) & 255;
        color_before_contrast(c, r, gg, b);
        sum += (uint32_t)color_l(r, gg, b);
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
  if ((threadIdx.x & 63) == 0 && sum != 0) atomicAdd(&sums[entry], sum);
}

__global__ void __launch_bounds__(kColorThreads)
    k_color_apply(const ldt_color *__restrict__ colors, const uint8_t *__restrict__ ws,
                  const uint32_t *__restrict__ sums, const int32_t *__restrict__ status,
                  const float *__restrict__ lut, uint8_t *__restrict__ out, OutFmt fmt, int n, const ColorGeom g) {
  __shared__ uint32_t s_bits[768]; // the table as element bits, as the resize kernels' FMT instantiations hold it
  const ColorWork k = color_work(g, blockIdx.x, n);
  if (k.img >= n || status[k.img] != 0) return;
  const int es = dtype_bytes(fmt.dtype);
  for (int i = threadIdx.x; i < 768; i += kColorThreads)
    s_bits[i] = es == 4   ? reinterpret_cast<const uint32_t *>(lut)[i]
                : es == 2 ? (uint32_t) reinterpret_cast<const uint16_t *>(lut)[i]
                          : (uint32_t)(i & 255);
  const int entry = k.img * g.views + k.view;
  const ldt_color c = colors[entry];
  if (c.blur_ww != 0) return; // k_color_blur's (the whole workgroup: no barrier is left waiting)
  const int mean = color_has_contrast(c) ? color_mean_round(sums[entry], (uint32_t)(k.oh * k.ow)) : 0;
  const bool plain = color_is_identity(c);
  __syncthreads();
  const int Q = (k.ow + 3) >> 2;
  const int64_t plane = (int64_t)k.oh * k.ow;
  uint8_t *ob = out + k.base * es; // the image's first element
  for (int idx = threadIdx.x; idx < k.rows * Q; idx += kColorThreads) {
    const int row = idx / Q, x = (idx - row * Q) * 4;
    const int cnt = min(4, k.ow - x);
    const int64_t at = (int64_t)(k.y0 + row) * k.ow + x; // the quad's first pixel in a plane
    const uint8_t *p = ws + k.base + at;
    const uint32_t qr = load_quad(p, cnt), qg = load_quad(p + plane, cnt), qb = load_quad(p + 2 * plane, cnt);
    uint32_t v[3][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int r = (qr >> (8 * e)) & 255, gg = (qg >> (8 * e)) & 255, b = (qb >> (8 * e)) & 255;
      if (!plain) color_chain(c, mean, r, gg, b);
      v[0][e] = s_bits[r];
      v[1][e] = s_bits[256 + gg];
      v[2][e] = s_bits[512 + b];
    }
    store_quad(ob, fmt, es, plane, at, cnt, v);
  }
}

// floor(i / d) for 0 <= i < 2^15, 1 <= d < 2^7 and a quotient below 2^9, without
// an integer division: (i + 0.5) * (1 / d) is off by at most 2^9 * 2^-22 from
// the real quotient of i + 0.5, which lies at least 1 / (2 d) > 2^-8 from every
// integer.
__device__ __forceinline__ int div_small(int i, float inv_d) { return (int)(((float)i + 0.5f) * inv_d); }

// One blur pass over three planes of `len` lines of `pq` dwords each (plane,
// line, dword), along the lines' index: a lane per dword, the four bytes of a
// dword being four independent columns of the pass, summed as two pairs of
// 16-bit sums (at most 15 * 255 each). Lines are clamped to 0..len-1. TR: the
// result goes to the other layout, byte (plane, 4 * q + e, line) of planes of
// out_lines lines of out_pitch bytes, for the 4 * q + e below out_lines.
template <bool TR>
__device__ __forceinline__ void blur_pass4(const uint8_t *src, uint8_t *dst, int len, int pq, int r, uint32_t ww,
                                           uint32_t fw, int out_lines, int out_pitch) {
  const uint32_t *s32 = reinterpret_cast<const uint32_t *>(src);
  const float inv_pq = 1.0f / (float)pq;
  for (int i = threadIdx.x; i < 3 * len * pq; i += kColorThreads) {
    const int line = div_small(i, inv_pq), q = i - line * pq; // line: plane * len + position
    const int ch = (line >= len) + (line >= 2 * len), pos = line - ch * len;
    const uint32_t *col = s32 + ch * len * pq + q;
    uint32_t lo = 0, hi = 0;
    for (int k = -r; k <= r; ++k) {
      const uint32_t d = col[min(max(pos + k, 0), len - 1) * pq];
      lo += d & 0x00FF00FFu;
      hi += (d >> 8) & 0x00FF00FFu;
    }
    const uint32_t d0 = col[max(pos - r - 1, 0) * pq], d1 = col[min(pos + r + 1, len - 1) * pq];
    const uint32_t elo = (d0 & 0x00FF00FFu) + (d1 & 0x00FF00FFu);
    const uint32_t ehi = ((d0 >> 8) & 0x00FF00FFu) + ((d1 >> 8) & 0x00FF00FFu);
    const uint32_t b0 = blur_tap(lo & 0xFFFFu, elo & 0xFFFFu, ww, fw), b1 = blur_tap(hi & 0xFFFFu, ehi & 0xFFFFu, ww, fw);
    const uint32_t b2 = blur_tap(lo >> 16, elo >> 16, ww, fw), b3 = blur_tap(hi >> 16, ehi >> 16, ww, fw);
    if (TR) {
      uint8_t *o = dst + (ch * out_lines + 4 * q) * out_pitch + pos;
      const int left = out_lines - 4 * q;
      o[0] = (uint8_t)b0; // 4 * q < out_lines: pq covers out_lines rounded up to 4
      if (left > 1) o[out_pitch] = (uint8_t)b1;
      if (left > 2) o[2 * out_pitch] = (uint8_t)b2;
      if (left > 3) o[3 * out_pitch] = (uint8_t)b3;
    } else {
      reinterpret_cast<uint32_t *>(dst)[line * pq + q] = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
    }
  }
}

__global__ void __launch_bounds__(kColorThreads)
    k_color_blur(const ldt_color *__restrict__ colors, const uint8_t *__restrict__ ws,
                 const uint32_t *__restrict__ sums, const int32_t *__restrict__ status,
                 const float *__restrict__ lut, uint8_t *__restrict__ out, OutFmt fmt, int n, const BlurGeom g) {
  extern __shared__ __align__(16) uint8_t s_px[]; // two buffers of three planes of the tile and its halo
  __shared__ uint32_t s_bits[768];
  const int img = blockIdx.x / g.tiles;
  if (img >= n || status[img] != 0) return;
  const int t = blockIdx.x - img * g.tiles;
  int view = 0;
#pragma unroll
  for (int u = 1; u < kMaxViews; ++u)
    if (u < g.views && t >= g.tile0[u]) view = u;
  const int entry = img * g.views + view;
  const ldt_color c = colors[entry];
  if (c.blur_ww == 0) return; // k_color_apply's
  const int oh = g.oh[view], ow = g.ow[view];
  const int tl = t - g.tile0[view];
  const int tile_y = tl / g.tiles_x[view], tile_x = tl - tile_y * g.tiles_x[view];
  const int es = dtype_bytes(fmt.dtype);
  for (int i = threadIdx.x; i < 768; i += kColorThreads)
    s_bits[i] = es == 4   ? reinterpret_cast<const uint32_t *>(lut)[i]
                : es == 2 ? (uint32_t) reinterpret_cast<const uint16_t *>(lut)[i]
                          : (uint32_t)(i & 255);
  const int mean = color_has_contrast(c) ? color_mean_round(sums[entry], (uint32_t)(oh * ow)) : 0;
  const int r = min((int)c.blur_r, kBlurMaxR); // ldt_set_colors lets no larger one in
  const uint32_t ww = c.blur_ww, fw = blur_fw(r, ww);
  const int halo = 3 * (r + 1);
  // the tile, and the region its blur reads: the halo clipped to the image, so
  // that a region edge that is no image edge lies `halo` pixels from the tile.
  // Every pass runs over the whole region and clamps at the region's edges:
  // what a wrong clamp spoils grows by r + 1 pixels per pass and stops at the
  // tile's edge after three.
  const int ty0 = tile_y * kBlurTileH, tx0 = tile_x * kBlurTileW;
  const int th = min(kBlurTileH, oh - ty0), tw = min(kBlurTileW, ow - tx0);
  const int ry0 = max(0, ty0 - halo), rx0 = max(0, tx0 - halo);
  const int RH = min(oh, ty0 + th + halo) - ry0, RW = min(ow, tx0 + tw + halo) - rx0;
  // Two layouts in LDS, both of whole dwords per line so that a pass handles
  // four lines' bytes at once: "columns" (plane, x, y: a dword holds four rows
  // of one column) for the passes along the rows, "rows" (plane, y, x) for the
  // passes along the columns. The bytes of a line past its end are computed
  // from whatever lies there and never read for a result.
  const int P = (RW + 3) & ~3, PT = (RH + 3) & ~3; // a line's bytes: rows layout, columns layout
  const int PS = RH * P, PST = RW * PT;            // a plane's
  uint8_t *bufA = s_px, *bufB = s_px + 3 * max(PS, PST);
  const float inv_rw = 1.0f / (float)RW;
  const int64_t plane = (int64_t)oh * ow;
  const int64_t base = g.base[view] + (int64_t)img * 3 * plane;

  // load: the resized bytes through the chain up to grayscale, lanes along the
  // image's rows, into the columns layout
  for (int i = threadIdx.x; i < RH * RW; i += kColorThreads) {
    const int y = div_small(i, inv_rw), x = i - y * RW;
    const uint8_t *p = ws + base + (int64_t)(ry0 + y) * ow + (rx0 + x);
    int rr = p[0], gg = p[plane], bb = p[2 * plane];
    color_chain_head(c, mean, rr, gg, bb);
    uint8_t *q = bufA + x * PT + y;
    q[0] = (uint8_t)rr;
    q[PST] = (uint8_t)gg;
    q[2 * PST] = (uint8_t)bb;
  }
  __syncthreads();
  // three passes along the rows; the third stores into the rows layout
  blur_pass4<false>(bufA, bufB, RW, PT >> 2, r, ww, fw, 0, 0);
  __syncthreads();
  blur_pass4<false>(bufB, bufA, RW, PT >> 2, r, ww, fw, 0, 0);
  __syncthreads();
  blur_pass4<true>(bufA, bufB, RW, PT >> 2, r, ww, fw, RH, P);
  __syncthreads();
  // three along the columns
  blur_pass4<false>(bufB, bufA, RH, P >> 2, r, ww, fw, 0, 0);
  __syncthreads();
  blur_pass4<false>(bufA, bufB, RH, P >> 2, r, ww, fw, 0, 0);
  __syncthreads();
  blur_pass4<false>(bufB, bufA, RH, P >> 2, r, ww, fw, 0, 0);
  __syncthreads();
  const uint8_t *src = bufA;
  // the tile: solarize, the table, the store (src is bufA again after six passes)
  const int Q = (tw + 3) >> 2;
  uint8_t *ob = out + base * es;
  for (int idx = threadIdx.x; idx < th * Q; idx += kColorThreads) {
    const int row = idx / Q, x = (idx - row * Q) * 4;
    const int cnt = min(4, tw - x);
    const int64_t at = (int64_t)(ty0 + row) * ow + (tx0 + x);
    const uint8_t *p = src + (ty0 + row - ry0) * P + (tx0 + x - rx0);
    uint32_t v[3][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      // past the row's end: a byte of the row's padding or of the next row, inside the buffer, not stored
      int rr = p[e], gg = p[PS + e], bb = p[2 * PS + e];
      color_chain_tail(c, rr, gg, bb);
      v[0][e] = s_bits[rr];
      v[1][e] = s_bits[256 + gg];
      v[2][e] = s_bits[512 + bb];
    }
    store_quad(ob, fmt, es, plane, at, cnt, v);
  }
}

} // namespace

hipError_t launch_color_mean(const ldt_color *colors, const uint8_t *ws, uint32_t *sums, const int32_t *status,
                             int n, const ColorGeom &g, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (g.views < 1 || g.tiles < 1 || (int64_t)n * g.tiles > 0x7FFFFFFF) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_color_mean, dim3((unsigned)(n * g.tiles)), dim3(kColorThreads), 0, s, colors, ws, sums, status,
                     n, g);
  return hipGetLastError();
}

hipError_t launch_color_apply(const ldt_color *colors, const uint8_t *ws, const uint32_t *sums,
                              const int32_t *status, const float *lut, float *out, OutFmt fmt, int n,
                              const ColorGeom &g, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (g.views < 1 || g.tiles < 1 || (int64_t)n * g.tiles > 0x7FFFFFFF) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_color_apply, dim3((unsigned)(n * g.tiles)), dim3(kColorThreads), 0, s, colors, ws, sums,
                     status, lut, reinterpret_cast<uint8_t *>(out), fmt, n, g);
  return hipGetLastError();
}

hipError_t launch_color_blur(const ldt_color *colors, const uint8_t *ws, const uint32_t *sums,
                             const int32_t *status, const float *lut, float *out, OutFmt fmt, int n,
                             const BlurGeom &g, int max_r, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (g.views < 1 || g.tiles < 1 || (int64_t)n * g.tiles > 0x7FFFFFFF || max_r < 0 || max_r > kBlurMaxR)
    return hipErrorInvalidValue;
  // two buffers of three planes of the largest region, each side rounded up to
  // whole dwords (either layout fits): 53,776 bytes at r = 7 (beside the
  // table's 3 KiB, inside the 64 KiB a launch may ask for without more ado),
  // 20,080 at r <= 1, where seven workgroups share a CU's LDS
  const int halo = 3 * (max_r + 1);
  const size_t lds = 2 * 3 * (size_t)((kBlurTileH + 2 * halo + 3) & ~3) * (size_t)((kBlurTileW + 2 * halo + 3) & ~3) + 16;
  hipLaunchKernelGGL(k_color_blur, dim3((unsigned)(n * g.tiles)), dim3(kColorThreads), lds, s, colors, ws, sums,
                     status, lut, reinterpret_cast<uint8_t *>(out), fmt, n, g);
  return hipGetLastError();
}

} // namespace ldt
