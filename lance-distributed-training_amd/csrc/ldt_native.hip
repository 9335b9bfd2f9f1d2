// ldt_native.hip — the store of a native call (ldt_set_native): every good
// row's source rectangle at full resolution, Pillow's
// Image.open(b).convert("RGB") (after a draft and a crop when the call has
// them), in the call's dtype and layout, at the row's own offset of a ragged
// output. It takes the place of the resize launch; everything before it (H2D,
// destuff, Huffman, progressive, IDCT) is what every other call launches.
//
// k_emit_rgb. One workgroup of 256 lanes serves one tile of kNatTileRows x
// kNatTileCols (16 x 256) pixels of one image's rectangle; the tiles of all
// images sit in one grid, and a workgroup finds its image with a uniform
// binary search over the plan's tile prefix (int32 [n + 1]: O(n) bytes of plan
// whatever the images' sizes, where a tile-to-image table would add 4 bytes
// per tile to every call's H2D copy; the search is at most 17 scalar loads of
// a cache-resident array).
//
// Staging. The planes are read once, with 8-byte loads (planes start
// 256-aligned and their strides are multiples of kPlaneStrideAlign = 8, so a
// row's 8-byte chunks are aligned whatever the box's origin): the tile's luma
// rows from the chunk that holds its first column, and per chroma component
// the rows and columns the tile touches plus one sample of halo on each side,
// clipped to cdw / cdh. What chroma_at clamps, it clamps on LDS indices here:
// the arithmetic is chroma_at itself (ldt_device.hpp), handed a descriptor
// whose plane stride is the LDS pitch, a y counted from the region's first row
// and a base moved back by its first column, so every ratio, the cdw <= 2 exceptions and nofancy are its code,
// reading LDS in place of four to eight scattered global bytes per pixel.
// h2v2 fancy, the common case, goes one step further: each chroma sample's
// vertical sum 3 * r0 + r1 is computed once per (output row, chroma column)
// into LDS, and a lane reads the four sums its four pixels share (each sum
// serves two pixels as `thiscol` and two as `nextcol`). The phase x & 1, y & 1
// is that of the image's absolute coordinates, so a box at an odd origin
// shifts which sums a lane takes, not their values.
//
// Work split. A step is 4 rows, one per wave; a lane owns 4 consecutive pixels
// of its wave's row, converts them (ycc_to_rgb, RGB passthrough, grey
// replicated), looks the element bits up in the call's 768-entry table (copied
// to LDS once per workgroup) and puts them into the wave's row buffer in LDS in
// output order: channel-planar under NCHW, interleaved under NHWC, mirrored
// when the row is flipped. 4 steps make the tile.
//
// Store. An output row starts at any alignment (w is any value and the offsets
// are the caller's), and under NCHW the three channel planes of one image have
// three different ones, so no lane-to-pixel mapping is aligned for all three.
// The wave therefore stores from its row buffer by destination address, not by
// pixel: per run of consecutive elements (a channel's row segment under NCHW,
// the whole 3 * ncols segment under NHWC) the elements up to the first
// 4-element boundary and after the last go as element stores, everything
// between as one 4-element vector per lane (16, 8 or 4 bytes). A failed row is
// not touched here: k_native_fill zeroes its whole region, whatever its length,
// and sets its label to -100.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ldt_device.hpp"
#include "ldt_kernels.hpp"

namespace ldt {
namespace {

constexpr int kEmitThreads = 256;
static_assert(kNatTileCols == kEmitThreads && kNatTileRows == 16, "4 steps of 4 waves, 4 pixels a lane");
// Bytes per staged plane row: 256 columns, a halo sample on each side and up
// to 7 bytes before the first column (the 8-byte chunk it lies in) are at most
// 34 chunks.
constexpr int kPitch = 272;
constexpr int kChromaRows = kNatTileRows + 2;
// uint16 per row of h2v2 sums: 128 chroma columns, one more when the tile
// starts at an odd x, a halo sample on each side (131); a lane past the tile's
// last column reads inside the row too (index 129 at most).
constexpr int kSumPitch = 136;
constexpr int kFillSplit = 8; // workgroups per failed row's region

struct EmitLds {
  uint32_t lut[768]; // element bits
  uint8_t y[kNatTileRows][kPitch];
  uint32_t out[4][3 * kNatTileCols]; // one row of element bits per wave: written and read by that wave alone
  uint8_t c[2][kChromaRows][kPitch];
  uint16_t sum[2][kNatTileRows][kSumPitch];
};
// chroma_at's plane pointer for a staged region is the region's first byte
// moved back by its first column (below): that stays inside the structure.
static_assert(offsetof(EmitLds, c) >= LDT_MAX_DIM, "a chroma region's base minus its first column lies inside EmitLds");

// What a wave wrote to LDS is visible to its own lanes' later reads: LDS
// operations of one wave complete in order, so only the compiler has to keep
// them in order.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// One chroma component's staged region: chroma rows [cy0, cy0 + rows), columns
// from ca (a multiple of 8) in `chunks` 8-byte chunks.
struct ChromaRegion {
  int ca, cy0, rows, chunks;
};

__device__ __forceinline__ uint2 load8(const uint8_t *p) { return *reinterpret_cast<const uint2 *>(p); }

// store_run, the wave's store of a run of elements by destination address, is
// ldt_device.hpp's: k_resize_ragged stores the same way.

__global__ void __launch_bounds__(kEmitThreads)
    k_emit_rgb(const ImgDesc *__restrict__ descs, const uint8_t *__restrict__ planes,
               const int32_t *__restrict__ status, const int32_t *__restrict__ tile_pref,
               const int64_t *__restrict__ nat_off, int n, const float *__restrict__ lut,
               const int64_t *__restrict__ labels, uint8_t *__restrict__ out, int64_t *__restrict__ out_labels,
               OutFmt fmt) {
  __shared__ __attribute__((aligned(16))) EmitLds L;
  const int tid = threadIdx.x, tile = blockIdx.x;
  // the image whose tiles hold this one: tile_pref[img] <= tile < tile_pref[img + 1]
  // (rows without tiles, the host's failed ones, share their neighbour's value
  // and are never found)
  int img = 0;
  for (int hi = n; hi - img > 1;) {
    const int mid = (img + hi) >> 1;
    if (tile_pref[mid] <= tile) img = mid;
    else hi = mid;
  }
  if (status[img] != 0) return;
  const ImgDesc &d = descs[img];
  const int w = d.box_w, h = d.box_h;
  const int t = tile - tile_pref[img];
  const int tiles_x = (w + kNatTileCols - 1) / kNatTileCols;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int bx0 = tx * kNatTileCols, by0 = ty * kNatTileRows; // in the box
  const int ncols = min(kNatTileCols, w - bx0), nrows = min(kNatTileRows, h - by0);
  const int X0 = d.box_left + bx0, Y0 = d.box_top + by0; // in the image
  if (t == 0 && tid == 0 && labels != nullptr) out_labels[img] = labels[img];

  const int es = dtype_bytes(fmt.dtype);
  for (int i = tid; i < 768; i += kEmitThreads)
    L.lut[i] = es == 4   ? reinterpret_cast<const uint32_t *>(lut)[i]
               : es == 2 ? (uint32_t) reinterpret_cast<const uint16_t *>(lut)[i]
                         : (uint32_t)(i & 255);

  // ---- stage: 16 lanes a row, 8 bytes a lane ----
  const int srow = tid >> 4, scol = tid & 15;
  const int xa = X0 & ~7;
  {
    const int chunks = (X0 + ncols - xa + 7) >> 3; // at most 33; the last one ends inside the stride
    const uint8_t *py = planes + d.plane_off[0] + xa;
    if (srow < nrows)
#pragma unroll 1
      for (int k = scol; k < chunks; k += 16) // at most 3 trips: kept a loop
        *reinterpret_cast<uint2 *>(&L.y[srow][8 * k]) = load8(py + (int64_t)(Y0 + srow) * d.plane_stride[0] + 8 * k);
  }
  const int color = d.color;
  ChromaRegion cr[2] = {};
  bool fancy22[2] = {false, false};
  // chroma_at's view of the staged regions: the fields it reads, the LDS pitch
  // as the plane stride, rows counted from the region's first (cdh and the y
  // handed to it are moved by cy0, a whole number of chroma rows, so y's phase,
  // y / vf and both row clamps mean what they meant: the row before the first
  // staged one is never asked for unless the first is row 0)
  ImgDesc ld;
  ld.nofancy = d.nofancy;
  ld.vf[1] = ld.vf[2] = 1;
  if (color != 2) {
#pragma unroll
    for (int c = 1; c <= 2; ++c) {
      const int hf = d.hf[c], vf = d.vf[c], dw = d.cdw[c], dh = d.cdh[c];
      ld.hf[c] = hf, ld.vf[c] = vf, ld.cdw[c] = dw;
      ld.plane_stride[c] = kPitch;
      fancy22[c - 1] = !d.nofancy && hf == 2 && vf == 2 && dw > 2;
      const int cx0 = max(X0 / hf - 1, 0), cx1 = min((X0 + ncols - 1) / hf + 1, dw - 1);
      const int cy0 = max(Y0 / vf - 1, 0), cy1 = min((Y0 + nrows - 1) / vf + 1, dh - 1);
      ChromaRegion &g = cr[c - 1];
      g.ca = cx0 & ~7;
      g.cy0 = cy0;
      g.rows = cy1 - cy0 + 1;          // at most kChromaRows
      ld.cdh[c] = dh - cy0;
      g.chunks = (cx1 - g.ca + 8) >> 3; // at most 34: cx1 < cdw <= the stride
      const uint8_t *pc = planes + d.plane_off[c] + g.ca;
#pragma unroll 1
      for (int r = srow; r < g.rows; r += 16)
#pragma unroll 1
        for (int k = scol; k < g.chunks; k += 16)
          *reinterpret_cast<uint2 *>(&L.c[c - 1][r][8 * k]) = load8(pc + (int64_t)(cy0 + r) * d.plane_stride[c] + 8 * k);
    }
  }
  __syncthreads();
  // ---- h2v2 fancy: the vertical sums, once per (output row, chroma column) ----
  // column j of a row holds chroma column (X0 >> 1) - 1 + j, clamped as
  // chroma_at clamps its neighbour
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    if (!fancy22[c]) continue;
    const int dw = d.cdw[c + 1], dh = d.cdh[c + 1];
    const int cxs = (X0 >> 1) - 1;
    const int nsum = ((X0 + ncols - 1) >> 1) + 2 - cxs; // at most 131
    if (srow < nrows) {
      const int y = Y0 + srow, cy = y >> 1;
      const int ny = (y & 1) ? min(cy + 1, dh - 1) : max(cy - 1, 0);
      const uint8_t *r0 = L.c[c][cy - cr[c].cy0], *r1 = L.c[c][ny - cr[c].cy0];
      for (int j = scol; j < nsum; j += 16) {
        const int cx = clampi(cxs + j, 0, dw - 1) - cr[c].ca;
        L.sum[c][srow][j] = (uint16_t)(r0[cx] * 3 + r1[cx]);
      }
    }
  }
  __syncthreads();

  // ---- convert and store: 4 steps of 4 rows, a wave a row, 4 pixels a lane ----
  const int wave = tid >> 6, lane = tid & 63, lx0 = lane * 4;
  const int P = X0 & 1; // the tile's first column's phase; a lane's own is the same (lx0 is even)
  // chroma_at's planes: the staged regions, moved back by their first column
  // so that the image's chroma columns index them (a byte offset into L that
  // is never negative: the static_assert above); cyo: the rows y is moved by
  const uint8_t *lds = reinterpret_cast<const uint8_t *>(&L);
  const uint8_t *vb[2] = {lds + (offsetof(EmitLds, c) - cr[0].ca),
                          lds + (offsetof(EmitLds, c) + sizeof(L.c[0]) - cr[1].ca)};
  const int cyo[2] = {cr[0].cy0 * ld.vf[1], cr[1].cy0 * ld.vf[2]};
  const int flip = d.flip;
  const bool nhwc = fmt.layout == kLayoutNHWC;
  uint8_t *ob = out + nat_off[img] * es;
  const int ocol0 = flip ? w - bx0 - ncols : bx0; // the tile's first output column
  uint32_t *orow = L.out[wave];
  for (int step = 0; step < kNatTileRows / 4; ++step) {
    const int r = step * 4 + wave;
    if (r < nrows && lx0 < ncols) {
      const int y = Y0 + r;
      const uint8_t *yr = &L.y[r][X0 - xa + lx0];
      int cbv[2][4];
      if (color != 2) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          if (fancy22[c]) {
            // sums of chroma columns (x0 >> 1) - 1 .. + 2, x0 this lane's first x
            const uint16_t *s = &L.sum[c][r][lx0 >> 1];
            const int t0 = s[0], t1 = s[1], t2 = s[2], t3 = s[3];
            // pixel k: x & 1 = (P + k) & 1, thiscol at 1 + ((P + k) >> 1), nextcol one
            // to the right of it for an odd x, one to the left for an even one
            cbv[c][0] = P ? (t1 * 3 + t2 + 7) >> 4 : (t1 * 3 + t0 + 8) >> 4;
            cbv[c][1] = P ? (t2 * 3 + t1 + 8) >> 4 : (t1 * 3 + t2 + 7) >> 4;
            cbv[c][2] = P ? (t2 * 3 + t3 + 7) >> 4 : (t2 * 3 + t1 + 8) >> 4;
            cbv[c][3] = P ? (t3 * 3 + t2 + 8) >> 4 : (t2 * 3 + t3 + 7) >> 4;
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) // a pixel past the tile takes the last one's x: its value is not stored
              cbv[c][k] = chroma_at(ld, vb[c], c + 1, X0 + min(lx0 + k, ncols - 1), y - cyo[c]);
          }
        }
      }
      uint32_t e[3][4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int Y = yr[k];
        uint8_t rgb[3];
        if (color == 2) {
          rgb[0] = rgb[1] = rgb[2] = (uint8_t)Y;
        } else if (color == 1) {
          rgb[0] = (uint8_t)Y, rgb[1] = (uint8_t)cbv[0][k], rgb[2] = (uint8_t)cbv[1][k];
        } else {
          ycc_to_rgb(Y, cbv[0][k], cbv[1][k], rgb);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) e[c][k] = L.lut[c * 256 + rgb[c]];
      }
      if (!nhwc && !flip) {
        // entries past ncols are written too and never stored
#pragma unroll
        for (int c = 0; c < 3; ++c)
          *reinterpret_cast<uint4 *>(&orow[c * kNatTileCols + lx0]) = make_uint4(e[c][0], e[c][1], e[c][2], e[c][3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (lx0 + k >= ncols) continue;
          const int li = flip ? ncols - 1 - (lx0 + k) : lx0 + k;
#pragma unroll
          for (int c = 0; c < 3; ++c) orow[nhwc ? li * 3 + c : c * kNatTileCols + li] = e[c][k];
        }
      }
    }
    wave_lds_sync();
    if (r < nrows) {
      const int oy = by0 + r;
      if (nhwc) {
        store_run(ob + (((int64_t)oy * w + ocol0) * 3) * es, orow, 3 * ncols, es, lane);
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
          store_run(ob + (((int64_t)c * h + oy) * w + ocol0) * es, orow + c * kNatTileCols, ncols, es, lane);
      }
    }
    wave_lds_sync(); // the next step overwrites the row buffer
  }
}

// The failed rows of a native call: row i's region [nat_off[i], nat_off[i + 1])
// elements is zero bytes, whatever its length, and its label -100. kFillSplit
// workgroups a row, each a 16-byte-rounded slice; rows that decoded return.
__global__ void __launch_bounds__(256) k_native_fill(const int32_t *__restrict__ status,
                                                     const int64_t *__restrict__ nat_off, uint8_t *__restrict__ out,
                                                     int64_t *__restrict__ out_labels, int es) {
  const int img = blockIdx.x;
  if (status[img] == 0) return;
  const int64_t bytes = (nat_off[img + 1] - nat_off[img]) * es;
  const int64_t slice = ((bytes + kFillSplit - 1) / kFillSplit + 15) & ~(int64_t)15;
  int64_t lo = (int64_t)blockIdx.y * slice, hi = lo + slice;
  lo = lo < bytes ? lo : bytes;
  hi = hi < bytes ? hi : bytes;
  fmt_zero_bytes(out + nat_off[img] * es + lo, hi - lo, threadIdx.x, 256);
  if (blockIdx.y == 0 && threadIdx.x == 0 && out_labels != nullptr) out_labels[img] = -100;
}

} // namespace

hipError_t launch_emit_rgb(const DevPlan &p, const DevWork &w, float *out, int64_t *out_labels, hipStream_t s) {
  if (p.nat_tiles_total == 0) return hipSuccess;
  hipLaunchKernelGGL(k_emit_rgb, dim3(p.nat_tiles_total), dim3(kEmitThreads), 0, s, p.descs, w.planes, w.status,
                     p.nat_tiles, p.nat_off, p.n, p.lut, p.labels, reinterpret_cast<uint8_t *>(out), out_labels,
                     p.ro.fmt);
  return hipGetLastError();
}

hipError_t launch_fill_failed_native(const DevPlan &p, const DevWork &w, float *out, int64_t *out_labels,
                                     hipStream_t s) {
  if (p.n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_native_fill, dim3(p.n, kFillSplit), dim3(256), 0, s, w.status, p.nat_off,
                     reinterpret_cast<uint8_t *>(out), out_labels, dtype_bytes(p.ro.fmt.dtype));
  return hipGetLastError();
}

} // namespace ldt
