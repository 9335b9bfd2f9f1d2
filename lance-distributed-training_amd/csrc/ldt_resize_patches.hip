// ldt_resize_patches.hip — the store of a patch call (ldt_decode_patches):
// every good row's source rectangle resized to its own res_h x res_w as
// k_resize_ragged does (Pillow's BILINEAR or BICUBIC bit for bit), and stored
// not as a planar image but as the packed patches a native-resolution ViT
// takes: region row (gy * gw + gx in merge-block order) of C * T * P * P
// elements, the Hugging Face Qwen2-VL image processor's order (include/ldt.h).
// It is launched in place of k_resize_ragged, whose plan it shares (tile
// prefix, int64 offsets, sizes, the uniform binary search).
//
// k_resize_patches<FILT, NR>. One workgroup of 256 lanes serves one tile: one
// block row (B = P * m pixel rows) by TC = (256 / B) * B columns, so a tile
// holds nb = ncols / B whole blocks of m x m patches, and those are one
// contiguous run of nb * m * m * 3 * T * P * P elements of the output. The
// permutation is therefore a property of the tile's store and costs no pass.
//
// Staging and the horizontal pass are k_resize_ragged's: the tile's column
// span of each source row in aligned 8-byte loads, chroma_at / ycc_to_rgb once
// per staged pixel, Pillow's horizontal taps to a clip8 byte per source row,
// floating-point contraction off.
//
// Vertical pass. A lane owns one output column and all B rows of the block
// row, in two halves of B / 2 rows: 3 * NR int32 accumulators (NR = 8 for B =
// 14, 16; 16 for B = 28, 32) instead of 3 * B, which held the kernel to two
// waves per SIMD (DESIGN.md §4 has the compiler's counts). Each half walks only
// the source rows its own windows read, so the halves share no more than the
// filter's reach of rows. The first half's clipped bytes wait packed in
// 3 * NR / 4 registers. Which rows a source row feeds is found once per source
// row and wave: lane j of each half wave holds row j's window in two
// registers, a ballot over "y is inside" gives a scalar mask, and the unrolled
// loop over the rows branches on its bits, so a row outside costs two scalar
// instructions and no LDS read.
//
// Pixel tile. After the last source row the staging is dead; the lane writes
// its 3 * B clipped bytes into the tile [3][B][TC] that lies over it, at its
// mirrored column when the row is flipped (rw and TC are multiples of B, so
// the mirrored tile is block-aligned too).
//
// Write-out. The 256 lanes walk the run linearly, four elements a lane a step.
// An element's index is taken apart with multiply-high divisions by the
// call's uniform sizes (block, my, mx, then c, t, py, px or t, py, px, c) to a
// tile address, the byte goes through the call's 768-entry table in LDS, and
// the elements are stored as store_run stores them: singly up to the first
// 4-element boundary and after the last, vectors between. T = 2 reads each
// tile byte twice; no pixel is computed twice. The label is written once per
// image. A failed row is not touched: k_native_fill does it.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ldt_device.hpp"
#include "ldt_kernels.hpp"

#pragma clang fp contract(off)

namespace ldt {
namespace {

constexpr int kPatThreads = 256;
static_assert(kPatchChromaBase >= LDT_MAX_DIM, "a chroma region's base minus its first column stays in LDS");

__device__ __forceinline__ uint2 load8(const uint8_t *p) { return *reinterpret_cast<const uint2 *>(p); }

// e / d for e < 2^16 and d < 2^16 by one multiply-high: magic = ceil(2^32 / d)
// errs by less than e * d / 2^32 < 1 part of d.
struct Div16 {
  uint32_t d, magic;
  __device__ __forceinline__ explicit Div16(uint32_t dd) : d(dd), magic(0xFFFFFFFFu / dd + 1u) {}
  __device__ __forceinline__ uint32_t div(uint32_t e, uint32_t *rem) const {
    const uint32_t q = __umulhi(e, magic);
    *rem = e - q * d;
    return q;
  }
};

// The tile address of element e of a tile's run: patch q = e / (3 * T * P * P)
// is (block, my, mx) in merge order, the rest (c, t, py, px) under NCHW and
// (t, py, px, c) under NHWC; t only repeats the frame.
struct RunIndex {
  Div16 by_patch, by_plane, by_row, by_px;
  uint32_t P, PP, T, sh, B, TC;
  bool nhwc;
  __device__ __forceinline__ RunIndex(const PatchGeom &g, bool nhwc_)
      : by_patch(3u * g.temporal * g.patch * g.patch),
        by_plane(nhwc_ ? 3u * g.patch : (uint32_t)g.temporal * g.patch * g.patch), by_row(g.patch), by_px(3u),
        P(g.patch), PP(g.patch * g.patch), T(g.temporal), sh(g.merge - 1), B(g.rows), TC(g.cols), nhwc(nhwc_) {}
  // -> the tile byte's offset and its channel
  __device__ __forceinline__ uint32_t at(uint32_t e, uint32_t *c_out) const {
    uint32_t r, c, py, px;
    const uint32_t q = by_patch.div(e, &r);
    if (nhwc) {
      if (T == 2 && r >= 3 * PP) r -= 3 * PP;
      py = by_plane.div(r, &r);
      px = by_px.div(r, &c);
    } else {
      c = by_plane.div(r, &r);
      if (T == 2 && r >= PP) r -= PP;
      py = by_row.div(r, &px);
    }
    const uint32_t mx = q & sh, my = (q >> sh) & sh, blk = q >> (2 * sh);
    *c_out = c;
    return (c * B + my * P + py) * TC + ((blk << sh) + mx) * P + px;
  }
};

template <int FILT, int NR>
__global__ void __launch_bounds__(kPatThreads)
    k_resize_patches(const ImgDesc *__restrict__ descs, const uint8_t *__restrict__ planes,
                     const int32_t *__restrict__ status, const int32_t *__restrict__ tile_pref,
                     const int64_t *__restrict__ nat_off, const int32_t *__restrict__ nat_res, int n,
                     const float *__restrict__ lut, const int64_t *__restrict__ labels, uint8_t *__restrict__ out,
                     int64_t *__restrict__ out_labels, OutFmt fmt, PatchCap cap) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int tid = threadIdx.x, tile = blockIdx.x;
  const int B = cap.g.rows, TC = cap.g.cols;
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
  const int tiles_x = (rw + TC - 1) / TC;
  const int by = t / tiles_x, tx = t - by * tiles_x;
  const int ox0 = tx * TC, oy0 = by * B;
  const int ncols = min(TC, rw - ox0);
  const int ks_h = resample_ksize_host(W, rw, FILT), ks_v = resample_ksize_host(H, rh, FILT);
  // what the planner checked and sized the LDS by holds this tile (uniform; never taken)
  const int HB = B >> 1; // rows of a half
  if (HB > NR || rh % B != 0 || rw % B != 0 || oy0 + B > rh || ncols * ks_h > cap.kh_words || ks_v > cap.ks_v) return;
  if (t == 0 && tid == 0 && labels != nullptr) out_labels[img] = labels[img];

  const PatchLds L = patch_lds(cap);
  const int pitch = ragged_pitch(cap.span);
  uint32_t *s_lut = reinterpret_cast<uint32_t *>(smem);
  int32_t *s_hb = reinterpret_cast<int32_t *>(smem + L.hb);
  int32_t *s_vb = reinterpret_cast<int32_t *>(smem + L.vb);
  int32_t *s_kv = reinterpret_cast<int32_t *>(smem + L.kv);
  int32_t *s_kh = reinterpret_cast<int32_t *>(smem + L.kh);
  uint8_t *s_y = smem + L.y;
  uint8_t *s_rgb = smem + L.rgb;
  uint8_t *s_tile = smem + L.tile;

  const int es = dtype_bytes(fmt.dtype);
  for (int i = tid; i < 768; i += kPatThreads)
    s_lut[i] = es == 4   ? reinterpret_cast<const uint32_t *>(lut)[i]
               : es == 2 ? (uint32_t) reinterpret_cast<const uint16_t *>(lut)[i]
                         : (uint32_t)(i & 255);
  // ---- coefficients: a lane a column, the last B lanes a row each ----
  if (tid < ncols) {
    int xmin;
    const int cnt = resample_coeffs<FILT>(W, rw, ox0 + tid, ks_h, s_kh + tid * ks_h, &xmin);
    s_hb[2 * tid] = xmin;
    s_hb[2 * tid + 1] = cnt;
  }
  if (tid >= kPatThreads - B) {
    const int j = tid - (kPatThreads - B);
    int ymin;
    const int cnt = resample_coeffs<FILT>(H, rh, oy0 + j, ks_v, s_kv + j * ks_v, &ymin);
    s_vb[2 * j] = ymin;
    s_vb[2 * j + 1] = cnt;
  }
  __syncthreads();
  const int xa = s_hb[0], span = s_hb[2 * (ncols - 1)] + s_hb[2 * (ncols - 1) + 1] - xa;
  if (span > cap.span) return; // uniform; the planner's bound says never

  // ---- the span in the image, and what of each plane holds it ----
  const int X0 = d.box_left + xa, xa8 = X0 & ~7;
  const int ychunks = (X0 + span - xa8 + 7) >> 3; // 8 * ychunks <= span + 14 <= pitch; ends inside the stride
  const uint8_t *py = planes + d.plane_off[0] + xa8;
  const int color = d.color;
  // chroma_at's view of a component's staged rows, as in k_resize_ragged
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

  int hoff = 0, hcnt = 0;
  if (tid < ncols) {
    hoff = s_hb[2 * tid] - xa;
    hcnt = s_hb[2 * tid + 1];
  }
  int32_t acc[NR][3];
  uint32_t keep[3 * NR / 4]; // the first half's bytes, byte 3 * j + c
#pragma unroll
  for (int k = 0; k < 3 * NR / 4; ++k) keep[k] = 0;

#pragma unroll 1
  for (int half = 0; half < 2; ++half) {
  const int j0 = half * HB;
  // row j0 + (lane & 31)'s window in this lane's registers: every wave ballots
  // the rows a source row feeds from them (a lane past HB holds an empty window)
  const int jrow = tid & 31;
  const int wmin = jrow < HB ? s_vb[2 * (j0 + jrow)] : 0, wcnt = jrow < HB ? s_vb[2 * (j0 + jrow) + 1] : 0;
  const int ya = s_vb[2 * j0], yb = s_vb[2 * (j0 + HB - 1)] + s_vb[2 * (j0 + HB - 1) + 1];
#pragma unroll
  for (int j = 0; j < NR; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 1 << (kPrecisionBits - 1);

  for (int y = ya; y < yb; ++y) {
    const int Y = d.box_top + y;
    // ---- raw: this row's luma and the chroma rows its upsampling reads ----
#pragma unroll 1
    for (int k = tid; k < ychunks; k += kPatThreads)
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
    for (int x = tid; x < span; x += kPatThreads) {
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
    // ---- the rows this source row feeds: bit j of a wave-uniform mask ----
    const uint64_t inside = __ballot(y >= wmin && y - wmin < wcnt);
    const uint32_t rows = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)inside);
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
      for (int j = 0; j < NR; ++j) {
        if (rows & (1u << j)) { // uniform
          const int32_t kw = s_kv[(j0 + j) * ks_v + y - __builtin_amdgcn_readlane(wmin, j)];
          acc[j][0] += h0 * kw;
          acc[j][1] += h1 * kw;
          acc[j][2] += h2 * kw;
        }
      }
    }
  }
  if (half == 0) {
#pragma unroll
    for (int j = 0; j < NR; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) keep[(3 * j + c) >> 2] |= clip8(acc[j][c]) << (8 * ((3 * j + c) & 3));
  }
  } // half

  // ---- the pixel tile over the dead staging, mirrored when the row is flipped ----
  __syncthreads(); // every lane is past the last row's taps
  const int flip = d.flip;
  if (tid < ncols) {
    uint8_t *o = s_tile + (flip ? ncols - 1 - tid : tid);
#pragma unroll
    for (int j = 0; j < NR; ++j)
      if (j < HB) { // uniform
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          o[(c * B + j) * TC] = (uint8_t)(keep[(3 * j + c) >> 2] >> (8 * ((3 * j + c) & 3)));
          o[(c * B + HB + j) * TC] = (uint8_t)clip8(acc[j][c]);
        }
      }
  }
  __syncthreads();

  // ---- write-out: the tile's blocks are one run of the row's region ----
  const int E = 3 * cap.g.temporal * cap.g.patch * cap.g.patch, mm = cap.g.merge * cap.g.merge;
  const int ocol0 = flip ? rw - ox0 - ncols : ox0; // the tile's first output column
  const int nrun = (ncols / B) * mm * E;           // <= 49152 elements
  uint8_t *dst = out + (nat_off[img] + ((int64_t)by * (rw / B) + ocol0 / B) * mm * E) * es;
  const RunIndex ix(cap.g, fmt.layout == kLayoutNHWC);
  auto elem = [&](int e) {
    uint32_t c;
    const uint32_t a = ix.at((uint32_t)e, &c);
    return s_lut[c * 256 + s_tile[a]];
  };
  const int vbytes = 4 * es;
  int head = (int)((vbytes - (int)((uintptr_t)dst & (uintptr_t)(vbytes - 1))) & (vbytes - 1)) / es;
  if (head > nrun) head = nrun;
  if (tid < head) fmt_store1(dst + tid * es, es, elem(tid));
  const int nq = (nrun - head) >> 2;
  for (int q = tid; q < nq; q += kPatThreads) {
    const int e = head + 4 * q;
    fmt_store4(dst + (int64_t)e * es, es, elem(e), elem(e + 1), elem(e + 2), elem(e + 3));
  }
  const int t0 = head + 4 * nq;
  if (tid < nrun - t0) fmt_store1(dst + (int64_t)(t0 + tid) * es, es, elem(t0 + tid));
}

template <int FILT, int NR>
hipError_t launch_one(const DevPlan &p, const DevWork &w, float *out, int64_t *out_labels, hipStream_t s) {
  // up to the full 160 KiB of LDS (wide boxes under a large reduction), once per kernel
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_resize_patches<FILT, NR>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, kRaggedLdsMax);
  if (attr != hipSuccess) return attr;
  hipLaunchKernelGGL((k_resize_patches<FILT, NR>), dim3(p.nat_tiles_total), dim3(kPatThreads), patch_lds(p.pat).bytes,
                     s, p.descs, w.planes, w.status, p.nat_tiles, p.nat_off, p.nat_res, p.n, p.lut, p.labels,
                     reinterpret_cast<uint8_t *>(out), out_labels, p.ro.fmt, p.pat);
  return hipGetLastError();
}

} // namespace

hipError_t launch_resize_patches(const DevPlan &p, const DevWork &w, float *out, int64_t *out_labels, hipStream_t s,
                                 int filter) {
  if (p.nat_tiles_total == 0) return hipSuccess;
  const PatchGeom &g = p.pat.g;
  if (!patch_spec_ok(g.patch, g.merge, g.temporal, 0) || g.rows != g.patch * g.merge ||
      patch_lds(p.pat).bytes > kRaggedLdsMax)
    return hipErrorInvalidValue;
  const bool cubic = filter == kFilterBicubic;
  // NR: the rows of a half, 7 or 8 and 14 or 16
  if (g.rows <= 16)
    return cubic ? launch_one<kFilterBicubic, 8>(p, w, out, out_labels, s)
                 : launch_one<kFilterBilinear, 8>(p, w, out, out_labels, s);
  return cubic ? launch_one<kFilterBicubic, 16>(p, w, out, out_labels, s)
               : launch_one<kFilterBilinear, 16>(p, w, out, out_labels, s);
}

} // namespace ldt
