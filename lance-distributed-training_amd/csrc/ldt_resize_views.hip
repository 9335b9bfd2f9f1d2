// ldt_resize_views.hip — the streaming resize of a call with several views
// per image (ldt_set_views): k_resize<0, 2, FILT, F...> (ldt_kernels.hip) over
// (image, view, band, tile). The decoded planes are read once per view from
// d_planes instead of being decoded once per view: everything before the
// resize runs once for the batch.
//
// What differs from k_resize's BOX == 2 variant, and nothing else does:
//   - the box, the flip, the resized size and the window's origin come from
//     the plan's view table (ViewDesc, one entry per output image) and not
//     from the descriptor;
//   - the planes and the colour handling come from descs[img], the status from
//     status[img], and the store goes to output image view * n + img
//     (view-major: out[v] is a dense batch);
//   - the label is written once per image, by view 0.
// The staging, the coefficients (resample_coeffs<FILT> per workgroup), the
// uint8 value between the passes, the table lookup and both stores are
// k_resize's, so output image (v, i) is bit for bit what a single-view call
// with row i's view-v crop and window gives. The LDS layout and size are
// k_resize's too (resize_lds_bytes over the widest view), and with them the
// occupancy.
//
// Grid order. k_resize gives all workgroups of an image one blockIdx % 8 (one
// XCD under the observed round-robin placement). Both orders here keep that
// residue for every view of the image, so the V reads of its planes go
// through one XCD's L2:
//   order 0 (default)  the views of an image follow each other inside its
//                      group of 8 images: group, view, band, tile, image % 8.
//                      A view starts while the planes the view before it read
//                      may still be in that L2.
//   order 1            view-major launch order: all images' view 0, then all
//                      images' view 1, ... A batch's planes (about 100 MB at
//                      256 x 512 x 512) pass between two views of an image.
// LDT_OPT_VIEW_ORDER chooses; DESIGN.md §4 has the measurement.
//
// Per-view output sizes (ldt_set_view_sizes): the SIZED instantiations. The
// output size, bands and tiles of a workgroup's view, and where the view's
// dense block starts in the output, come from the call's geometry table
// (ViewGeomTab, ldt_view_index.hpp: a kernel argument, so finding the view is
// a walk over at most 16 scalars, uniform over the workgroup) and not from
// launch arguments; the grid is the sum over the views in the same two orders.
// Nothing else differs, so output (v, i) is bit for bit what a single-size
// call at (h_v, w_v) gives. A call without sizes launches the instantiations
// it always did: SIZED is a compile-time branch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "ldt_device.hpp"
#include "ldt_kernels.hpp"
#include "ldt_view_index.hpp"

#pragma clang fp contract(off)

namespace ldt {

namespace {

__device__ __forceinline__ OutFmt vfmt_arg() { return OutFmt(); }
__device__ __forceinline__ OutFmt vfmt_arg(OutFmt f) { return f; }

static_assert(kViewGeomMax == kMaxViews && kViewGeomBandRows == kBandRows && kViewGeomTileCols == kTileCols,
              "ldt_view_index.hpp and ldt_types.hpp disagree");
// What a uniform call passes where a sized one passes its table.
struct NoGeom {};

template <int FILT, bool SIZED, typename... F>
__global__ void __launch_bounds__(kResizeThreads)
    k_resize_views(const ImgDesc *__restrict__ descs, const ViewDesc *__restrict__ vtab,
                   const uint8_t *__restrict__ planes, const float *__restrict__ lut,
                   const int64_t *__restrict__ labels, float *__restrict__ out, int64_t *__restrict__ out_labels,
                   const int32_t *__restrict__ status, int n, int views, int order, int ks_h, int ks_v,
                   int row_bytes, int oh, int ow, const std::conditional_t<SIZED, ViewGeomTab, NoGeom> geom,
                   F... fmt_pack) {
  static_assert(kResizeThreads == kTileCols, "one thread per column of a tile");
  static_assert(sizeof...(F) <= 1, "at most the format");
  constexpr bool FMT = sizeof...(F) == 1;
  const OutFmt fmt = vfmt_arg(fmt_pack...);
  const int L = blockIdx.x;
  int img, view, band, tile;
  int64_t obase = 0; // SIZED: first element of the view's dense block
  if constexpr (SIZED) {
    // oh, ow arrive as the widest view's (unused); the view's own replace them
    const ViewWork vw = view_work(geom, order, L);
    img = vw.img;
    view = vw.view;
    band = vw.band;
    tile = vw.tile;
    oh = geom.g[view].oh;
    ow = geom.g[view].ow;
    obase = geom.g[view].base;
  } else {
    const int NB = (oh + kBandRows - 1) / kBandRows, NT = (ow + kTileCols - 1) / kTileCols;
    const int per_view = 8 * NB * NT; // workgroups of one view of one group of 8 images
    int g, rr;
    if (order == 0) {
      g = L / (per_view * views);
      const int q = L % (per_view * views);
      view = q / per_view;
      rr = q % per_view;
    } else {
      const int groups = (n + 7) / 8;
      view = L / (per_view * groups);
      const int q = L % (per_view * groups);
      g = q / per_view;
      rr = q % per_view;
    }
    img = g * 8 + (rr % 8); // per_view is a multiple of 8: blockIdx % 8 == img % 8 in both orders
    band = (rr / 8) / NT;
    tile = (rr / 8) % NT;
  }
  if (img >= n || view >= views) return;
  if (status[img] != 0) return;
  const int tid = threadIdx.x;
  const int64_t vimg = (int64_t)view * n + img; // the view table's index
  // the output image: in a sized call the row inside the view's own block at obase
  const int64_t oimg = SIZED ? (int64_t)img : vimg;
  const ViewDesc vd = vtab[vimg];
  const int W = vd.box_w, H = vd.box_h, top = vd.box_top, left = vd.box_left, flip = vd.flip;
  const int rh = vd.res_h, rw = vd.res_w, wtop = vd.win_top, wleft = vd.win_left;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  float *s_lut = reinterpret_cast<float *>(smem);                 // 768 floats
  const int tcols = min(ow, kTileCols);                           // columns of a full tile (SIZED: this view's)
  int32_t *s_kh = reinterpret_cast<int32_t *>(smem + 3072);       // tcols * ks_h
  int32_t *s_kv = s_kh + tcols * ks_h;                            // kBandRows * ks_v
  int32_t *s_hb = s_kv + kBandRows * ks_v;                        // tcols * 2
  int32_t *s_vb = s_hb + 2 * tcols;                               // kBandRows * 2
  uint8_t *s_row = reinterpret_cast<uint8_t *>(s_vb + 2 * kBandRows); // 2 * row_bytes

  const int es = FMT ? dtype_bytes(fmt.dtype) : 4; // FMT: bytes per element
  if constexpr (FMT) {
    uint32_t *sb = reinterpret_cast<uint32_t *>(smem);
    for (int i = tid; i < 768; i += kResizeThreads)
      sb[i] = es == 4   ? reinterpret_cast<const uint32_t *>(lut)[i]
              : es == 2 ? (uint32_t) reinterpret_cast<const uint16_t *>(lut)[i]
                        : (uint32_t)(i & 255);
  } else {
    for (int i = tid; i < 768; i += kResizeThreads) s_lut[i] = lut[i];
  }
  const int oy0 = band * kBandRows, ox0 = tile * kTileCols;
  const int nrows = min(kBandRows, oh - oy0); // rows of this band (the last one may be short)
  const int ncols = min(kTileCols, ow - ox0); // columns of this tile
  if (tid < ncols) {
    int xmin;
    const int cnt = resample_coeffs<FILT>(W, rw, wleft + ox0 + tid, ks_h, s_kh + tid * ks_h, &xmin);
    s_hb[2 * tid] = xmin;
    s_hb[2 * tid + 1] = cnt;
  }
  // the vertical rows by the last kBandRows threads: idle ones unless the tile
  // is nearly full. Rows past the image get an empty window.
  if (tid >= kResizeThreads - kBandRows) {
    const int j = tid - (kResizeThreads - kBandRows);
    int ymin = 0, cnt = 0;
    if (j < nrows) cnt = resample_coeffs<FILT>(H, rh, wtop + oy0 + j, ks_v, s_kv + j * ks_v, &ymin);
    s_vb[2 * j] = ymin;
    s_vb[2 * j + 1] = cnt;
  }
  if (view == 0 && band == 0 && tile == 0 && tid == 0 && labels != nullptr) out_labels[img] = labels[img];
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

  const ImgDesc &d = descs[img];
  for (int y = ya; y < yb; ++y) {
    uint8_t *row = s_row + ((y - ya) & 1) * row_bytes;
    // ---- stage row top + y of the image, from column left, as interleaved RGB in LDS ----
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
        // the image's absolute coordinates: the fancy upsampling's edge rules
        // are those of the whole image
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
    __syncthreads();
    // ---- horizontal taps for column ox0 + tid, then vertical accumulate ----
    if (tid < ncols) {
      int32_t s0 = 1 << (kPrecisionBits - 1), s1 = s0, s2 = s0;
      const int32_t *k = s_kh + tid * ks_h;
      const uint8_t *p = row + 3 * hxmin;
      for (int t = 0; t < hcnt; ++t) {
        const int32_t kw = k[t];
        s0 += (int32_t)p[3 * t] * kw;
        s1 += (int32_t)p[3 * t + 1] * kw;
        s2 += (int32_t)p[3 * t + 2] * kw;
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
  const int ox = flip ? ow - 1 - (ox0 + tid) : ox0 + tid;
  if constexpr (FMT) {
    const uint32_t *s_bits = reinterpret_cast<const uint32_t *>(smem);
    uint8_t *ob = reinterpret_cast<uint8_t *>(out) + obase * es;
#pragma unroll
    for (int j = 0; j < kBandRows; ++j) {
      const int oy = oy0 + j;
      if (j < nrows) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int64_t e = fmt.layout == kLayoutNHWC ? ((oimg * oh + oy) * ow + ox) * 3 + c
                                                      : ((oimg * 3 + c) * oh + oy) * ow + ox;
          fmt_store1(ob + e * es, es, s_bits[c * 256 + clip8(acc[j][c])]);
        }
      }
    }
  } else {
    float *o = out + obase + oimg * 3 * oh * ow;
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

// The failed rows of a call with views: all `views` outputs of a row whose
// status is not 0 are zero bytes (zero in every element type), its label -100.
// One workgroup per output image, blockIdx.y the view.
__global__ void __launch_bounds__(256) k_fill_failed_views(const int32_t *__restrict__ status,
                                                           uint8_t *__restrict__ out,
                                                           int64_t *__restrict__ out_labels, int n,
                                                           int64_t cell_bytes) {
  const int img = blockIdx.x, view = blockIdx.y;
  if (status[img] == 0) return;
  fmt_zero_bytes(out + ((int64_t)view * n + img) * cell_bytes, cell_bytes, threadIdx.x, 256);
  if (view == 0 && threadIdx.x == 0 && out_labels != nullptr) out_labels[img] = -100;
}

// The same for a call with per-view sizes: each view's own cell at its own base.
__global__ void __launch_bounds__(256) k_fill_failed_view_sizes(const int32_t *__restrict__ status,
                                                                uint8_t *__restrict__ out,
                                                                int64_t *__restrict__ out_labels, int n, int es,
                                                                const ViewGeomTab geom) {
  const int img = blockIdx.x, view = blockIdx.y;
  if (status[img] != 0) {
    const int64_t cell = (int64_t)3 * geom.g[view].oh * geom.g[view].ow;
    fmt_zero_bytes(out + (geom.g[view].base + img * cell) * es, cell * es, threadIdx.x, 256);
    if (view == 0 && threadIdx.x == 0 && out_labels != nullptr) out_labels[img] = -100;
  }
}

size_t views_lds_bytes(int ks_h, int ks_v, int row_bytes, int ow) {
  const int tcols = ow < kTileCols ? ow : kTileCols;
  return 3072 + (size_t)4 * (tcols * ks_h + kBandRows * ks_v + 2 * tcols + 2 * kBandRows) + 2 * (size_t)row_bytes;
}

// Allow up to the full 160 KiB of LDS (wide boxes), as k_resize has it.
hipError_t views_lds_attr() {
  static hipError_t once = [] {
    const void *fns[] = {reinterpret_cast<const void *>(&k_resize_views<kFilterBilinear, false>),
                         reinterpret_cast<const void *>(&k_resize_views<kFilterBicubic, false>),
                         reinterpret_cast<const void *>(&k_resize_views<kFilterBilinear, false, OutFmt>),
                         reinterpret_cast<const void *>(&k_resize_views<kFilterBicubic, false, OutFmt>),
                         reinterpret_cast<const void *>(&k_resize_views<kFilterBilinear, true>),
                         reinterpret_cast<const void *>(&k_resize_views<kFilterBicubic, true>),
                         reinterpret_cast<const void *>(&k_resize_views<kFilterBilinear, true, OutFmt>),
                         reinterpret_cast<const void *>(&k_resize_views<kFilterBicubic, true, OutFmt>)};
    hipError_t e = hipSuccess;
    for (const void *f : fns)
      if (e == hipSuccess) e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    return e;
  }();
  return once;
}

} // namespace

int64_t resize_views_groups(int n, int views, int oh, int ow) {
  const int64_t nb = (oh + kBandRows - 1) / kBandRows, nt = (ow + kTileCols - 1) / kTileCols;
  return (int64_t)((n + 7) / 8) * 8 * views * nb * nt;
}

hipError_t launch_resize_views(const DevPlan &p, const DevWork &w, float *out, int64_t *out_labels, hipStream_t s,
                               int filter, int order) {
  if (p.n == 0) return hipSuccess;
  if (p.geom != nullptr) {
    // per-view sizes: the grid is the table's sum, the LDS that of the widest view
    const ViewGeomTab &t = *p.geom;
    if (t.views != p.n_views || t.views < 1 || p.views == nullptr || t.total < 1 || t.total > 0x7FFFFFFF ||
        t.groups != (p.n + 7) / 8)
      return hipErrorInvalidValue;
    const int row_bytes = ((p.max_w * 3 + 15) / 16) * 16;
    const size_t lds = views_lds_bytes(p.max_ks_h, p.max_ks_v, row_bytes, t.max_ow);
    if (lds > 64 * 1024) {
      hipError_t e = views_lds_attr();
      if (e != hipSuccess) return e;
    }
    const dim3 grid((unsigned)t.total), block(kResizeThreads);
    if (!fmt_default(p.ro.fmt)) {
      auto kern = filter == kFilterBicubic ? k_resize_views<kFilterBicubic, true, OutFmt>
                                           : k_resize_views<kFilterBilinear, true, OutFmt>;
      hipLaunchKernelGGL(kern, grid, block, lds, s, p.descs, p.views, w.planes, p.lut, p.labels, out, out_labels,
                         w.status, p.n, p.n_views, order, p.max_ks_h, p.max_ks_v, row_bytes, 0, t.max_ow, t, p.ro.fmt);
      return hipGetLastError();
    }
    auto kern = filter == kFilterBicubic ? k_resize_views<kFilterBicubic, true> : k_resize_views<kFilterBilinear, true>;
    hipLaunchKernelGGL(kern, grid, block, lds, s, p.descs, p.views, w.planes, p.lut, p.labels, out, out_labels,
                       w.status, p.n, p.n_views, order, p.max_ks_h, p.max_ks_v, row_bytes, 0, t.max_ow, t);
    return hipGetLastError();
  }
  const int64_t groups = resize_views_groups(p.n, p.n_views, p.ro.oh, p.ro.ow);
  if (p.n_views < 1 || p.n_views > kMaxViews || p.views == nullptr || groups > 0x7FFFFFFF) return hipErrorInvalidValue;
  const int row_bytes = ((p.max_w * 3 + 15) / 16) * 16;
  const size_t lds = views_lds_bytes(p.max_ks_h, p.max_ks_v, row_bytes, p.ro.ow);
  if (lds > 64 * 1024) {
    hipError_t e = views_lds_attr();
    if (e != hipSuccess) return e;
  }
  const dim3 grid((unsigned)groups), block(kResizeThreads);
  if (!fmt_default(p.ro.fmt)) {
    auto kern = filter == kFilterBicubic ? k_resize_views<kFilterBicubic, false, OutFmt>
                                         : k_resize_views<kFilterBilinear, false, OutFmt>;
    hipLaunchKernelGGL(kern, grid, block, lds, s, p.descs, p.views, w.planes, p.lut, p.labels, out, out_labels,
                       w.status, p.n, p.n_views, order, p.max_ks_h, p.max_ks_v, row_bytes, p.ro.oh, p.ro.ow, NoGeom(),
                       p.ro.fmt);
    return hipGetLastError();
  }
  auto kern = filter == kFilterBicubic ? k_resize_views<kFilterBicubic, false> : k_resize_views<kFilterBilinear, false>;
  hipLaunchKernelGGL(kern, grid, block, lds, s, p.descs, p.views, w.planes, p.lut, p.labels, out, out_labels,
                     w.status, p.n, p.n_views, order, p.max_ks_h, p.max_ks_v, row_bytes, p.ro.oh, p.ro.ow, NoGeom());
  return hipGetLastError();
}

hipError_t launch_fill_failed_views(const DevPlan &p, const DevWork &w, float *out, int64_t *out_labels,
                                    hipStream_t s) {
  if (p.n == 0) return hipSuccess;
  if (p.geom != nullptr) {
    hipLaunchKernelGGL(k_fill_failed_view_sizes, dim3(p.n, p.n_views), dim3(256), 0, s, w.status,
                       reinterpret_cast<uint8_t *>(out), out_labels, p.n, dtype_bytes(p.ro.fmt.dtype), *p.geom);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(k_fill_failed_views, dim3(p.n, p.n_views), dim3(256), 0, s, w.status,
                     reinterpret_cast<uint8_t *>(out), out_labels, p.n,
                     (int64_t)3 * p.ro.oh * p.ro.ow * dtype_bytes(p.ro.fmt.dtype));
  return hipGetLastError();
}

} // namespace ldt
