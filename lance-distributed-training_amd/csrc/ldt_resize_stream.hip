// ldt_resize_stream.hip — the streaming resize: every call the band kernel
// k_resize4 (ldt_resize4.hip) does not take. Crops, windows, BICUBIC, outputs
// wider than kTileCols, wide sources, and every call with views.
//
// Fused source (JPEG planes or raw HWC) -> Pillow BILINEAR or BICUBIC oh x ow
// -> LUT (ToTensor [+Normalize]) -> fp32 CHW, or the call's format. Two
// kernels find a workgroup's tile, one body (resize_stream_tile,
// ldt_resize_stream.hpp) resizes it:
//   k_resize<SRC, BOX, FILT, F...>      a call with one view per image, over
//                                       (image, band, tile); SRC 1: raw HWC cells
//   k_resize_views<FILT, SIZED, F...>   a call with views (ldt_set_views,
//                                       ldt_set_view_sizes), over (image, view,
//                                       band, tile), JPEG planes only
// Because the body is one, output image (v, i) of a call with views is bit for
// bit what a single-view call with row i's view-v crop and window gives, the
// LDS layout and size (stream_lds_bytes, over the widest source and output of
// the launch) are the same, and with them the occupancy.
//
// Grid order. k_resize: workgroups of an image share blockIdx % 8 (one XCD
// under the observed round-robin placement, for L2 reuse of overlapping rows),
// a band's tiles follow each other.
//
// BOX (a batch with crops, ldt_set_crops): the image's box is the whole source
// of the resize. W and H are the box's, the staging reads source column
// left + x and row top + y and stages only the box's columns (row_bytes is
// sized by the widest box), while chroma_at still gets the image's absolute
// coordinates, so the fancy upsampling's edge rules stay those of the whole
// image; a flipped image stores column x at ow - 1 - x. The box comes from
// the descriptor (JPEG planes) or from `boxes` (raw HWC, one ldt_crop per
// image), checked on the host to lie inside the source. Without BOX nothing
// of this is compiled in and `boxes` is not read.
//
// BOX == 2 (a batch with windows, ldt_set_windows): the source (the box, which
// the planner fills with the whole image when the batch has no crops) is
// resized to the image's own res_h x res_w, and the oh x ow output is the
// window of that result at (win_top, win_left): output column x takes the
// coefficients of (W -> res_w) at index win_left + x and output row y those
// of (H -> res_h) at win_top + y; staging, chroma_at, the store and the flip
// are those of BOX == 1. ks_h / ks_v are the taps of (source -> res). The
// window comes from the descriptor (JPEG planes) or from `wins` (raw HWC, one
// ldt_window per image; `boxes` may then be null: the whole cell), checked on
// the host to lie inside res. BOX < 2 compiles none of this in and does not
// read `wins`.
//
// FILT (ldt_set_filter, per call): the filter whose coefficients
// resample_coeffs<FILT> computes, Pillow's BILINEAR or BICUBIC; ks_h / ks_v are
// the taps of that filter (resample_ksize_host). Nothing else depends on it.
//
// FMT (ldt_set_output_format, every call whose format is not float32 CHW): the
// LDS table holds the output element's bits and the store takes fmt.dtype /
// fmt.layout, uniform over the launch. The format is a trailing kernel
// argument that only the FMT instantiations have (F = OutFmt; the pack is
// empty otherwise), so the float32 CHW kernels keep the signature, and with it
// the code, they had before the format existed.
//
// k_resize_views. The decoded planes are read once per view from d_planes
// instead of being decoded once per view: everything before the resize runs
// once for the batch. What differs from k_resize's BOX == 2 variant, and
// nothing else does:
//   - the box, the flip, the resized size and the window's origin come from
//     the plan's view table (ViewDesc, one entry per output image) and not
//     from the descriptor;
//   - the planes and the colour handling come from descs[img], the status from
//     status[img], and the store goes to output image view * n + img
//     (view-major: out[v] is a dense batch);
//   - the label is written once per image, by view 0.
// Both of its grid orders keep k_resize's blockIdx % 8 residue for every view
// of the image, so the V reads of its planes go through one XCD's L2:
//   order 0 (default)  the views of an image follow each other inside its
//                      group of 8 images: group, view, band, tile, image % 8.
//                      A view starts while the planes the view before it read
//                      may still be in that L2.
//   order 1            view-major launch order: all images' view 0, then all
//                      images' view 1, ... A batch's planes (about 100 MB at
//                      256 x 512 x 512) pass between two views of an image.
// LDT_OPT_VIEW_ORDER chooses; DESIGN.md §4 has the measurement.
//
// SIZED (per-view output sizes, ldt_set_view_sizes): the output size, bands
// and tiles of a workgroup's view, and where the view's dense block starts in
// the output, come from the call's geometry table (ViewGeomTab,
// ldt_view_index.hpp: a kernel argument, so finding the view is a walk over at
// most 16 scalars, uniform over the workgroup) and not from launch arguments;
// the grid is the sum over the views in the same two orders. Nothing else
// differs, so output (v, i) is bit for bit what a single-size call at
// (h_v, w_v) gives. A call without sizes launches the instantiations it
// always did: SIZED is a compile-time branch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <array>
#include <type_traits>
#include <utility>

#include "ldt_kernels.hpp"
#include "ldt_resize_stream.hpp"
#include "ldt_view_index.hpp"

#pragma clang fp contract(off)

namespace ldt {

template <int SRC, int BOX, int FILT, typename... F>
__global__ void __launch_bounds__(kResizeThreads)
    k_resize(const ImgDesc *__restrict__ descs, const uint8_t *__restrict__ planes, RawSrc raw,
             const float *__restrict__ lut, const int64_t *__restrict__ labels,
             float *__restrict__ out, int64_t *__restrict__ out_labels,
             const int32_t *__restrict__ status, int n, int ks_h, int ks_v, int row_bytes, int oh,
             int ow, const ldt_crop *__restrict__ boxes, const ldt_window *__restrict__ wins, F... fmt_pack) {
  static_assert(sizeof...(F) <= 1, "at most the format");
  const int NB = (oh + kBandRows - 1) / kBandRows, NT = (ow + kTileCols - 1) / kTileCols;
  const int L = blockIdx.x;
  const int g = L / (8 * NB * NT), rr = L % (8 * NB * NT);
  const int img = g * 8 + (rr % 8);
  const int band = (rr / 8) / NT, tile = (rr / 8) % NT;
  if (img >= n) return;
  if (SRC == 0 && status[img] != 0) return;
  StreamTile t;
  t.img = img;
  t.band = band;
  t.tile = tile;
  t.oh = oh;
  t.ow = ow;
  t.oimg = img;
  t.obase = 0;
  if (SRC == 0) {
    t.desc = &descs[img];
    t.src = planes;
    t.src_stride = t.src_w = 0;
    t.W = descs[img].width;
    t.H = descs[img].height;
  } else {
    t.desc = nullptr;
    t.src = raw.base;
    t.src_stride = raw.cell_stride;
    t.src_w = t.W = raw.w;
    t.H = raw.h;
  }
  t.top = t.left = t.flip = 0; // BOX only
  t.rh = oh, t.rw = ow, t.wtop = t.wleft = 0; // BOX == 2 only
  if (BOX == 2) {
    if (SRC == 0) {
      const ImgDesc &d = descs[img];
      t.rh = d.res_h;
      t.rw = d.res_w;
      t.wtop = d.win_top;
      t.wleft = d.win_left;
    } else {
      const ldt_window v = wins[img];
      t.rh = v.res_h;
      t.rw = v.res_w;
      t.wtop = v.top;
      t.wleft = v.left;
    }
  }
  if (BOX && SRC == 0) {
    const ImgDesc &d = descs[img];
    t.W = d.box_w;
    t.H = d.box_h;
    t.top = d.box_top;
    t.left = d.box_left;
    t.flip = d.flip;
  } else if (BOX && !(BOX == 2 && boxes == nullptr)) {
    const ldt_crop b = boxes[img];
    t.W = b.width;
    t.H = b.height;
    t.top = b.top;
    t.left = b.left;
    t.flip = b.flip;
  }
  t.labels = labels;
  t.out_labels = out_labels;
  resize_stream_tile<SRC, FILT, sizeof...(F) == 1>(t, lut, out, fmt_arg(fmt_pack...), ks_h, ks_v, row_bytes);
}

namespace {

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
  static_assert(sizeof...(F) <= 1, "at most the format");
  const int L = blockIdx.x;
  int img, view;
  StreamTile t;
  t.obase = 0; // SIZED: first element of the view's dense block
  if constexpr (SIZED) {
    // oh, ow arrive as the widest view's (unused); the view's own replace them
    const ViewWork vw = view_work(geom, order, L);
    img = vw.img;
    view = vw.view;
    t.band = vw.band;
    t.tile = vw.tile;
    oh = geom.g[view].oh;
    ow = geom.g[view].ow;
    t.obase = geom.g[view].base;
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
    t.band = (rr / 8) / NT;
    t.tile = (rr / 8) % NT;
  }
  if (img >= n || view >= views) return;
  if (status[img] != 0) return;
  const int64_t vimg = (int64_t)view * n + img; // the view table's index
  // the output image: in a sized call the row inside the view's own block at obase
  t.oimg = SIZED ? (int64_t)img : vimg;
  const ViewDesc vd = vtab[vimg];
  t.desc = &descs[img];
  t.src = planes;
  t.src_stride = t.src_w = 0;
  t.W = vd.box_w, t.H = vd.box_h, t.top = vd.box_top, t.left = vd.box_left, t.flip = vd.flip;
  t.rh = vd.res_h, t.rw = vd.res_w, t.wtop = vd.win_top, t.wleft = vd.win_left;
  t.oh = oh;
  t.ow = ow;
  t.img = img;
  t.labels = view == 0 ? labels : nullptr; // the label is written once per image, by view 0
  t.out_labels = out_labels;
  resize_stream_tile<0, FILT, sizeof...(F) == 1>(t, lut, out, fmt_arg(fmt_pack...), ks_h, ks_v, row_bytes);
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

// ---------------------------------------------------------------------------
// The instantiations, described once: entry i of each table is the kernel
// whose template arguments are the digits of i. Choosing a call's kernel and
// raising the dynamic-LDS limit of all of them both read these tables.
// ---------------------------------------------------------------------------
static_assert(kFilterBilinear == 0 && kFilterBicubic == 1, "the filter is a table index");
constexpr int kResizeKernels = 2 * 3 * 2 * 2, kViewsKernels = 2 * 2 * 2;
constexpr int resize_index(int src, int box, int filter, bool fmt) { return ((src * 3 + box) * 2 + filter) * 2 + fmt; }
constexpr int views_index(int filter, bool sized, bool fmt) { return (filter * 2 + sized) * 2 + fmt; }

template <int I>
const void *resize_kernel() {
  constexpr int SRC = I / 12, BOX = I / 4 % 3, FILT = I / 2 % 2;
  static_assert(resize_index(SRC, BOX, FILT, I % 2) == I, "resize_index");
  if constexpr (I % 2) return reinterpret_cast<const void *>(&k_resize<SRC, BOX, FILT, OutFmt>);
  else return reinterpret_cast<const void *>(&k_resize<SRC, BOX, FILT>);
}
template <int I>
const void *views_kernel() {
  constexpr int FILT = I / 4;
  constexpr bool SIZED = I / 2 % 2;
  static_assert(views_index(FILT, SIZED, I % 2) == I, "views_index");
  if constexpr (I % 2) return reinterpret_cast<const void *>(&k_resize_views<FILT, SIZED, OutFmt>);
  else return reinterpret_cast<const void *>(&k_resize_views<FILT, SIZED>);
}
template <int... I>
std::array<const void *, sizeof...(I)> resize_kernels(std::integer_sequence<int, I...>) {
  return {resize_kernel<I>()...};
}
template <int... I>
std::array<const void *, sizeof...(I)> views_kernels(std::integer_sequence<int, I...>) {
  return {views_kernel<I>()...};
}
const auto kResizeTab = resize_kernels(std::make_integer_sequence<int, kResizeKernels>());
const auto kViewsTab = views_kernels(std::make_integer_sequence<int, kViewsKernels>());

// Allow up to the full 160 KiB of LDS (wide images and boxes).
hipError_t stream_lds_attr() {
  static hipError_t once = [] {
    hipError_t e = hipSuccess;
    auto raise = [&e](const void *f) {
      if (e == hipSuccess) e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    };
    for (const void *f : kResizeTab) raise(f);
    for (const void *f : kViewsTab) raise(f);
    return e;
  }();
  return once;
}

// The body's LDS (resize_stream_tile): the table, the coefficient rows and
// bounds of a full tile and a band, two staged rows.
size_t stream_lds_bytes(int ks_h, int ks_v, int row_bytes, int ow) {
  const int tcols = ow < kTileCols ? ow : kTileCols;
  return 3072 + (size_t)4 * (tcols * ks_h + kBandRows * ks_v + 2 * tcols + 2 * kBandRows) + 2 * (size_t)row_bytes;
}

int round_row_bytes(int w) { return ((w * 3 + 15) / 16) * 16; }

template <typename T>
struct exactly {
  using type = T;
};

// Launches table entry `kern` with the arguments of `signature`, the FMT
// instantiation of its family: the arguments convert to exactly the kernel's
// parameter types, and an instantiation without the trailing format does not
// read it. ks_h, ks_v, w (the widest source) and ow size the LDS.
template <typename... P>
hipError_t stream_launch(void (*signature)(P...), const void *kern, int64_t groups, int ks_h, int ks_v, int w, int ow,
                         hipStream_t s, typename exactly<P>::type... a) {
  (void)signature;
  const size_t lds = stream_lds_bytes(ks_h, ks_v, round_row_bytes(w), ow);
  if (lds > 64 * 1024) {
    hipError_t e = stream_lds_attr();
    if (e != hipSuccess) return e;
  }
  void *args[] = {static_cast<void *>(&a)...};
  (void)hipLaunchKernel(kern, dim3((unsigned)groups), dim3(kResizeThreads), args, lds, s);
  return hipGetLastError();
}

} // namespace

// Workgroups of the streaming kernels: images in groups of 8, views, bands, column tiles.
int64_t resize_views_groups(int n, int views, int oh, int ow) {
  const int64_t nb = (oh + kBandRows - 1) / kBandRows, nt = (ow + kTileCols - 1) / kTileCols;
  return (int64_t)((n + 7) / 8) * 8 * views * nb * nt;
}

hipError_t launch_resize_jpeg(const DevPlan &p, const DevWork &w, float *out, int64_t *out_labels,
                              hipStream_t s, int box, int filter) {
  if (p.n == 0) return hipSuccess;
  // box 1: the descriptors carry crops; max_w and the tap counts are the boxes'.
  // box 2: and windows; the tap counts are those of (box -> res)
  // filter: the planner's tap counts are that filter's
  const void *kern = kResizeTab[resize_index(0, box == 2 ? 2 : box ? 1 : 0, filter == kFilterBicubic, !fmt_default(p.ro.fmt))];
  return stream_launch(&k_resize<0, 0, 0, OutFmt>, kern, resize_views_groups(p.n, 1, p.ro.oh, p.ro.ow), p.max_ks_h,
                       p.max_ks_v, p.max_w, p.ro.ow, s, p.descs, w.planes, RawSrc{nullptr, 0, 0, 0}, p.lut, p.labels, out,
                       out_labels, w.status, p.n, p.max_ks_h, p.max_ks_v, round_row_bytes(p.max_w), p.ro.oh, p.ro.ow,
                       nullptr, nullptr, p.ro.fmt);
}

hipError_t launch_resize_raw(const uint8_t *hwc, int64_t cell_stride, int n, int h, int w,
                             const float *lut, int oh, int ow, float *out, hipStream_t s,
                             const ldt_crop *boxes, int box_w, int box_h, const ldt_window *wins, int win_ks_h,
                             int win_ks_v, int filter, OutFmt fmt) {
  if (n == 0) return hipSuccess;
  // boxes: the widest and tallest box size the taps and the staged row;
  // wins: the caller's taps, the most of any row's (source -> res)
  const int sw = boxes ? box_w : w, sh = boxes ? box_h : h;
  const int ks_h = wins ? win_ks_h : resample_ksize_host(sw, ow, filter),
            ks_v = wins ? win_ks_v : resample_ksize_host(sh, oh, filter);
  const void *kern = kResizeTab[resize_index(1, wins ? 2 : boxes ? 1 : 0, filter == kFilterBicubic, !fmt_default(fmt))];
  return stream_launch(&k_resize<1, 0, 0, OutFmt>, kern, resize_views_groups(n, 1, oh, ow), ks_h, ks_v, sw, ow, s,
                       nullptr, nullptr, RawSrc{hwc, cell_stride, h, w}, lut, nullptr, out, nullptr, nullptr, n, ks_h,
                       ks_v, round_row_bytes(sw), oh, ow, boxes, wins, fmt);
}

hipError_t launch_resize_views(const DevPlan &p, const DevWork &w, float *out, int64_t *out_labels, hipStream_t s,
                               int filter, int order) {
  if (p.n == 0) return hipSuccess;
  const bool sized = p.geom != nullptr;
  const void *kern = kViewsTab[views_index(filter == kFilterBicubic, sized, !fmt_default(p.ro.fmt))];
  if (sized) {
    // per-view sizes: the grid is the table's sum, the LDS that of the widest view
    const ViewGeomTab &t = *p.geom;
    if (t.views != p.n_views || t.views < 1 || p.views == nullptr || t.total < 1 || t.total > 0x7FFFFFFF ||
        t.groups != (p.n + 7) / 8)
      return hipErrorInvalidValue;
    return stream_launch(&k_resize_views<0, true, OutFmt>, kern, t.total, p.max_ks_h, p.max_ks_v, p.max_w, t.max_ow, s,
                         p.descs, p.views, w.planes, p.lut, p.labels, out, out_labels, w.status, p.n, p.n_views, order,
                         p.max_ks_h, p.max_ks_v, round_row_bytes(p.max_w), 0, t.max_ow, t, p.ro.fmt);
  }
  const int64_t groups = resize_views_groups(p.n, p.n_views, p.ro.oh, p.ro.ow);
  if (p.n_views < 1 || p.n_views > kMaxViews || p.views == nullptr || groups > 0x7FFFFFFF) return hipErrorInvalidValue;
  return stream_launch(&k_resize_views<0, false, OutFmt>, kern, groups, p.max_ks_h, p.max_ks_v, p.max_w, p.ro.ow, s,
                       p.descs, p.views, w.planes, p.lut, p.labels, out, out_labels, w.status, p.n, p.n_views, order,
                       p.max_ks_h, p.max_ks_v, round_row_bytes(p.max_w), p.ro.oh, p.ro.ow, NoGeom(), p.ro.fmt);
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
