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
// Both: one workgroup per (output image, tile of kColorRows rows); a lane takes
// four consecutive pixels of a row, one dword from each of the three planes
// when the row's address allows it (w a multiple of 4, or a row that happens to
// start aligned), single bytes at a tail or an unaligned row. The geometry of
// a workgroup's view comes from ColorGeom, a kernel argument: finding the view
// is a walk over at most 16 scalars, uniform over the workgroup. Rows whose
// status is not 0 are skipped: launch_fill_failed* zeroes them afterwards.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ldt_color.hpp"
#include "ldt_device.hpp"
#include "ldt_kernels.hpp"

#pragma clang fp contract(off)

namespace ldt {

namespace {

constexpr int kColorThreads = 256;

// The work of workgroup L: its output image, view and rows.
struct ColorWork {
  int img, view, y0, rows, oh, ow;
  int64_t base; // first element of the image's three planes (bytes in the workspace)
};

__device__ __forceinline__ ColorWork color_work(const ColorGeom &g, int L, int n) {
  ColorWork k;
  k.img = L / g.tiles;
  const int t = L - k.img * g.tiles;
  int view = 0;
#pragma unroll
  for (int u = 1; u < kMaxViews; ++u)
    if (u < g.views && t >= g.tile0[u]) view = u;
  k.view = view;
  k.oh = g.oh[view];
  k.ow = g.ow[view];
  k.y0 = (t - g.tile0[view]) * kColorRows;
  k.rows = min(kColorRows, k.oh - k.y0);
  k.base = g.base[view] + (int64_t)k.img * 3 * k.oh * k.ow;
  return k;
}

// Four consecutive pixels of one plane row at p (cnt of them inside the row),
// as bytes of a dword: one load when p is dword-aligned and the quad is whole.
__device__ __forceinline__ uint32_t load_quad(const uint8_t *p, int cnt) {
  if (cnt == 4 && (((uintptr_t)p) & 3) == 0) return *reinterpret_cast<const uint32_t *>(p);
  uint32_t v = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (e < cnt) v |= (uint32_t)p[e] << (8 * e);
  return v;
}

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
    if (fmt.layout == kLayoutNHWC) {
      // twelve consecutive elements
      uint8_t *q = ob + at * 3 * es;
      if (cnt == 4 && (((uintptr_t)q) & (4 * es - 1)) == 0) {
        fmt_store4(q, es, v[0][0], v[1][0], v[2][0], v[0][1]);
        fmt_store4(q + 4 * es, es, v[1][1], v[2][1], v[0][2], v[1][2]);
        fmt_store4(q + 8 * es, es, v[2][2], v[0][3], v[1][3], v[2][3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < cnt) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) fmt_store1(q + (3 * e + ch) * es, es, v[ch][e]);
          }
      }
    } else {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        uint8_t *q = ob + (ch * plane + at) * es;
        if (cnt == 4 && (((uintptr_t)q) & (4 * es - 1)) == 0) {
          fmt_store4(q, es, v[ch][0], v[ch][1], v[ch][2], v[ch][3]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (e < cnt) fmt_store1(q + e * es, es, v[ch][e]);
        }
      }
    }
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

} // namespace ldt
