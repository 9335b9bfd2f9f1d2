// ldt_mix.hip — the mix stage of a call with a mix (ldt_set_mix): MixUp /
// CutMix of every row with its partner row, the last stage before the store,
// and the rows' soft labels. The arithmetic is ldt_mix.hpp's, which the CPU
// check holds against torch itself.
//
// The call is staged: the resize (and the colour or augment stage, when the
// call has one) leaves every row's final uint8 planes in a workspace laid out
// like a uint8 contiguous output. Two kernels follow on the same stream:
//
//   k_mix_apply   one workgroup per (image, tile of kColorRows rows), geometry
//                 from ColorGeom with one view. It holds the float32 ToTensor /
//                 Normalize table in LDS, reads a quad of the row's three planes
//                 and of its partner's, turns bytes into values (+0.0f inside
//                 the byte's own erase box, read from the ldt_aug records: the
//                 byte 0 the augment stage could write there is not the value
//                 0), mixes, converts and stores in the call's dtype and layout.
//                 The record and both status words are read once per workgroup,
//                 so every branch on them is wave-uniform
//   k_mix_labels  launched only with num_classes > 0: one workgroup per row,
//                 lane c writes class c's value from the closed form, so every
//                 element is written once and none needs a zero-fill before
//
// A row whose status is not 0 is skipped (staged_tail zeroes it); its soft row
// is zero. A row whose partner failed is stored unmixed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ldt_color_dev.hpp"
#include "ldt_device.hpp"
#include "ldt_kernels.hpp"
#include "ldt_mix.hpp"

#pragma clang fp contract(off)

namespace ldt {

namespace {

// The workspace that holds entry e's final bytes.
__device__ __forceinline__ const uint8_t *mix_src(const ldt_aug *augs, int e, const uint8_t *wsa, const uint8_t *wsb,
                                                  int src) {
  if (src == kMixSrcByCount) return (augs[e].count & 1) ? wsb : wsa;
  return src == kMixSrcB ? wsb : wsa;
}

__global__ void __launch_bounds__(kColorThreads)
    k_mix_apply(const ldt_mix *__restrict__ mix, const ldt_aug *__restrict__ augs, const uint8_t *__restrict__ wsa,
                const uint8_t *__restrict__ wsb, int src, const int32_t *__restrict__ status,
                const float *__restrict__ lut, uint8_t *__restrict__ out, OutFmt fmt, int n, const ColorGeom g) {
  __shared__ float s_lut[768];
  const ColorWork k = color_work(g, blockIdx.x, n);
  if (k.img >= n || status[k.img] != 0) return;
  for (int i = threadIdx.x; i < 768; i += kColorThreads) s_lut[i] = lut[i];
  const ldt_mix m = mix[k.img];
  const int pi = m.partner;
  const bool solo = status[pi] != 0; // the partner failed: the row as it is
  const float ws = m.w_self, wp = m.w_partner;
  const int bt = m.box[0], bl = m.box[1], bh = solo ? 0 : m.box[2], bw = m.box[3];
  // both rows' erase boxes
  int et = 0, el = 0, eh = 0, ew = 0, pt = 0, pl = 0, ph = 0, pw = 0;
  if (augs) {
    const ldt_aug *e = augs + k.img, *p = augs + pi;
    et = e->erase[0], el = e->erase[1], eh = e->erase[2], ew = e->erase[3];
    pt = p->erase[0], pl = p->erase[1], ph = p->erase[2], pw = p->erase[3];
  }
  const int64_t plane = (int64_t)k.oh * k.ow;
  const uint8_t *xs = mix_src(augs, k.img, wsa, wsb, src) + k.base;
  const uint8_t *ps = mix_src(augs, pi, wsa, wsb, src) + (int64_t)pi * 3 * plane; // one view: g.base[0] == 0
  const int es = dtype_bytes(fmt.dtype);
  const int dtype = fmt.dtype;
  __syncthreads();
  const int Q = (k.ow + 3) >> 2;
  uint8_t *ob = out + k.base * es; // the image's first element
  for (int idx = threadIdx.x; idx < k.rows * Q; idx += kColorThreads) {
    const int row = idx / Q, x0 = (idx - row * Q) * 4;
    const int y = k.y0 + row;
    const int cnt = min(4, k.ow - x0);
    const int64_t at = (int64_t)y * k.ow + x0; // the quad's first pixel in a plane
    uint32_t qx[3], qp[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      qx[ch] = load_quad(xs + ch * plane + at, cnt);
      qp[ch] = solo ? 0u : load_quad(ps + ch * plane + at, cnt);
    }
    uint32_t v[3][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int x = x0 + q;
      const bool xe = mix_in_box(y, x, et, el, eh, ew), pe = mix_in_box(y, x, pt, pl, ph, pw);
      const bool boxed = mix_in_box(y, x, bt, bl, bh, bw);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float xv = xe ? 0.0f : s_lut[256 * ch + ((qx[ch] >> (8 * q)) & 255)];
        const float pv = pe ? 0.0f : s_lut[256 * ch + ((qp[ch] >> (8 * q)) & 255)];
        v[ch][q] = mix_store_bits(solo ? xv : mix_element(xv, pv, ws, wp, boxed), dtype);
      }
    }
    store_quad(ob, fmt, es, plane, at, cnt, v);
  }
}

__global__ void __launch_bounds__(kColorThreads)
    k_mix_labels(const ldt_mix *__restrict__ mix, const int64_t *__restrict__ labels,
                 const int32_t *__restrict__ status, float *__restrict__ soft, int n, int num_classes) {
  const int i = blockIdx.x;
  if (i >= n) return;
  const ldt_mix m = mix[i];
  const bool failed = status[i] != 0, solo = status[m.partner] != 0;
  const int64_t a = labels[i], b = solo ? a : labels[m.partner];
  const float ls = solo ? 1.0f : m.lw_self, lp = solo ? 0.0f : m.lw_partner;
  float *o = soft + (int64_t)i * num_classes;
  for (int c = threadIdx.x; c < num_classes; c += kColorThreads)
    o[c] = failed ? 0.0f : mix_soft_label(c, a, b, ls, lp);
}

} // namespace

hipError_t launch_mix_apply(const ldt_mix *mix, const ldt_aug *augs, const uint8_t *wsa, const uint8_t *wsb, int src,
                            const int32_t *status, const float *lut, float *out, OutFmt fmt, int n,
                            const ColorGeom &g, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (g.views != 1 || g.tiles < 1 || (int64_t)n * g.tiles > 0x7FFFFFFF || fmt.dtype == kDtypeU8 ||
      (src == kMixSrcByCount && !augs) || src < kMixSrcA || src > kMixSrcByCount)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_mix_apply, dim3((unsigned)(n * g.tiles)), dim3(kColorThreads), 0, s, mix, augs, wsa, wsb, src,
                     status, lut, reinterpret_cast<uint8_t *>(out), fmt, n, g);
  return hipGetLastError();
}

hipError_t launch_mix_labels(const ldt_mix *mix, const int64_t *labels, const int32_t *status, float *soft, int n,
                             int num_classes, hipStream_t s) {
  if (n == 0 || num_classes == 0) return hipSuccess;
  if (!labels || !soft || num_classes < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_mix_labels, dim3((unsigned)n), dim3(kColorThreads), 0, s, mix, labels, status, soft, n,
                     num_classes);
  return hipGetLastError();
}

} // namespace ldt
