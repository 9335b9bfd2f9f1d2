// ldt_augment.hip — the auto-augment stage of a call with augments
// (ldt_set_augments): up to LDT_MAX_AUG_OPS ops per output image from the op
// set of TrivialAugmentWide / RandAugment / AutoAugment, on the resized uint8
// image, then the erase box, ToTensor / Normalize and the store in the call's
// dtype and layout. The arithmetic is ldt_augment.hpp's, which the CPU check
// holds against Pillow itself.
//
// The resize of such a call runs as it does for a uint8 contiguous output and
// writes its Pillow-exact bytes into workspace A, laid out like that output
// (view-major, dense planes whose rows are `w` bytes). An op reads the whole
// image it changes (the affine gather, the 3 x 3 of sharpness, the statistics),
// so the ops ping-pong between A and a second workspace B of the same layout.
// With K the largest count of the call the stage is K slots (one when K is 0):
//
//   slot alignment  an entry with k ops runs op j in slot K - k + j, so its
//                   last op lands in the last slot; the slots before skip it
//                   without a copy pass. Op j reads A when j is even and B
//                   when it is odd, and writes the other one
//   k_aug_stats     launched for a slot only when some entry's op in it is
//                   contrast, autocontrast or equalize: one workgroup per
//                   entry, which reads the image in the state it has before
//                   that op, sums L (contrast) or builds the three 256-bin
//                   histograms in LDS (integer adds: the order of arrival does
//                   not matter) and writes the rounded L mean or the 768-byte
//                   table to the entry's record in `stats`
//   k_aug_apply     one workgroup per (output image, tile of kColorRows rows),
//                   geometry from ColorGeom as in the photometric stage. It
//                   runs the slot's op of every entry active in it; in every
//                   slot but the last it writes uint8 planes to the other
//                   workspace, in the last it applies the erase box, the
//                   768-entry table and the formatted store. Entries without
//                   ops are a plain table store in that last launch
//
// Rows whose status is not 0 are skipped: launch_fill_failed* zeroes them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ldt_augment.hpp"
#include "ldt_color_dev.hpp"
#include "ldt_device.hpp"
#include "ldt_kernels.hpp"

#pragma clang fp contract(off)

namespace ldt {

namespace {

// The op of entry `e` (count cnt) that runs in `slot` of K: its index, or -1.
__device__ __forceinline__ int aug_slot_op(int cnt, int slot, int K) {
  const int j = slot - (K - cnt);
  return j >= 0 && j < cnt ? j : -1;
}

__global__ void __launch_bounds__(kColorThreads)
    k_aug_stats(const ldt_aug *__restrict__ augs, const uint8_t *__restrict__ wsa, const uint8_t *__restrict__ wsb,
                uint8_t *__restrict__ stats, const int32_t *__restrict__ status, int n, const ColorGeom g, int slot,
                int K) {
  // one histogram per wave, so that waves do not contend for a bin
  __shared__ uint32_t s_hist[kColorThreads / 64][768];
  __shared__ uint32_t s_sum;
  __shared__ uint8_t s_lut[768];
  const int entry = blockIdx.x;
  const int img = entry / g.views, view = entry - img * g.views;
  if (img >= n || status[img] != 0) return;
  const ldt_aug *e = augs + entry;
  const int j = aug_slot_op(e->count, slot, K);
  if (j < 0) return;
  const int code = e->op[j].code;
  if (!aug_needs_stats(code)) return;
  const int oh = g.oh[view], ow = g.ow[view];
  const int64_t plane = (int64_t)oh * ow;
  const uint8_t *src = ((j & 1) ? wsb : wsa) + g.base[view] + (int64_t)img * 3 * plane;
  uint8_t *st = stats + (int64_t)entry * kAugStatBytes;
  const int Q = (ow + 3) >> 2;
  if (code == kAugContrast) {
    if (threadIdx.x == 0) s_sum = 0;
    __syncthreads();
    uint32_t sum = 0; // at most 255 * 2^20 over the image
    for (int idx = threadIdx.x; idx < oh * Q; idx += kColorThreads) {
      const int row = idx / Q, x = (idx - row * Q) * 4;
      const int cnt = min(4, ow - x);
      const uint8_t *p = src + (int64_t)row * ow + x;
      const uint32_t qr = load_quad(p, cnt), qg = load_quad(p + plane, cnt), qb = load_quad(p + 2 * plane, cnt);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q < cnt) sum += (uint32_t)color_l((qr >> (8 * q)) & 255, (qg >> (8 * q)) & 255, (qb >> (8 * q)) & 255);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(&s_sum, sum);
    __syncthreads();
    if (threadIdx.x == 0)
      *reinterpret_cast<int32_t *>(st + 768) = color_mean_round(s_sum, (uint32_t)(oh * ow));
    return;
  }
  for (int i = threadIdx.x; i < (kColorThreads / 64) * 768; i += kColorThreads) (&s_hist[0][0])[i] = 0;
  __syncthreads();
  uint32_t *hist = s_hist[threadIdx.x >> 6];
  for (int idx = threadIdx.x; idx < oh * Q; idx += kColorThreads) {
    const int row = idx / Q, x = (idx - row * Q) * 4;
    const int cnt = min(4, ow - x);
    const uint8_t *p = src + (int64_t)row * ow + x;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const uint32_t d = load_quad(p + ch * plane, cnt);
      // a quad of one value (a flat region: every lane on one bin) is one add
      if (cnt == 4 && d == (d & 255) * 0x01010101u) {
        atomicAdd(&hist[256 * ch + (d & 255)], 4u);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (q < cnt) atomicAdd(&hist[256 * ch + ((d >> (8 * q)) & 255)], 1u);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 768; i += kColorThreads) {
    uint32_t v = 0;
#pragma unroll
    for (int wv = 0; wv < kColorThreads / 64; ++wv) v += s_hist[wv][i];
    s_hist[0][i] = v; // bin i is this thread's alone
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    if (code == kAugAutoContrast) aug_autocontrast_lut(&s_hist[0][256 * threadIdx.x], &s_lut[256 * threadIdx.x]);
    else aug_equalize_lut(&s_hist[0][256 * threadIdx.x], &s_lut[256 * threadIdx.x]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 768; i += kColorThreads) st[i] = s_lut[i];
}

// LAST: the stage's last slot, which stores the call's output; otherwise the
// slot writes uint8 planes to the other workspace.
template <bool LAST>
__global__ void __launch_bounds__(kColorThreads)
    k_aug_apply(const ldt_aug *__restrict__ augs, uint8_t *__restrict__ wsa, uint8_t *__restrict__ wsb,
                const uint8_t *__restrict__ stats, const int32_t *__restrict__ status, const float *__restrict__ lut,
                uint8_t *__restrict__ out, OutFmt fmt, int n, const ColorGeom g, int slot, int K) {
  __shared__ uint32_t s_bits[LAST ? 768 : 1]; // the table as element bits
  __shared__ uint8_t s_lut[768];              // the slot's table op
  const ColorWork k = color_work(g, blockIdx.x, n);
  if (k.img >= n || status[k.img] != 0) return;
  const int entry = k.img * g.views + k.view;
  const ldt_aug *e = augs + entry;
  const int j = aug_slot_op(e->count, slot, K);
  if (!LAST && j < 0) return; // not its turn yet: no copy pass
  const int code = j < 0 ? kAugIdentity : e->op[j].code;
  const ldt_aug_op *op = &e->op[j < 0 ? 0 : j];
  const float factor = op->factor;
  const int param = op->param;
  const int es = dtype_bytes(fmt.dtype);
  if (LAST)
    for (int i = threadIdx.x; i < 768; i += kColorThreads)
      s_bits[i] = es == 4   ? reinterpret_cast<const uint32_t *>(lut)[i]
                  : es == 2 ? (uint32_t) reinterpret_cast<const uint16_t *>(lut)[i]
                            : (uint32_t)(i & 255);
  const uint8_t *st = stats + (int64_t)entry * kAugStatBytes;
  const bool table = code == kAugAutoContrast || code == kAugEqualize;
  if (table)
    for (int i = threadIdx.x; i < 768; i += kColorThreads) s_lut[i] = st[i];
  const int mean = code == kAugContrast ? *reinterpret_cast<const int32_t *>(st + 768) : 0;
  int32_t a[6];
  int fill[3];
#pragma unroll
  for (int c = 0; c < 6; ++c) a[c] = op->a[c];
#pragma unroll
  for (int c = 0; c < 3; ++c) fill[c] = op->fill[c];
  const int et = e->erase[0], el = e->erase[1], eh = e->erase[2], ew = e->erase[3];
  __syncthreads();
  const bool odd = j > 0 && (j & 1);
  const uint8_t *src = (odd ? wsb : wsa) + k.base;
  uint8_t *dst = (odd ? wsa : wsb) + k.base;
  const int Q = (k.ow + 3) >> 2;
  const int64_t plane = (int64_t)k.oh * k.ow;
  uint8_t *ob = out + k.base * es; // the image's first element
  for (int idx = threadIdx.x; idx < k.rows * Q; idx += kColorThreads) {
    const int row = idx / Q, x0 = (idx - row * Q) * 4;
    const int y = k.y0 + row;
    const int cnt = min(4, k.ow - x0);
    const int64_t at = (int64_t)y * k.ow + x0; // the quad's first pixel in a plane
    const uint8_t *p = src + at;
    const uint32_t qr = load_quad(p, cnt), qg = load_quad(p + plane, cnt), qb = load_quad(p + 2 * plane, cnt);
    uint32_t v[3][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      int px[3] = {(int)((qr >> (8 * q)) & 255), (int)((qg >> (8 * q)) & 255), (int)((qb >> (8 * q)) & 255)};
      const int x = x0 + q;
      if (q < cnt) {
        if (code == kAugAffine) {
          int xin, yin;
          if (aug_affine_src(a, x, y, k.ow, k.oh, xin, yin)) {
            const uint8_t *s = src + (int64_t)yin * k.ow + xin;
            px[0] = s[0];
            px[1] = s[plane];
            px[2] = s[2 * plane];
          } else {
            px[0] = fill[0];
            px[1] = fill[1];
            px[2] = fill[2];
          }
        } else if (code == kAugSharpness) {
          if (!aug_smooth_is_border(x, y, k.ow, k.oh)) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
              const uint8_t *s = p + ch * plane + q;
              const int up[3] = {s[-k.ow - 1], s[-k.ow], s[-k.ow + 1]};
              const int mid[3] = {s[-1], s[0], s[1]};
              const int down[3] = {s[k.ow - 1], s[k.ow], s[k.ow + 1]};
              px[ch] = color_blend(aug_smooth3x3(up, mid, down), px[ch], factor);
            }
          }
        } else if (table) {
          px[0] = s_lut[px[0]];
          px[1] = s_lut[256 + px[1]];
          px[2] = s_lut[512 + px[2]];
        } else {
          aug_pointwise(code, factor, param, mean, px[0], px[1], px[2]);
        }
      }
      if (LAST) {
        const bool erased = eh != 0 && y >= et && y - et < eh && x >= el && x - el < ew;
        v[0][q] = erased ? 0u : s_bits[px[0]];
        v[1][q] = erased ? 0u : s_bits[256 + px[1]];
        v[2][q] = erased ? 0u : s_bits[512 + px[2]];
      } else {
        v[0][q] = (uint32_t)px[0];
        v[1][q] = (uint32_t)px[1];
        v[2][q] = (uint32_t)px[2];
      }
    }
    if (LAST) store_quad(ob, fmt, es, plane, at, cnt, v);
    else store_quad(dst, OutFmt{kDtypeU8, kLayoutNCHW}, 1, plane, at, cnt, v);
  }
}

} // namespace

hipError_t launch_aug_stats(const ldt_aug *augs, const uint8_t *wsa, const uint8_t *wsb, uint8_t *stats,
                            const int32_t *status, int n, const ColorGeom &g, int slot, int K, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (g.views < 1 || (int64_t)n * g.views > 0x7FFFFFFF || slot < 0 || slot >= K || K > LDT_MAX_AUG_OPS)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_aug_stats, dim3((unsigned)(n * g.views)), dim3(kColorThreads), 0, s, augs, wsa, wsb, stats,
                     status, n, g, slot, K);
  return hipGetLastError();
}

hipError_t launch_aug_apply(const ldt_aug *augs, uint8_t *wsa, uint8_t *wsb, const uint8_t *stats,
                            const int32_t *status, const float *lut, float *out, OutFmt fmt, int n,
                            const ColorGeom &g, int slot, int K, hipStream_t s, bool to_ws) {
  if (n == 0) return hipSuccess;
  if (g.views < 1 || g.tiles < 1 || (int64_t)n * g.tiles > 0x7FFFFFFF || slot < 0 || slot >= (K > 0 ? K : 1) ||
      K < 0 || K > LDT_MAX_AUG_OPS)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)(n * g.tiles)), block(kColorThreads);
  if (!to_ws && slot == (K > 0 ? K : 1) - 1)
    hipLaunchKernelGGL(k_aug_apply<true>, grid, block, 0, s, augs, wsa, wsb, stats, status, lut,
                       reinterpret_cast<uint8_t *>(out), fmt, n, g, slot, K);
  else
    hipLaunchKernelGGL(k_aug_apply<false>, grid, block, 0, s, augs, wsa, wsb, stats, status, lut,
                       reinterpret_cast<uint8_t *>(out), fmt, n, g, slot, K);
  return hipGetLastError();
}

} // namespace ldt
