// ldt_resize4.hip — fused source staging + Pillow BILINEAR Resize((224,224)) +
// ToTensor/Normalize store, one wavefront per band of output rows.
//
// Every wave owns one (image, band) task and runs it alone: it streams the
// band's source rows two at a time, stages them as RGBx dwords in a
// wave-private LDS buffer (raw HWC bytes, or JPEG planes with libjpeg's h2v2
// fancy upsampling and YCbCr->RGB done in registers), computes the rows'
// 224x3 horizontal taps (Pillow Resample.c, 22-bit fixed point; its clip8 can
// never fire on BILINEAR sums, kMaxRowSum below) into a wave-private LDS ring
// of uint8 rows, and finishes every output row whose vertical window is
// complete: vertical taps, the ToTensor[/Normalize] float32 LUT and float4
// stores into the CHW fp32 output. A band's boundary rows that no output row
// reads are neither loaded nor staged nor filtered. There is no
// workgroup barrier after the prologue, so the waves of a CU overlap their
// loads and arithmetic freely; the next row pair is prefetched into registers
// while the current one is computed. The Pillow coefficients (22-bit weights
// and window bounds per output index) are not computed here: they depend only
// on (input size, 224), so the context keeps one table per input size it has
// seen (k_fill_resample, ldt_types.hpp kResamp*) and the waves load them: the
// horizontal ones per lane, the vertical ones through the scalar cache.
//
// 224 x 224 is the default output size and has the instantiations above,
// with the size compiled in. Any other size up to kTileCols columns
// (ldt_set_output_size) runs the GEN variant of the same body, which takes
// the size, the ring row stride and the group count from the launch
// geometry (ldt_geom4.hpp) and its tables from the context's tables for that
// out_w and out_h.
//
// float32 CHW is the default output and has the instantiations above. Any
// other element type or layout (ldt_set_output_format: fp16, bf16, uint8,
// HWC) runs the FMT variant of the same body, one per kernel form, built in
// ldt_resize4_fmt.hip: its table holds the element's bits and its store is
// the formatted one (ldt_device.hpp fmt_store*).
//
// Reference semantics: lance_iterable.py:28-32 (Resize((224,224)), ToTensor),
// :31 (Normalize); jdsample.c h2v2_fancy_upsample, jdcolor.c ycc_rgb_convert,
// Pillow Resample.c ImagingResample (horizontal pass first, uint8 between).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <type_traits>

#include "ldt_device.hpp"
#include "ldt_geom4.hpp"
#include "ldt_kernels.hpp"

namespace ldt {

namespace {

__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Lane l receives lane l-1's value (lane 0 keeps its own): DPP wave_shr:1.
__device__ __forceinline__ uint32_t from_prev_lane(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x138, 0xF, 0xF, false);
}
// Lane l receives lane l+1's value (lane 63 keeps its own): DPP wave_shl:1.
__device__ __forceinline__ uint32_t from_next_lane(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x130, 0xF, 0xF, false);
}

// v_mul_u32_u24 of one byte, or of the low half, of v, taken by the
// instruction's own SDWA source select: one instruction per product. Written
// out because the compiler gets there only for some of them: (v >> 16) & 255
// becomes a v_and_b32_sdwa (WORD_1) feeding a plain multiply, a tap alone in
// its basic block a separate extraction per byte feeding v_mad_u32_u24, and
// the low half of a value known to be below 2^12 a v_and 0xfff feeding a
// multiply. k is always a vector register: gfx950 needs two wait states between
// a VALU write of a scalar register (v_readfirstlane, the v_readlane of a
// spilled one) and a VALU read of it, and the compiler's hazard recognizer
// does not look inside inline asm. A scalar weight is copied by a v_mov the
// compiler sees (one per tap).
template <int B> __device__ __forceinline__ uint32_t mul24_byte(uint32_t v, uint32_t k) {
  static_assert(B >= 0 && B < 4, "byte select");
  uint32_t r;
  asm("v_mul_u32_u24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_%3 src1_sel:DWORD"
      : "=v"(r)
      : "v"(v), "v"(k), "n"(B));
  return r;
}
__device__ __forceinline__ uint32_t mul24_lo16(uint32_t v, uint32_t k) {
  uint32_t r;
  asm("v_mul_u32_u24_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:DWORD" : "=v"(r) : "v"(v), "v"(k));
  return r;
}

// A wave-uniform 64-bit value, pinned to scalar registers: an address built
// on it keeps its uniform part out of the lanes' arithmetic (the compiler
// otherwise folds row * stride into a v_mad_u64_u32 on the lane's pointer).
__device__ __forceinline__ int64_t uniform64(int64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ uint8_t *uniform_ptr(uint8_t *p) {
  return reinterpret_cast<uint8_t *>((uintptr_t)uniform64((int64_t)(uintptr_t)p));
}

// Bits 22..29 of a tap sum, the table index (no clip8: see kMaxRowSum below),
// kept from being merged into the address arithmetic: shift, then one
// v_lshl_add with the table's base, where the merged form is a shift, a mask
// and an add.
__device__ __forceinline__ uint32_t lut_index(int32_t acc) {
  uint32_t i = (uint32_t)acc >> kPrecisionBits;
  asm("" : "+v"(i));
  return i;
}

__device__ __forceinline__ uint32_t rgbx(int r, int g, int b) {
  return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
}

// jdcolor.c ycc_rgb_convert (16-bit fixed point, ONE_HALF in the Cb->G term).
// Every factor fits 24 bits, so the products are v_mul_i32_i24 (full rate)
// rather than the quarter-rate v_mul_lo_u32 the compiler would pick.
__device__ __forceinline__ uint32_t ycc_px(int y, int cb, int cr) {
  const int xcr = cr - 128, xcb = cb - 128;
  const int r = y + ((__mul24(91881, xcr) + 32768) >> 16);
  const int g = y + ((__mul24(-22554, xcb) + 32768 + __mul24(-46802, xcr)) >> 16);
  const int b = y + ((__mul24(116130, xcb) + 32768) >> 16);
  return rgbx(clampi(r, 0, 255), clampi(g, 0, 255), clampi(b, 0, 255));
}

struct Raw16 {
  uint4 a, b, c;
};

__device__ __forceinline__ Raw16 load16_aligned(const uint8_t *p) {
  const uint4 *q = reinterpret_cast<const uint4 *>(p);
  Raw16 r;
  r.a = q[0];
  r.b = q[1];
  r.c = q[2];
  return r;
}

// Bytes [3*x0, 3*x0 + 48) of a row, any alignment, zero past the row end.
__device__ __forceinline__ Raw16 load16_any(const uint8_t *row, int W, int x0) {
  const uint8_t *p = row + 3 * x0;
  uint32_t w[12];
  const int nb = max(0, min(48, 3 * (W - x0)));
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    uint32_t v = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (4 * i + e < nb) v |= (uint32_t)p[4 * i + e] << (8 * e);
    w[i] = v;
  }
  Raw16 r;
  r.a = make_uint4(w[0], w[1], w[2], w[3]);
  r.b = make_uint4(w[4], w[5], w[6], w[7]);
  r.c = make_uint4(w[8], w[9], w[10], w[11]);
  return r;
}

// Staging rows are skewed by 4 dwords per 32 pixels: the horizontal taps of
// neighbouring output columns start ~scale pixels apart, and for 224-wide
// outputs of 512 / 1024 (scale 16/7, 32/7) every 7th lane would otherwise hit
// the same LDS bank (4-5-way conflicts on every tap). Blocks of 8 or 16
// pixels starting at a multiple of 8 stay contiguous and 16-byte aligned.
template <bool SKEW = true> __device__ __forceinline__ int skw(int x) {
  return SKEW ? x + ((x >> 5) << 2) : x;
}

// 16 packed RGB pixels -> 16 RGBx dwords at pixels [x0, x0+16) of a staging
// row. The byte above B is left as whatever follows (the taps read bytes 0..2).
template <bool SKEW>
__device__ __forceinline__ void stage16_raw(const Raw16 &r, uint32_t *row, int x0) {
  const uint32_t w[13] = {r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y, r.b.z, r.b.w,
                          r.c.x, r.c.y, r.c.z, r.c.w, 0u};
  uint32_t px[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int o = 3 * j;
    px[j] = __builtin_amdgcn_alignbyte(w[(o >> 2) + 1], w[o >> 2], (uint32_t)(o & 3));
  }
  uint4 *d = reinterpret_cast<uint4 *>(row + skw<SKEW>(x0));
#pragma unroll
  for (int q = 0; q < 4; ++q) d[q] = make_uint4(px[4 * q], px[4 * q + 1], px[4 * q + 2], px[4 * q + 3]);
}

// One JPEG row pair's registers for the 4:2:0 fast path (lane = 8 pixels).
struct Jpair {
  uint2 y0, y1;        // luma rows 2cy, 2cy+1 (8 px each)
  uint32_t c[2][3];    // chroma comp (Cb, Cr) x row (cy-1, cy, cy+1), 4 samples each
};

__device__ __forceinline__ void bytes6(uint32_t w, int lane, int rc, int s[6]) {
  const uint32_t p = from_prev_lane(w), n = from_next_lane(w);
  s[0] = (int)(p >> 24);
  s[1] = (int)(w & 255);
  s[2] = (int)((w >> 8) & 255);
  s[3] = (int)((w >> 16) & 255);
  s[4] = (int)(w >> 24);
  s[5] = (int)(n & 255);
  // column -1 -> column 0; columns past downsampled_width - 1 -> that column
  // (jdsample.c special first/last columns, context rows replicated)
  s[0] = lane == 0 ? s[1] : s[0];
  int e = s[1];
#pragma unroll
  for (int i = 2; i <= 5; ++i) e = rc == i ? s[i] : e;
#pragma unroll
  for (int i = 2; i <= 5; ++i) s[i] = i > rc ? e : s[i];
}

// ---- packed 16-bit fancy upsampling (SRC 5) ----
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u16x2 as_pk(uint32_t v) { return __builtin_bit_cast(u16x2, v); }

// A chroma row's upsampling context, columns 4*lane-1 .. 4*lane+4 (jdsample.c
// edge rules: column -1 -> column 0, columns past the last one -> the last),
// as six (cb, cr) u16x2 pairs built by v_perm_b32 from the Cb and Cr dwords
// (4 samples each) and the neighbouring lanes', with per-lane byte selectors
// that encode the edge rules once (0x0C selects a zero byte). The fancy
// upsampling's packed 16-bit arithmetic then covers both components at once,
// and each output pixel's (cb, cr) arrives in one register (round 5: 377 ->
// 348 VALU per staged row pair against one component per register,
// standalone c2 resize 0.149 -> 0.146 ms, profiles/r5/resize_cc_r5.txt). Selectors per lane: q[i]
// for i = 1..4 from (M_hi, M_lo) (own samples, clamped to the last valid
// column), q[0] from (previous lane's M_hi, M_lo) (lane 0: its own column 0),
// q[5] from (next lane's M_lo, M_lo or M_hi) (the last valid lane: its own
// last column).
struct CC6 {
  u16x2 q[6];
};

__device__ __forceinline__ void cc_selectors(int lane, int rc, uint32_t sel[6], bool &x_lo) {
  auto pair = [](uint32_t b) { return b | (0x0Cu << 8) | ((b + 1u) << 16) | (0x0Cu << 24); };
  sel[0] = lane == 0 ? pair(0u) : pair(6u);
#pragma unroll
  for (int i = 1; i <= 4; ++i) sel[i] = pair(2u * (uint32_t)(min(i, rc) - 1));
  // q[5]: next lane's column 0 (bytes 4, 5 of (Mn, X)), or own column rc - 1
  // in X = M_lo (rc <= 2) or M_hi
  x_lo = rc <= 2;
  sel[5] = rc == 5 ? pair(4u) : pair(2u * (uint32_t)((rc - 1) & 1));
}

__device__ __forceinline__ CC6 cc_pairs(uint32_t cbw, uint32_t crw, const uint32_t sel[6], bool x_lo) {
  const uint32_t mlo = __builtin_amdgcn_perm(crw, cbw, 0x05010400u); // cb0 cr0 cb1 cr1
  const uint32_t mhi = __builtin_amdgcn_perm(crw, cbw, 0x07030602u); // cb2 cr2 cb3 cr3
  const uint32_t mp = from_prev_lane(mhi), mn = from_next_lane(mlo);
  CC6 r;
  r.q[0] = as_pk(__builtin_amdgcn_perm(mp, mlo, sel[0]));
#pragma unroll
  for (int i = 1; i <= 4; ++i) r.q[i] = as_pk(__builtin_amdgcn_perm(mhi, mlo, sel[i]));
  r.q[5] = as_pk(__builtin_amdgcn_perm(mn, x_lo ? mlo : mhi, sel[5]));
  return r;
}


} // namespace

// The cached tables as constant memory (nothing writes them while a resize
// kernel runs): a wave-uniform read is then a scalar load whatever fences
// lie between it and the kernel's start.
typedef const __attribute__((address_space(4))) int32_t *ResampTab;
__device__ __forceinline__ ResampTab resamp_entry(const int32_t *tab, int size) {
  return (ResampTab)(uintptr_t)(tab + (int64_t)(size - 1) * kResampEntry);
}

// Waves (tasks) per workgroup. Raw sources: two. JPEG sources: four (3 KB
// LUT + 4 x 9,472 B at 512 px with rows, ring and KS sized by the real tap
// counts, 5 of Pillow's 7: 40,960 B, four workgroups in the CU's 160 KB;
// while they were sized by Pillow's capacity, 4 x 11.2 KB, three workgroups
// fit, and 2-wave workgroups of 26 KB fit only 5 per CU and measured
// 0.183 vs 0.150 ms standalone, profiles/r5/resize_rgbx_wg_r5wg.txt). No
// resize workgroup shares a CU with a k_huff_image workgroup usefully: one
// that fits (1 wave, <= 128 VGPRs) slows the decoder's rounds more than it
// gains (profiles/r5/resize_coresident_ab_r5co.txt).
constexpr int kResizeWaves = 2;
constexpr int kResizeWavesJpeg = 4;

// SRC: 0 JPEG planes, 4:2:0 fast staging (resize_fast420 images only);
// 2 JPEG planes, generic staging (the other images); 1 raw HWC rows, 16-byte
// aligned; 3 raw HWC rows, any alignment. Each variant is its own kernel so
// the waitcnt pass never sees another path's loads pending at the loop's
// merge points (that forced a vmcnt(0) ahead of the horizontal taps and
// serialised the prefetch).
// SRC 5: the 4:2:0 fast path on packed 16-bit pairs (the default).
// GEN: the output size is a launch parameter (Geom4 oh, ow <= kTileCols): up
// to four column sets lane + 64q per row, ceil(ow / 4) four-column groups in
// the vertical pass, a ring row stride of ow rounded up to 4 whose padding
// columns hold zeros and are never stored, and stores that fall back to
// single floats when ow % 4 != 0 takes the rows off 16-byte alignment. `resamp`
// is then the horizontal table (rows of ow entries), g.tab_v the vertical
// one. Without GEN the size is kOut x kOut at compile time, as before.
//
// FMT (ldt_set_output_format, every call whose format is not float32 CHW): the
// LDS table holds the output element's bits (float32, the host-rounded 16-bit
// table widened to dwords, or the byte itself for uint8), and the store takes
// the format (in g.vec4's place), uniform over the launch: in CHW a lane's four columns are
// one 16-, 8- or 4-byte store where that address is aligned, in HWC the RGBx
// lane's 12 consecutive elements are three of them, and the raw source's
// per-channel items store their elements one by one. Without FMT none of it
// is compiled in.
template <int SRC, int KS, bool GEN, bool FMT = false>
__device__ __forceinline__ void resize4_body(const ImgDesc *__restrict__ descs,
                                             const uint8_t *__restrict__ planes, RawSrc raw,
                                             const float *__restrict__ lut,
                                             const int32_t *__restrict__ resamp,
                                             const int64_t *__restrict__ labels,
                                             float *__restrict__ out,
                                             int64_t *__restrict__ out_labels,
                                             const int32_t *__restrict__ status, const Geom4 &g) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  // Skewed staging for raw rows (c5: 4-5-way tap conflicts otherwise, and the
  // kernel is LDS-bound). JPEG rows stay plain (the
  // skew's per-tap selects took k_resize4<5,7> to 190 VGPRs, 2 waves per
  // SIMD, 0.153 -> 0.175 ms at c2 with half the bank conflicts; blocked rows
  // with a halo copy, 2-way banks at 148 VGPRs, measured 0.155 vs 0.152 ms).
  constexpr bool kJpeg = SRC == 0 || SRC == 2 || SRC == 5;
  constexpr bool kSkew = !kJpeg;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // output height, width, ring row stride, four-column groups: constants unless GEN
  const int OH = GEN ? g.oh : kOut, OW = GEN ? g.ow : kOut, OWS = GEN ? g.ows : kOut;
  const int NG = GEN ? (g.ows >> 2) : kOut / 4;
  float *s_lut = reinterpret_cast<float *>(smem);
  const uint32_t *s_bits = reinterpret_cast<const uint32_t *>(smem); // FMT: the element's bits
  const int es = FMT ? dtype_bytes(g.vec4 & 255) : 4;                // FMT: bytes per element
  const bool nhwc = FMT && (g.vec4 >> 8) == kLayoutNHWC;             // FMT: HWC element order
  uint8_t *outb = reinterpret_cast<uint8_t *>(out);
  if constexpr (FMT) {
    uint32_t *sb = reinterpret_cast<uint32_t *>(smem);
    for (int i = tid; i < 768; i += (int)blockDim.x)
      sb[i] = es == 4   ? reinterpret_cast<const uint32_t *>(lut)[i]
              : es == 2 ? (uint32_t) reinterpret_cast<const uint16_t *>(lut)[i]
                        : (uint32_t)(i & 255);
  } else {
    for (int i = tid; i < 768; i += (int)blockDim.x) s_lut[i] = lut[i];
  }
  __syncthreads(); // the only workgroup barrier
  // wave-uniform task: descriptor loads become scalar loads into SGPRs
  const int task = __builtin_amdgcn_readfirstlane((int)blockIdx.x * g.wpg + wave);
  if (task >= g.ntask) return;
  const int img = task / g.nbands, band = task - img * g.nbands;
  if (kJpeg && status[img] != 0) {
    // a failed image's band: zeros (and label -100), by one of the launches
    const int oy0 = band * g.bh, nb = min(g.bh, OH - oy0);
    if (!g.fill || nb <= 0) return;
    if (band == 0 && lane == 0 && out_labels != nullptr) out_labels[img] = -100;
    if constexpr (FMT) {
      // the band's bytes: one run in HWC, one per channel plane in CHW
      if (nhwc) {
        fmt_zero_bytes(outb + (((int64_t)img * OH + oy0) * OW * 3) * es, (int64_t)nb * OW * 3 * es, lane, 64);
      } else {
        for (int c = 0; c < 3; ++c)
          fmt_zero_bytes(outb + ((((int64_t)img * 3 + c) * OH + oy0) * OW) * es, (int64_t)nb * OW * es, lane, 64);
      }
      return;
    }
    if constexpr (GEN) {
      // the band's nb * ow floats of each channel plane; float4s only where
      // the planes keep 16-byte alignment
      for (int c = 0; c < 3; ++c) {
        float *o = out + (((int64_t)img * 3 + c) * OH + oy0) * OW;
        const int per = nb * OW;
        if (g.vec4) {
          for (int i = lane; i < per / 4; i += 64) reinterpret_cast<float4 *>(o)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
          for (int i = lane; i < per; i += 64) o[i] = 0.f;
        }
      }
      return;
    }
    float4 *o = reinterpret_cast<float4 *>(out + (int64_t)img * 3 * kOut * kOut + oy0 * kOut);
    const int per = nb * kOut / 4; // float4s of the band in one channel plane
    for (int c = 0; c < 3; ++c)
      for (int i = lane; i < per; i += 64) o[c * (kOut * kOut / 4) + i] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  if (kJpeg && resize_fast420(descs[img]) != (SRC == 0 || SRC == 5)) return;
  int W, H;
  if constexpr (kJpeg) {
    W = descs[img].width;
    H = descs[img].height;
  } else {
    W = raw.w;
    H = raw.h;
  }
  const int oy0 = band * g.bh;
  const int nb = min(g.bh, OH - oy0);
  if (nb <= 0) return;
  if (band == 0 && lane == 0 && labels != nullptr) out_labels[img] = labels[img];

  uint8_t *wbase = smem + 3072 + wave * g.wave_bytes;
  uint32_t *stg = reinterpret_cast<uint32_t *>(wbase);               // 2 * spad dwords
  // the intermediate ring: JPEG sources keep RGBx dwords per column (one
  // 4-byte store per column and row, one 16-byte read of 4 columns per
  // vertical tap); raw sources three byte planes (their larger rings would
  // cost a workgroup per CU as dwords)
  constexpr bool kRgbx = kJpeg;
  uint8_t *ring = wbase + 8 * g.spad;                                // (kRgbx ? 4 : 3) * ring * 224
  // only with Geom4::vcalc:
  int32_t *kv = reinterpret_cast<int32_t *>(ring + (kRgbx ? 4 : 3) * g.ring * OWS); // kKvRows * ks_v
  int32_t *vb = kv + kKvRows * g.ks_v;                               // kKvRows * 2
  const int ks_v = g.ks_v, RING = g.ring;

  // horizontal weights of this lane's output columns, in registers:
  // q = 0..2 -> column lane + 64q of both rows; q = 3 -> column 192 + lane%32
  // of row (lane / 32); GEN: q = 0..3 -> column lane + 64q of both rows, a
  // column past the output takes the last one's (its result is not used)
  // KS is the batch's real tap count (resample_taps_host), not Pillow's
  // capacity; the table rows hold zeros past a narrower image's own count
  int32_t wgt[4][KS];
  int xm[4];
  {
    const int4 *th = reinterpret_cast<const int4 *>(resamp + (int64_t)(W - 1) * (GEN ? OW * kResampRow : kResampEntry));
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int ox = GEN ? min(lane + 64 * q, OW - 1) : q < 3 ? lane + 64 * q : 192 + (lane & 31);
      constexpr int kQuads = (2 + KS + 3) / 4;
      int32_t rw[4 * kQuads];
#pragma unroll
      for (int i = 0; i < kQuads; ++i) {
        const int4 v = th[ox * (kResampRow / 4) + i];
        rw[4 * i] = v.x;
        rw[4 * i + 1] = v.y;
        rw[4 * i + 2] = v.z;
        rw[4 * i + 3] = v.w;
      }
      xm[q] = rw[0];
#pragma unroll
      for (int t = 0; t < KS; ++t) wgt[q][t] = rw[2 + t];
    }
  }
  // skewed staging address of each window start, and the first tap past a skew step
  int xsk[4], xcr[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    xsk[q] = skw<kSkew>(xm[q]);
    xcr[q] = 32 - (xm[q] & 31);
  }
  // vertical coefficients: the band's rows of this height's table entry, one
  // row in (scalar) registers at a time; a height past the cache's limit
  // computes its own (kv, vb)
  const bool vtab = GEN ? resamp_cached(H, OH, g.vmax_in) : H <= kResampMaxSize;
  const ResampTab tv = GEN ? (ResampTab)(uintptr_t)(g.tab_v + ((int64_t)(H - 1) * OH + oy0) * kResampRow)
                           : resamp_entry(resamp, H) + oy0 * kResampRow;
  // band source rows
  int ya, yb;
  if (vtab) {
    ya = tv[0];
    yb = tv[(nb - 1) * kResampRow] + tv[(nb - 1) * kResampRow + 1];
  } else {
    int32_t kk[32];
    int ymin_a, ymin_b;
    resample_coeffs_one(H, OH, oy0, 0, kk, &ymin_a);
    const int cnt_b = resample_coeffs_one(H, OH, oy0 + nb - 1, 0, kk, &ymin_b);
    ya = ymin_a;
    yb = ymin_b + cnt_b;
  }
  const int ya0 = kJpeg ? (ya & ~1) : ya;

  // vertical-pass items: 168 dwords (3 channels x 56 groups of 4 columns);
  // GEN: 3 x NG <= 192
  int vc[3], vo[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int it = min(lane + 64 * i, 3 * NG - 1);
    vc[i] = it / NG;
    vo[i] = (it - vc[i] * NG) * 4;
  }

  // JPEG fast path: 4:2:0 with both chroma planes fancy-upsampled, W <= 512
  constexpr bool fast420 = SRC == 0 || SRC == 5;
  constexpr bool kPk = SRC == 5; // packed 16-bit fancy upsampling, (cb, cr) pairs
  int rc = 5, cdh = 1;
  // plane geometry copied to registers once: the wave fences in process()
  // would otherwise make every fetch reload it (a dependent global round trip
  // per plane load, which serialised the prefetch)
  int64_t po0 = 0, po1 = 0, po2 = 0;
  int ps0 = 0, ps1 = 0;
  const ImgDesc *dp = nullptr;
  const uint8_t *raw_cell = nullptr;
  uint32_t csel[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  bool cx_lo = false;
  constexpr bool raw_al16 = SRC == 1;
  if constexpr (kJpeg) {
    dp = descs + img;
    const ImgDesc &d = *dp;
    const int dw = d.cdw[1];
    rc = lane == (dw - 1) / 4 ? (dw - 1) % 4 + 1 : 5;
    cdh = d.cdh[1];
    if constexpr (kPk) cc_selectors(lane, rc, csel, cx_lo);
    po0 = d.plane_off[0];
    po1 = d.plane_off[1];
    po2 = d.plane_off[2];
    ps0 = d.plane_stride[0];
    ps1 = d.plane_stride[1];
  } else {
    raw_cell = raw.base + (int64_t)img * raw.cell_stride;
  }

  // ---- prefetch helpers ----
  struct Pre {
    Jpair jp;
    Raw16 r0, r1;
  } pa;
  // need0, need1 (wave-uniform): whether some output row of the band reads
  // row y, row y + 1 of the pair. A JPEG band stages whole pairs from the even
  // row at or below its first row ya to its end yb, so the first pair's row
  // y < ya and the last pair's row y + 1 >= yb (yb <= H) lie in no vertical
  // window: they are not loaded, staged or filtered, and their ring slots keep
  // what they held (tools/checks/trim_check.cpp). The packed staging skips the
  // row's loads as well; the 32-bit cross-check staging (SRC 0) computes both
  // rows together and only skips the row's horizontal jobs.
  auto fetch = [&](Pre &pf, int y, bool need0, bool need1) {
    Jpair &jp = pf.jp;
    if constexpr (kJpeg) {
      if constexpr (fast420) {
        const bool ld0 = kPk ? need0 : true, ld1 = kPk ? need1 : y + 1 < H;
        // a row's address: wave-uniform (scalar registers) plus the lane's 32-bit offset
        const int x0 = lane * 8;
        const uint8_t *py = planes + uniform64(po0 + (int64_t)y * ps0);
        if (ld0) jp.y0 = x0 < W ? *reinterpret_cast<const uint2 *>(py + (uint32_t)x0) : make_uint2(0, 0);
        if (ld1) jp.y1 = x0 < W ? *reinterpret_cast<const uint2 *>(py + ps0 + (uint32_t)x0) : make_uint2(0, 0);
        if (!kPk && !ld1) jp.y1 = make_uint2(0, 0);
        const int cy = y >> 1;
        const int rows[3] = {max(cy - 1, 0), cy, min(cy + 1, cdh - 1)};
        const int cx0 = lane * 4;
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int r = 0; r < 3; ++r)
            // the context row above serves row y only, the one below row y + 1
            // (the 32-bit staging computes both rows and loads all three)
            if (!kPk || r == 1 || (r ? ld1 : ld0)) {
              const uint8_t *pc = planes + uniform64((c ? po2 : po1) + (int64_t)rows[r] * ps1);
              jp.c[c][r] = cx0 < ps1 ? *reinterpret_cast<const uint32_t *>(pc + (uint32_t)cx0) : 0u;
            }
      }
    } else {
      if constexpr (raw_al16) {
        const int x0 = lane * 16;
        if (x0 < W) {
          pf.r0 = load16_aligned(raw_cell + (int64_t)y * W * 3 + 3 * x0);
          if (need1) pf.r1 = load16_aligned(raw_cell + (int64_t)(y + 1) * W * 3 + 3 * x0);
        }
      }
    }
  };

  // ---- staging of one row pair into stg[0..spad) / stg[spad..2 spad) ----
  auto stage = [&](const Pre &pf, int y, bool need0, bool need1) {
    const Jpair &jp = pf.jp;
    uint32_t *s0 = stg, *s1 = stg + g.spad;
    if constexpr (kJpeg) {
      const ImgDesc &d = *dp;
      if constexpr (kPk) {
        // h2v2 fancy upsampling on (cb, cr) pairs, then jdcolor.c
        // ycc_rgb_convert with the pair in one register: each channel's value
        // before the >> 16, with Y << 16 and the -128 offsets folded into
        // constants (y + ((91881 (cr - 128) + 32768) >> 16) = (Y16 + 91881 cr
        // + 32768 - 91881 * 128) >> 16, an arithmetic shift), clamped to
        // [0, 2^24) so that byte 2 is the channel; G's two chroma products by
        // one v_dot2_u32_u16
        const int x0 = lane * 8;
        const CC6 A = cc_pairs(jp.c[0][1], jp.c[1][1], csel, cx_lo);
        const u16x2 three = {3, 3}, c8 = {8, 8}, c7 = {7, 7};
        const u16x2 wg = {22554, 46802};
        // G = Y16 + kKg - dot2(P, wg) = Y16 - dot2(P, wg, -kKg) mod 2^32: the
        // constant rides in the dot product's accumulator operand
        constexpr uint32_t kKg = 32768u + (22554u + 46802u) * 128u;
        constexpr int32_t kKr = 32768 - 91881 * 128, kKb = 32768 - 116130 * 128;
        {
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            if (!(r ? need1 : need0)) continue;
            const CC6 F = cc_pairs(jp.c[0][r ? 2 : 0], jp.c[1][r ? 2 : 0], csel, cx_lo);
            u16x2 T[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) T[i] = A.q[i] * three + F.q[i];
            uint32_t px[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const int k = j >> 1;
              const u16x2 P = (j & 1) ? (T[k + 1] * three + T[k + 2] + c7) >> 4 : (T[k + 1] * three + T[k] + c8) >> 4;
              const uint32_t pw = __builtin_bit_cast(uint32_t, P);
              const uint32_t yw = r ? (j < 4 ? jp.y1.x : jp.y1.y) : (j < 4 ? jp.y0.x : jp.y0.y);
              const uint32_t yk = __builtin_amdgcn_perm(0u, yw, 0x0C000C0Cu | ((uint32_t)(j & 3) << 16));
              const int rr = (int)(yk + __umul24(pw >> 16, 91881u) + (uint32_t)kKr);
              const int gg = (int)(yk - __builtin_amdgcn_udot2(P, wg, 0u - kKg, false));
              const int bb = (int)(yk + mul24_lo16(pw, 116130u) + (uint32_t)kKb);
              const uint32_t xr = (uint32_t)min(max(rr, 0), 0xFFFFFF), xg = (uint32_t)min(max(gg, 0), 0xFFFFFF),
                             xb = (uint32_t)min(max(bb, 0), 0xFFFFFF);
              px[j] = __builtin_amdgcn_perm(xb, __builtin_amdgcn_perm(xg, xr, 0x0C0C0602u), 0x0C060100u);
            }
            if (x0 < W) {
              uint4 *dq = reinterpret_cast<uint4 *>((r ? s1 : s0) + x0);
              dq[0] = make_uint4(px[0], px[1], px[2], px[3]);
              dq[1] = make_uint4(px[4], px[5], px[6], px[7]);
            }
          }
        }
      } else if constexpr (fast420) {
        const int x0 = lane * 8;
        int cb[2][8], crr[2][8];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          int A[6], U[6], D[6];
          bytes6(jp.c[c][1], lane, rc, A);
          bytes6(jp.c[c][0], lane, rc, U);
          bytes6(jp.c[c][2], lane, rc, D);
          int T[6], B[6];
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            T[i] = A[i] * 3 + U[i];
            B[i] = A[i] * 3 + D[i];
          }
          int *o0 = c == 0 ? cb[0] : crr[0];
          int *o1 = c == 0 ? cb[1] : crr[1];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int ci = (j >> 1) + 1;
            const int nt = (j & 1) ? T[ci + 1] : T[ci - 1];
            const int nbv = (j & 1) ? B[ci + 1] : B[ci - 1];
            o0[j] = (T[ci] * 3 + nt + 8 - (j & 1)) >> 4;
            o1[j] = (B[ci] * 3 + nbv + 8 - (j & 1)) >> 4;
          }
        }
        uint32_t p0[8], p1[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint32_t ya_ = j < 4 ? jp.y0.x : jp.y0.y, yb_ = j < 4 ? jp.y1.x : jp.y1.y;
          const int sh = 8 * (j & 3);
          p0[j] = ycc_px((int)((ya_ >> sh) & 255), cb[0][j], crr[0][j]);
          p1[j] = ycc_px((int)((yb_ >> sh) & 255), cb[1][j], crr[1][j]);
        }
        if (x0 < W) {
          uint4 *d0 = reinterpret_cast<uint4 *>(s0 + skw<kSkew>(x0));
          uint4 *d1 = reinterpret_cast<uint4 *>(s1 + skw<kSkew>(x0));
          d0[0] = make_uint4(p0[0], p0[1], p0[2], p0[3]);
          d0[1] = make_uint4(p0[4], p0[5], p0[6], p0[7]);
          d1[0] = make_uint4(p1[0], p1[1], p1[2], p1[3]);
          d1[1] = make_uint4(p1[4], p1[5], p1[6], p1[7]);
        }
      } else {
        // generic: any supported sampling, gray, RGB, wide images
        const uint8_t *pl0 = planes + d.plane_off[0];
        for (int r = 0; r < 2; ++r) {
          const int yy = y + r;
          if (!(r ? need1 : need0)) continue;
          uint32_t *sr = r ? s1 : s0;
          for (int x0 = lane * 8; x0 < W; x0 += 512) {
            uint32_t px[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const int x = min(x0 + j, W - 1);
              const int Y = pl0[(int64_t)yy * d.plane_stride[0] + x];
              if (d.color == 2) {
                px[j] = rgbx(Y, Y, Y);
              } else {
                const int cb = chroma_at(d, planes + d.plane_off[1], 1, x, yy);
                const int cr = chroma_at(d, planes + d.plane_off[2], 2, x, yy);
                px[j] = d.color == 1 ? rgbx(Y, cb, cr) : ycc_px(Y, cb, cr);
              }
            }
            uint4 *dd = reinterpret_cast<uint4 *>(sr + skw<kSkew>(x0));
            dd[0] = make_uint4(px[0], px[1], px[2], px[3]);
            dd[1] = make_uint4(px[4], px[5], px[6], px[7]);
          }
        }
      }
    } else {
      if constexpr (raw_al16) {
        if (lane * 16 < W) {
          stage16_raw<kSkew>(pf.r0, s0, lane * 16);
          if (need1) stage16_raw<kSkew>(pf.r1, s1, lane * 16);
        }
      } else {
        for (int r = 0; r < 2; ++r) {
          const int yy = y + r;
          if (!(r ? need1 : need0)) continue;
          const uint8_t *row = raw_cell + (int64_t)yy * W * 3;
          for (int x0 = lane * 16; x0 < W; x0 += 1024) stage16_raw<kSkew>(load16_any(row, W, x0), r ? s1 : s0, x0);
        }
      }
    }
  };

  // Output addressing: everything but the lane's column (and, for the raw
  // sources' items, channel) is wave-uniform. The band's first row is
  // computed once per task and stepped per finished row (and per channel) in
  // scalar registers; a lane adds its 32-bit byte offset (3 oh ow elements of
  // at most 4 bytes stay far below 2^32 for every size the kernel serves).
  const int chs = OH * OW; // elements of a channel plane
  uint8_t *orow = outb + (nhwc ? ((int64_t)img * OH + oy0) * OW * 3 : ((int64_t)img * 3 * OH + oy0) * OW) * es;
  const int ostep = (nhwc ? 3 * OW : OW) * es;
  uint32_t voff[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    voff[i] = (uint32_t)(nhwc ? (kRgbx ? 12 * lane : vo[i] * 3 + vc[i]) : (kRgbx ? 4 * lane : vc[i] * chs + vo[i])) * (uint32_t)es;
  int next_oy = 0;     // next output row of the band to finish
  int kv_base = -1;    // first band row held in kv (computed coefficients)
  int slot = 0;        // ring slot of row y
  // No fixed-point sum of this kernel needs Pillow's clip8. It only runs
  // BILINEAR: every weight is >= 0 and a row's weights are (int)(0.5 + w 2^22)
  // of at most kResampTaps normalised w, so they sum to at most
  // 2^22 + (kResampTaps + 1) / 2, and with inputs <= 255 a sum is at most
  // 255 (2^22 + 6) + 2^21 < 256 * 2^22 (it stays below while the weights sum
  // to kMaxRowSum or less; tools/checks/trim_check.cpp sweeps the tables). The
  // result is then bits 22..29 as they stand, for any bytes in the source
  // dwords, a skipped row's stale ones included.
  constexpr int64_t kMaxRowSum = (((int64_t)256 << kPrecisionBits) - (1 << (kPrecisionBits - 1)) - 1) / 255;
  static_assert(kMaxRowSum == 4202528, "the bound trim_check.cpp tests");
  static_assert(((int64_t)1 << kPrecisionBits) + (kResampTaps + 1) / 2 <= kMaxRowSum, "a tap sum may pass 255: clip8 needed");
  // and the computed vertical coefficients of taller images, up to 2 kMaxReduce + 1 taps
  static_assert(((int64_t)1 << kPrecisionBits) + kMaxReduce + 1 <= kMaxRowSum, "a tap sum may pass 255: clip8 needed");
  // horizontal taps of the staged row pair y, y+1: 7 (q, row) jobs of 64
  // output columns. A row that no output row reads (need0, need1 above) has
  // no jobs of its own; the mixed job (q = 3, both rows) still runs and
  // leaves that row's half in a ring slot no window contains.
  auto horizontal = [&](int y, bool need0, bool need1) {
    const int slot1 = slot + 1 == RING ? 0 : slot + 1;
    const int so0 = slot * OWS, so1 = slot1 * OWS; // the rows' ring offsets, scalar
    // one job: column set q of row r (r < 0: the mixed job, row lane / 32)
    auto job = [&](int q, int rj) {
      const int r = rj < 0 ? (lane >> 5) : rj;
      const int ox = GEN || q < 3 ? lane + 64 * q : 192 + (lane & 31);
      const uint32_t *rowp = stg + (r ? g.spad : 0);
      int32_t a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
#pragma unroll
      for (int t = 0; t < KS; ++t) {
        // Pillow weights are >= 0 and <= 2^22: 24-bit products (v_mul_u32_u24
        // with SDWA byte selects), exact in 32 bits. The window crosses at
        // most one 32-pixel skew step (KS < 32), at tap xcr[q].
        const uint32_t v = kSkew ? (rowp + (t < xcr[q] ? xsk[q] : xsk[q] + 4))[t] : rowp[xm[q] + t];
        const uint32_t kw = (uint32_t)wgt[q][t];
        a0 += (int32_t)mul24_byte<0>(v, kw);
        a1 += (int32_t)mul24_byte<1>(v, kw);
        a2 += (int32_t)mul24_byte<2>(v, kw);
      }
      const int so = r ? so1 : so0;
      if constexpr (GEN) {
        // columns [ow, ows) pad the ring row: zeros, so that the last group's
        // vertical taps read defined values; nothing past ows is written
        if (ox >= OW) a0 = a1 = a2 = 0;
        if (ox >= OWS) return;
      }
      const uint32_t b0 = (uint32_t)a0 >> kPrecisionBits, b1 = (uint32_t)a1 >> kPrecisionBits,
                     b2 = (uint32_t)a2 >> kPrecisionBits;
      if constexpr (kRgbx) {
        reinterpret_cast<uint32_t *>(ring)[so + ox] = b0 | (b1 << 8) | (b2 << 16);
      } else {
        uint8_t *rw = ring + so + ox;
        rw[0] = (uint8_t)b0;
        rw[RING * OWS] = (uint8_t)b1;
        rw[2 * RING * OWS] = (uint8_t)b2;
      }
    };
    // a row's jobs in one basic block behind the row's predicate, then the mixed job
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (!(r ? need1 : need0)) continue;
#pragma unroll
      for (int q = 0; q < (GEN ? 4 : 3); ++q)
        if (!GEN || 64 * q < OWS) job(q, r); // a narrower output has no such column set (wave-uniform)
    }
    if constexpr (!GEN) job(3, -1);
    slot = slot1 + 1 == RING ? 0 : slot1 + 1;
  };
  // the table row of output row next_oy (ymin, count, weights), wave-uniform
  constexpr int kTabTaps = 2 * ((kResampMaxSize + kOut - 1) / kOut) + 1; // most taps of a cached height
  static_assert(kTabTaps <= kResampRow - 2, "table row too short");
  static_assert(kTabTaps == kResampTaps, "resamp_cached admits what a table row's unrolled taps cover");
  int32_t vrow[kResampRow] = {};
  auto load_vrow = [&]() {
    if (vtab && next_oy < nb) {
#pragma unroll
      for (int i = 0; i < kResampRow; ++i) vrow[i] = tv[next_oy * kResampRow + i];
    }
  };
  load_vrow();
  // finish every output row whose vertical window lies in ring rows [ya0, done)
  auto vertical = [&](int done) {
    while (next_oy < nb) {
      const int j = next_oy;
      int ymin, cnt, jr = 0;
      if (vtab) {
        ymin = vrow[0];
        cnt = vrow[1];
      } else {
        if (j >= kv_base + kKvRows || kv_base < 0) {
          kv_base = j;
          if (lane < kKvRows && j + lane < nb) {
            int ym;
            const int n = resample_coeffs_one(H, OH, oy0 + j + lane, ks_v, kv + lane * ks_v, &ym);
            vb[2 * lane] = ym;
            vb[2 * lane + 1] = n;
          }
          wave_lds_fence();
        }
        jr = j - kv_base;
        ymin = __builtin_amdgcn_readfirstlane(vb[2 * jr]);
        cnt = __builtin_amdgcn_readfirstlane(vb[2 * jr + 1]);
      }
      if (ymin + cnt > done) break;
      ++next_oy;
      const int s0 = (ymin - ya0) % RING;
      // JPEG (RGBx ring): lane g < 56 owns output columns 4g..4g+3, all three
      // channels, from one 16-byte read of the ring row per tap (lanes 56-63
      // read group 55). Raw (byte planes): 168 items of 4 columns of a channel.
      // GEN: NG groups, 3 x NG items.
      const int gq = min(lane, NG - 1);
      int32_t acc[3][4];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][e] = 1 << (kPrecisionBits - 1);
      // kw: the tap's weight, wave-uniform (a table row's from scalar registers,
      // or a computed one from an LDS broadcast)
      auto tap = [&](int t, uint32_t kw) {
        const int sl = s0 + t < RING ? s0 + t : s0 + t - RING;
        if constexpr (kRgbx) {
          // 16-byte aligned: wave_bytes and 8 spad are multiples of 16, ows of 4
          const uint4 v4 = *static_cast<const uint4 *>(__builtin_assume_aligned(ring + (sl * OWS + 4 * gq) * 4, 16));
          const uint32_t w4[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc[0][e] += (int32_t)mul24_byte<0>(w4[e], kw);
            acc[1][e] += (int32_t)mul24_byte<1>(w4[e], kw);
            acc[2][e] += (int32_t)mul24_byte<2>(w4[e], kw);
          }
        } else {
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            const uint32_t v = *reinterpret_cast<const uint32_t *>(ring + (vc[i] * RING + sl) * OWS + vo[i]);
            acc[i][0] += (int32_t)mul24_byte<0>(v, kw);
            acc[i][1] += (int32_t)mul24_byte<1>(v, kw);
            acc[i][2] += (int32_t)mul24_byte<2>(v, kw);
            acc[i][3] += (int32_t)mul24_byte<3>(v, kw);
          }
        }
      };
      if (vtab) {
        // Unrolled, so that every weight is a fixed scalar register (a loop to
        // cnt indexes them through VGPR copies), and in straight-line groups
        // of three, then two taps behind one scalar test each: a group's
        // products are then v_mul_u32_u24 with SDWA byte selects summed by
        // v_add3_u32, as in the horizontal pass (a tap in a basic block of its
        // own is 12 v_mad_u32_u24 fed by 16 separate byte extractions). A
        // group may run up to two taps past cnt: their weights are the table
        // row's zeros, and their slots are ring rows of this wave: a group
        // runs t <= max(2, cnt) <= ks_v + 1 = RING (cnt <= ks_v, ks_v >= 1),
        // and s0 <= RING - 1, so s0 + t < 2 RING and the wrap below holds.
        auto taps = [&](auto first, auto n) {
#pragma unroll
          for (int t = decltype(first)::value; t < decltype(first)::value + decltype(n)::value; ++t)
            tap(t, (uint32_t)vrow[2 + t]);
        };
        using std::integral_constant;
        static_assert(kTabTaps == 11, "the groups below cover 3 + 2 + 2 + 2 + 2 taps");
        taps(integral_constant<int, 0>{}, integral_constant<int, 3>{});
        if (cnt > 3) {
          taps(integral_constant<int, 3>{}, integral_constant<int, 2>{});
          if (cnt > 5) {
            taps(integral_constant<int, 5>{}, integral_constant<int, 2>{});
            if (cnt > 7) {
              taps(integral_constant<int, 7>{}, integral_constant<int, 2>{});
              if (cnt > 9) taps(integral_constant<int, 9>{}, integral_constant<int, 2>{});
            }
          }
        }
        load_vrow(); // the next row's, behind this row's LUT reads and stores
      } else {
        for (int t = 0; t < cnt; ++t) tap(t, (uint32_t)kv[jr * ks_v + t]);
      }
      // the row's wave-uniform address (scalar registers), stepped per row
      uint8_t *const prow = orow;
      orow += ostep;
      if constexpr (FMT) {
        uint32_t v[3][4];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            v[i][e] = (s_bits + (kRgbx ? i : vc[i]) * 256)[lut_index(acc[i][e])];
        if (nhwc) {
          if constexpr (kRgbx) {
            // 12 consecutive elements: columns 4 lane .. 4 lane + 3, all three
            // channels; the last group is cut per pixel
            const int col = 4 * lane;
            if (lane < NG) {
              uint8_t *p = prow + voff[0];
              if (col + 3 < OW && ((uintptr_t)p & (uintptr_t)(4 * es - 1)) == 0) {
                fmt_store4(p, es, v[0][0], v[1][0], v[2][0], v[0][1]);
                fmt_store4(p + 4 * es, es, v[1][1], v[2][1], v[0][2], v[1][2]);
                fmt_store4(p + 8 * es, es, v[2][2], v[0][3], v[1][3], v[2][3]);
              } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                  if (col + e < OW) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) fmt_store1(p + (3 * e + c) * es, es, v[c][e]);
                  }
              }
            }
          } else {
            // a channel's four columns: elements three apart
#pragma unroll
            for (int i = 0; i < 3; ++i)
              if (lane + 64 * i < 3 * NG) {
                uint8_t *p = prow + voff[i];
#pragma unroll
                for (int e = 0; e < 4; ++e)
                  if (vo[i] + e < OW) fmt_store1(p + 3 * e * es, es, v[i][e]);
              }
          }
        } else {
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            const int col = kRgbx ? 4 * lane : vo[i];
            if (kRgbx ? lane < NG : lane + 64 * i < 3 * NG) {
              uint8_t *p = uniform_ptr(prow + (kRgbx ? (int64_t)i * chs * es : 0)) + voff[i];
              if (col + 3 < OW && ((uintptr_t)p & (uintptr_t)(4 * es - 1)) == 0) {
                fmt_store4(p, es, v[i][0], v[i][1], v[i][2], v[i][3]);
              } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                  if (col + e < OW) fmt_store1(p + e * es, es, v[i][e]);
              }
            }
          }
        }
        continue;
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int ch = kRgbx ? i : vc[i], col = kRgbx ? 4 * lane : vo[i];
        if (kRgbx ? lane < NG : lane + 64 * i < 3 * NG) {
          const float *lc = s_lut + ch * 256;
          float4 f;
          f.x = lc[lut_index(acc[i][0])];
          f.y = lc[lut_index(acc[i][1])];
          f.z = lc[lut_index(acc[i][2])];
          f.w = lc[lut_index(acc[i][3])];
          float *op = reinterpret_cast<float *>(uniform_ptr(prow + (kRgbx ? (int64_t)i * chs * 4 : 0)) + voff[i]);
          if (!GEN || g.vec4) {
            *reinterpret_cast<float4 *>(op) = f;
          } else {
            // rows off 16-byte alignment, and the last group's columns past ow
            op[0] = f.x;
            if (col + 1 < OW) op[1] = f.y;
            if (col + 2 < OW) op[2] = f.z;
            if (col + 3 < OW) op[3] = f.w;
          }
        }
      }
    }
  };

  // One row pair in flight while the previous one is computed (a second
  // register set measured no faster and costs a wave per SIMD). The output
  // rows completed by the previous pair are finished BEFORE this pair's
  // horizontal taps: their float4 stores then drain behind the taps instead
  // of being waited for (vmcnt counts loads and stores together) by the next
  // staging's wait for its prefetched rows. The ring size is unchanged: the
  // rows still pending need at most ks_v - 1 earlier rows plus this pair.
  constexpr int kStep = 2;
#ifdef LDT_RESIZE4_NO_ROW_SKIP
  constexpr bool kRowSkip = false; // A/B build: every row of every pair staged and filtered
#else
  constexpr bool kRowSkip = true;
#endif
  fetch(pa, ya0, !kRowSkip || ya0 >= ya, kRowSkip ? ya0 + 1 < yb : ya0 + 1 < H);
  for (int y = ya0; y < yb; y += kStep) {
    const bool need0 = !kRowSkip || y >= ya, need1 = kRowSkip ? y + 1 < yb : y + 1 < H;
    stage(pa, y, need0, need1);
    // the next pair's first row is past ya
    if (y + kStep < yb) fetch(pa, y + kStep, true, kRowSkip ? y + kStep + 1 < yb : y + kStep + 1 < H);
    wave_lds_fence();
    vertical(y);
    horizontal(y, !kRowSkip || need0, !kRowSkip || need1);
    wave_lds_fence();
  }
  vertical(yb + 1);
}

template <int SRC, int KS, bool GEN = false, bool FMT = false>
__global__ void __launch_bounds__(256) k_resize4(const ImgDesc *__restrict__ descs,
                                                 const uint8_t *__restrict__ planes, RawSrc raw,
                                                 const float *__restrict__ lut,
                                                 const int32_t *__restrict__ resamp,
                                                 const int64_t *__restrict__ labels,
                                                 float *__restrict__ out,
                                                 int64_t *__restrict__ out_labels,
                                                 const int32_t *__restrict__ status, Geom4 g) {
  resize4_body<SRC, KS, GEN, FMT>(descs, planes, raw, lut, resamp, labels, out, out_labels, status, g);
}

// ---------------------------------------------------------------------------
// Launch geometry: Geom4 and make_geom4 live in ldt_geom4.hpp (no HIP there).
// ---------------------------------------------------------------------------
// The FMT instantiations (one per kernel form) are compiled in a translation
// unit of their own, ldt_resize4_fmt.hip, which includes this file with
// LDT_RESIZE4_FMT_TU defined: the two then build side by side, and this one
// holds exactly the kernels it held before the output format existed.
#ifdef LDT_RESIZE4_FMT_TU
constexpr bool kFmtTu = true;
#else
constexpr bool kFmtTu = false;
#endif
template <int SRC, int KS, bool GEN>
static hipError_t launch4(const ImgDesc *descs, const uint8_t *planes, RawSrc raw, const float *lut,
                          const int32_t *resamp, const int64_t *labels, float *out, int64_t *out_labels,
                          const int32_t *status, const Geom4 &g, hipStream_t s, int *occ) {
  static hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_resize4<SRC, KS, GEN, kFmtTu>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (attr != hipSuccess) return attr;
  const int lds = kResize4Lut + g.wpg * g.wave_bytes;
  if (occ) {
    // not a launch: the workgroups of this shape a CU holds (registers and the
    // launch's dynamic LDS), asked of the runtime once per instantiation and
    // shape: the last answer is kept as lds | wpg << 20 | blocks << 24
    static std::atomic<uint64_t> last{0};
    const uint64_t key = (uint64_t)lds | ((uint64_t)g.wpg << 20);
    const uint64_t v = last.load(std::memory_order_relaxed);
    if (v != 0 && (v & 0xFFFFFF) == key) {
      *occ = (int)(v >> 24);
      return hipSuccess;
    }
    int blocks = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &blocks, reinterpret_cast<const void *>(&k_resize4<SRC, KS, GEN, kFmtTu>), 64 * g.wpg, (size_t)lds);
    if (e != hipSuccess) {
      // no answer: the caller counts by the LDS alone
      (void)hipGetLastError();
      *occ = 0;
      return hipSuccess;
    }
    last.store(key | ((uint64_t)blocks << 24), std::memory_order_relaxed);
    *occ = blocks;
    return hipSuccess;
  }
  const int groups = (g.ntask + g.wpg - 1) / g.wpg;
  hipLaunchKernelGGL((k_resize4<SRC, KS, GEN, kFmtTu>), dim3(groups), dim3(64 * g.wpg), lds, s, descs,
                     planes, raw, lut, resamp, labels, out, out_labels, status, g);
  return hipGetLastError();
}

template <int SRC, bool GEN>
static bool dispatch4k(int ks_h, const ImgDesc *descs, const uint8_t *planes, RawSrc raw,
                      const float *lut, const int32_t *resamp, const int64_t *labels, float *out,
                      int64_t *out_labels, const int32_t *status, const Geom4 &g, hipStream_t s,
                      hipError_t *err, int *occ) {
  switch (ks_h) {
  case 3: *err = launch4<SRC, 3, GEN>(descs, planes, raw, lut, resamp, labels, out, out_labels, status, g, s, occ); return true;
  case 4: *err = launch4<SRC, 4, GEN>(descs, planes, raw, lut, resamp, labels, out, out_labels, status, g, s, occ); return true;
  case 5: *err = launch4<SRC, 5, GEN>(descs, planes, raw, lut, resamp, labels, out, out_labels, status, g, s, occ); return true;
  case 6: *err = launch4<SRC, 6, GEN>(descs, planes, raw, lut, resamp, labels, out, out_labels, status, g, s, occ); return true;
  case 7: *err = launch4<SRC, 7, GEN>(descs, planes, raw, lut, resamp, labels, out, out_labels, status, g, s, occ); return true;
  case 8: *err = launch4<SRC, 8, GEN>(descs, planes, raw, lut, resamp, labels, out, out_labels, status, g, s, occ); return true;
  case 9: *err = launch4<SRC, 9, GEN>(descs, planes, raw, lut, resamp, labels, out, out_labels, status, g, s, occ); return true;
  case 10: *err = launch4<SRC, 10, GEN>(descs, planes, raw, lut, resamp, labels, out, out_labels, status, g, s, occ); return true;
  case 11: *err = launch4<SRC, 11, GEN>(descs, planes, raw, lut, resamp, labels, out, out_labels, status, g, s, occ); return true;
  default: return false;
  }
}

// The kOut x kOut instantiations, or the generic-width kernel for any other
// size (and for kOut x kOut on request: ResizeOut::generic).
template <int SRC>
static bool dispatch4(int ks_h, const ImgDesc *descs, const uint8_t *planes, RawSrc raw,
                      const float *lut, const int32_t *resamp, const int64_t *labels, float *out,
                      int64_t *out_labels, const int32_t *status, const Geom4 &g, hipStream_t s,
                      hipError_t *err, bool gen, int *occ) {
  return gen ? dispatch4k<SRC, true>(ks_h, descs, planes, raw, lut, resamp, labels, out, out_labels, status, g, s, err, occ)
             : dispatch4k<SRC, false>(ks_h, descs, planes, raw, lut, resamp, labels, out, out_labels, status, g, s, err, occ);
}

#ifdef LDT_RESIZE4_FMT_TU
bool dispatch4_fmt(int src, int ks_h, const ImgDesc *descs, const uint8_t *planes, RawSrc raw, const float *lut,
                   const int32_t *resamp, const int64_t *labels, float *out, int64_t *out_labels,
                   const int32_t *status, const Geom4 &g, hipStream_t s, hipError_t *err, bool gen, int *occ) {
  switch (src) {
  case 0: return dispatch4<0>(ks_h, descs, planes, raw, lut, resamp, labels, out, out_labels, status, g, s, err, gen, occ);
  case 1: return dispatch4<1>(ks_h, descs, planes, raw, lut, resamp, labels, out, out_labels, status, g, s, err, gen, occ);
  case 2: return dispatch4<2>(ks_h, descs, planes, raw, lut, resamp, labels, out, out_labels, status, g, s, err, gen, occ);
  case 3: return dispatch4<3>(ks_h, descs, planes, raw, lut, resamp, labels, out, out_labels, status, g, s, err, gen, occ);
  case 5: return dispatch4<5>(ks_h, descs, planes, raw, lut, resamp, labels, out, out_labels, status, g, s, err, gen, occ);
  default: return false;
  }
}
#else
// ldt_resize4_fmt.hip: dispatch4<src> over the FMT instantiations
bool dispatch4_fmt(int src, int ks_h, const ImgDesc *descs, const uint8_t *planes, RawSrc raw, const float *lut,
                   const int32_t *resamp, const int64_t *labels, float *out, int64_t *out_labels,
                   const int32_t *status, const Geom4 &g, hipStream_t s, hipError_t *err, bool gen, int *occ);
// A call's kernels: the float32 CHW ones above, or the formatted ones.
template <int SRC>
static bool run4(const OutFmt &fmt, int ks_h, const ImgDesc *descs, const uint8_t *planes, RawSrc raw,
                 const float *lut, const int32_t *resamp, const int64_t *labels, float *out, int64_t *out_labels,
                 const int32_t *status, const Geom4 &g, hipStream_t s, hipError_t *err, bool gen, int *occ) {
  return fmt_default(fmt)
             ? dispatch4<SRC>(ks_h, descs, planes, raw, lut, resamp, labels, out, out_labels, status, g, s, err, gen, occ)
             : dispatch4_fmt(SRC, ks_h, descs, planes, raw, lut, resamp, labels, out, out_labels, status, g, s, err,
                             gen, occ);
}

// Whether a launch for `ro` takes the generic-width kernel, and whether the
// band kernel serves it at all: widths up to kTileCols, every source width of
// the batch with a horizontal table entry.
static bool use_generic4(const ResizeOut &ro) { return ro.generic || ro.oh != kOut || ro.ow != kOut; }
static bool band_kernel_ok(const ResizeOut &ro, int max_w) {
  return ro.ow <= kTileCols && ro.tab_h != nullptr && ro.tab_v != nullptr && resamp_cached(max_w, ro.ow, ro.max_in_h);
}
static void finish_geom4(Geom4 &g, const ResizeOut &ro, const float *out) {
  g.tab_v = ro.tab_v;
  g.vec4 = (ro.ow & 3) == 0 && (((uintptr_t)out) & 15) == 0 ? 1 : 0;
  // the formatted kernels' launch: the format in vec4's place (Geom4), so the
  // kernel argument block is the one the float32 CHW kernels always had
  if (!fmt_default(ro.fmt)) g.vec4 = ro.fmt.dtype | (ro.fmt.layout << 8);
}

// Waves to aim for: the CU count times the resident waves per CU, which is
// what the LDS holds and what the runtime reports for the instantiation
// (`blocks` workgroups per CU: registers and LDS; 0: not asked), at most
// kResizeMaxWaves.
constexpr int kResizeMaxWaves = 16;
static int waves_target4(const Geom4 &g, int pct, int blocks) {
  const int max_wg = kResizeMaxWaves / g.wpg;
  static int cus = 0;
  if (cus == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) cus = 256;
    else cus = prop.multiProcessorCount;
  }
  int wg = kResize4LdsMax / (kResize4Lut + g.wpg * g.wave_bytes);
  if (blocks > 0 && wg > blocks) wg = blocks;
  if (wg > max_wg) wg = max_wg;
  if (wg < 1) wg = 1;
  // LDT_OPT_RESIZE_WAVES_PCT: more, shorter bands fill the
  // pipeline's CU gaps better but cost the kernel's own efficiency
  return cus * g.wpg * wg * (pct > 0 ? pct : 100) / 100;
}

// The kernel's horizontal taps for a batch whose widths have at most `taps`
// (ResizeOut::taps_h; 0: not known, Pillow's capacity for the widest).
static int horizontal_taps4(const ResizeOut &ro, int max_w) {
  return resize4_taps(ro.taps_h > 0 ? ro.taps_h : resample_ksize_host(max_w, ro.ow));
}
static int vertical_taps4(const ResizeOut &ro, int max_h) {
  return ro.taps_v > 0 ? ro.taps_v : resample_ksize_host(max_h, ro.oh);
}

bool launch_resize4_jpeg(const DevPlan &p, const DevWork &w, float *out, int64_t *out_labels,
                         hipStream_t s, hipError_t *err, int *wpg_used, int *bands_used) {
  Geom4 g;
  const ResizeOut &ro = p.ro;
  if (resample_ksize_host(p.max_w, ro.ow) > kResampTaps || !band_kernel_ok(ro, p.max_w)) return false;
  const int ks_h = horizontal_taps4(ro, p.max_w), ks_v = vertical_taps4(ro, p.max_h);
  const bool gen = use_generic4(ro);
  // a tall image (large ring) may not fit 4 waves' LDS in one workgroup:
  // fewer waves per workgroup before giving the batch to the streaming kernel
  int wpg = p.resize_wpg > 0 ? p.resize_wpg : kResizeWavesJpeg;
  while (!make_geom4(p.n, p.max_w, p.max_h, ks_h, ks_v, 1, g, wpg, true, ro.oh, ro.ow, ro.max_in_v)) {
    if (wpg == 1) return false;
    wpg >>= 1;
  }
  RawSrc raw{nullptr, 0, 0, 0};
  // 4:2:0 images of width <= 512: the packed 16-bit staging (k_resize4<5>),
  // or the 32-bit one (k_resize4<0>, LDT_OPT_RESIZE_IMPL 1, cross-check)
  auto run420 = [&](int *occ) {
    return p.resize420 == 3
               ? run4<5>(ro.fmt, ks_h, p.descs, w.planes, raw, p.lut, ro.tab_h, p.labels, out, out_labels, w.status, g, s, err, gen, occ)
               : run4<0>(ro.fmt, ks_h, p.descs, w.planes, raw, p.lut, ro.tab_h, p.labels, out, out_labels, w.status, g, s, err, gen, occ);
  };
  auto run_rest = [&](int *occ) {
    return run4<2>(ro.fmt, ks_h, p.descs, w.planes, raw, p.lut, ro.tab_h, p.labels, out, out_labels, w.status, g, s,
                   err, gen, occ);
  };
  // the band count follows the batch's first kernel's occupancy
  int blocks = 0;
  if (!(p.n_fast420 > 0 ? run420(&blocks) : run_rest(&blocks))) return false;
  if (*err != hipSuccess) return true;
  if (!make_geom4(p.n, p.max_w, p.max_h, ks_h, ks_v, waves_target4(g, p.resize_waves_pct, blocks), g, wpg, true,
                  ro.oh, ro.ow, ro.max_in_v))
    return false;
  finish_geom4(g, ro, out);
  if (wpg_used) *wpg_used = wpg;
  if (bands_used) *bands_used = g.nbands;
  // fast-path images and the rest go to separate kernels (each skips the
  // other's images); a batch of one kind launches one kernel. The first
  // launch also writes the failed images (k_fill_failed's job otherwise).
  g.fill = 1;
  if (p.n_fast420 > 0) {
    if (!run420(nullptr)) return false;
    if (*err != hipSuccess || p.n_fast420 == p.n) return true;
    g.fill = 0;
  }
  return run_rest(nullptr);
}

bool launch_resize4_raw(const uint8_t *hwc, int64_t cell_stride, int n, int h, int wd,
                        const float *lut, const ResizeOut &ro, float *out, hipStream_t s,
                        hipError_t *err) {
  Geom4 g;
  if (resample_ksize_host(wd, ro.ow) > kResampTaps || !band_kernel_ok(ro, wd)) return false;
  const int ks_h = horizontal_taps4(ro, wd), ks_v = vertical_taps4(ro, h);
  const bool gen = use_generic4(ro);
  const int32_t *resamp = ro.tab_h;
  if (!make_geom4(n, wd, h, ks_h, ks_v, 1, g, kResizeWaves, false, ro.oh, ro.ow, ro.max_in_v)) return false;
  RawSrc raw{hwc, cell_stride, h, wd};
  const bool al16 = (((uintptr_t)hwc) & 15) == 0 && (cell_stride & 15) == 0 && ((wd * 3) & 15) == 0 &&
                    wd <= 1024;
  auto run = [&](int *occ) {
    if (!al16)
      return run4<3>(ro.fmt, ks_h, (const ImgDesc *)nullptr, (const uint8_t *)nullptr, raw, lut, resamp,
                     (const int64_t *)nullptr, out, (int64_t *)nullptr, (const int32_t *)nullptr, g, s, err, gen, occ);
    return run4<1>(ro.fmt, ks_h, (const ImgDesc *)nullptr, (const uint8_t *)nullptr, raw, lut, resamp,
                   (const int64_t *)nullptr, out, (int64_t *)nullptr, (const int32_t *)nullptr, g, s, err, gen, occ);
  };
  int blocks = 0;
  if (!run(&blocks)) return false;
  if (*err != hipSuccess) return true;
  if (!make_geom4(n, wd, h, ks_h, ks_v, waves_target4(g, 100, blocks), g, kResizeWaves, false, ro.oh, ro.ow,
                  ro.max_in_v))
    return false;
  finish_geom4(g, ro, out);
  g.fill = 0;
  return run(nullptr);
}

#endif // LDT_RESIZE4_FMT_TU

} // namespace ldt
