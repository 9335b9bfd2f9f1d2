// ldt_mix.hpp — the mix stage's arithmetic (ldt_set_mix): MixUp / CutMix of a
// row with its partner on the float32 values behind the ToTensor / Normalize
// table, the conversion of the result to the call's 16-bit dtypes and the soft
// label of a class. One source for the kernels (ldt_mix.hip) and for the CPU
// check against torch (tools/checks/mix_host.cpp, tests/test_mix_ops.py), so it
// is plain arithmetic with no HIP call.
//
// What is restated:
//   mix      torchvision v2 MixUp: inpt.roll(1, 0).mul_(1.0 - lam).add_(inpt.mul(lam)),
//            timm's x.mul_(lam).add_(x.flip(0).mul_(1. - lam)): two float32
//            products, each rounded, then one float32 add (never fused). CutMix
//            is the same formula with weights (1, 0) outside the box (exact for
//            finite values) and the partner's value inside it
//   to fp16  torch's .to(torch.float16): round to nearest even, overflow to
//            +-inf from 65520 on, subnormals kept
//   to bf16  torch's .to(torch.bfloat16): round to nearest even on the upper
//            16 bits, NaN -> 0x7FC0
//   labels   one_hot(label).float() through the same roll / mul / add, in
//            closed form per class
// Every floating-point step is an IEEE basic operation, so the device gives
// what the host gives as long as no multiply-add is contracted: the build has
// -ffp-contract=off and this header says so again.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/ldt.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LDT_MIX_HD __host__ __device__ __forceinline__
#else
#define LDT_MIX_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace ldt {

LDT_MIX_HD uint32_t mix_f32_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

// (y, x) inside the box (top, left, height, width); height == 0 = no box.
LDT_MIX_HD bool mix_in_box(int y, int x, int top, int left, int height, int width) {
  return height != 0 && y >= top && y - top < height && x >= left && x - left < width;
}

// One element: x the row's value, p its partner's; boxed: inside the row's box.
LDT_MIX_HD float mix_element(float x, float p, float w_self, float w_partner, bool boxed) {
  if (boxed) return p;
  const float a = p * w_partner;
  const float b = x * w_self;
  return a + b;
}

// float32 bits -> fp16 bits, round to nearest even.
LDT_MIX_HD uint32_t mix_f16_bits(uint32_t x) {
  const uint32_t sign = (x >> 16) & 0x8000u;
  x &= 0x7FFFFFFFu;
  if (x > 0x7F800000u) return sign | 0x7E00u; // NaN
  // 65520 = the tie between the largest finite value 65504 (odd mantissa) and 2^16: inf from there on
  if (x >= 0x477FF000u) return sign | 0x7C00u;
  if (x < 0x38800000u) {
    // below 2^-14: a subnormal result, in units of 2^-24
    const int shift = 126 - (int)(x >> 23);
    if (shift > 24) return sign; // below 2^-25: zero (the tie at 2^-25 goes to the even 0 below)
    const uint32_t mant = (x & 0x7FFFFFu) | 0x800000u;
    uint32_t r = mant >> shift;
    const uint32_t rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (r & 1u))) ++r; // 0x400 is the smallest normal: the carry is right
    return sign | r;
  }
  const uint32_t r = x - 0x38000000u; // exponent rebiased 127 -> 15; a mantissa carry moves into it
  return sign | ((r + 0xFFFu + ((r >> 13) & 1u)) >> 13);
}

// float32 bits -> bf16 bits, round to nearest even.
LDT_MIX_HD uint32_t mix_bf16_bits(uint32_t x) {
  if ((x & 0x7FFFFFFFu) > 0x7F800000u) return 0x7FC0u; // NaN, as c10::BFloat16 gives it
  return (x + 0x7FFFu + ((x >> 16) & 1u)) >> 16;
}

// The element's bits in the call's dtype (LDT_DTYPE_F32 / _F16 / _BF16), in
// the low bits of the result.
LDT_MIX_HD uint32_t mix_store_bits(float v, int dtype) {
  const uint32_t b = mix_f32_bits(v);
  return dtype == LDT_DTYPE_F16 ? mix_f16_bits(b) : dtype == LDT_DTYPE_BF16 ? mix_bf16_bits(b) : b;
}

// The soft label of class c for a row of label a whose partner has label b.
LDT_MIX_HD float mix_soft_label(int64_t c, int64_t a, int64_t b, float lw_self, float lw_partner) {
  if (a == b) return c == a ? lw_partner + lw_self : 0.0f;
  return c == a ? lw_self : c == b ? lw_partner : 0.0f;
}

} // namespace ldt
