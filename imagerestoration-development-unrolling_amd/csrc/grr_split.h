// Split-operand arithmetic of the MFMA kernels: fp32 values as exact sums of bf16 or fp16 terms, and the
// order in which the terms' products are accumulated.  One copy for every GEMM-class kernel (feature_ops,
// lnb_ops, wgrad_ops, feature_edge) and for the pack kernels that lay weights out in fragment order.
//
// The bit-level helpers are __host__ __device__, so a host program can call them (tests/test_split_terms.py).
#pragma once

#include "grr_device.h"

namespace grr {

// ---------------------------------------------------------------------------
// bf16, three terms: v = v0 + v1 + v2 exactly (v0 = rne(v), v1 = rne(v - v0), v2 = v - v0 - v1: the 24
// significand bits as 3 x 8).  Of the nine products of two such splits the six above 2^-24 |a b| are kept.
// ---------------------------------------------------------------------------

// Pack time: integer round-to-nearest-even on the bit pattern (finite values; the same bits as the
// hardware conversion of split3x8)
__host__ __device__ inline uint16_t bf16_bits_rne(float v) {
  uint32_t u;
  __builtin_memcpy(&u, &v, 4);
  return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
__host__ __device__ inline float bf16_bits_val(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float v;
  __builtin_memcpy(&v, &u, 4);
  return v;
}
// bf16 bit pattern of term q (0, 1, 2) of v
__host__ __device__ inline uint16_t split_term(float v, int q) {
  const uint16_t h0 = bf16_bits_rne(v);
  if (q == 0) return h0;
  const float r1 = v - bf16_bits_val(h0);
  const uint16_t h1 = bf16_bits_rne(r1);
  if (q == 1) return h1;
  return bf16_bits_rne(r1 - bf16_bits_val(h1));
}

// six-product accumulation of (a0+a1+a2)(b0+b1+b2), smallest terms first
#define GRR_X3_MFMA(FN, acc, a0, a1, a2, b0, b1, b2) \
  do {                                               \
    acc = FN(a1, b1, acc, 0, 0, 0);                  \
    acc = FN(a2, b0, acc, 0, 0, 0);                  \
    acc = FN(a0, b2, acc, 0, 0, 0);                  \
    acc = FN(a1, b0, acc, 0, 0, 0);                  \
    acc = FN(a0, b1, acc, 0, 0, 0);                  \
    acc = FN(a0, b0, acc, 0, 0, 0);                  \
  } while (0)

// ---------------------------------------------------------------------------
// fp16, two terms: v = hi + lo (hi = rne(v), lo = rne(v - hi)) of operands scaled by a power of two into
// fp16's range.  Three of the four products are kept (lo lo is below fp32 rounding).
// ---------------------------------------------------------------------------

// three-product accumulation of (ah+al)(bh+bl), smallest terms first
#define GRR_X2_MFMA(FN, acc, ah, al, bh, bl) \
  do {                                       \
    acc = FN(al, bh, acc, 0, 0, 0);          \
    acc = FN(ah, bl, acc, 0, 0, 0);          \
    acc = FN(ah, bh, acc, 0, 0, 0);          \
  } while (0)

// In the kernels: the same exact split of 8 values with the hardware RNE conversion (v_cvt_pk_bf16_f32: two
// values per instruction; the residuals come back through a shift / mask): about half the vector
// instructions of split_term, the same bits for finite values
__device__ __forceinline__ void split3x8(const float (&v)[8], bf16x8& t0, bf16x8& t1, bf16x8& t2) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const __bf16 h0 = (__bf16)v[j];
    const float r1 = v[j] - (float)h0;
    const __bf16 h1 = (__bf16)r1;
    const float r2 = r1 - (float)h1;
    t0[j] = h0;
    t1[j] = h1;
    t2[j] = (__bf16)r2;
  }
}

// scale exponent s of a row (or pixel) whose largest |entry| is mx: mx 2^s in [2^13, 2^14), |s| <= clamp
__device__ __forceinline__ int scale_exp(float mx, int clamp) {
  if (mx == 0.f) return 0;
  int e;
  frexpf(mx, &e);
  return clampi(14 - e, -clamp, clamp);
}
// Pack time: term q (0 hi, 1 lo) of a and b as one word (a in the low half)
__device__ __forceinline__ uint32_t f16_pair_word(float a, float b, int q) {
  const _Float16 ha = (_Float16)a, hb = (_Float16)b;
  const _Float16 ta = q == 0 ? ha : (_Float16)(a - (float)ha), tb = q == 0 ? hb : (_Float16)(b - (float)hb);
  return (uint32_t)__builtin_bit_cast(uint16_t, ta) | ((uint32_t)__builtin_bit_cast(uint16_t, tb) << 16);
}
// In the kernels: both terms of (a, b) with packed round-to-nearest conversions (v_cvt_pk_f16_f32): hi, lo
__device__ __forceinline__ void split2_f16(float a, float b, uint32_t& hi, uint32_t& lo) {
  const f32x2 v = f32x2{a, b};
  const f16x2 h = __builtin_convertvector(v, f16x2);
  const f16x2 l = __builtin_convertvector(v - __builtin_convertvector(h, f32x2), f16x2);
  hi = __builtin_bit_cast(uint32_t, h);
  lo = __builtin_bit_cast(uint32_t, l);
}

}  // namespace grr
