// split3.h -- the fp32-accurate three-way bf16 split that feeds the bf16 matrix cores
// (sa_mfma_common.h's header gives the derivation and the error bound).
//
// Every fp32 operand is the exact sum of three bf16 pieces, x = x0 + x1 + x2: x0 = bf16(x),
// x1 = bf16(x - x0), x2 = bf16(x - x0 - x1), each conversion round-to-nearest-even and each
// residual exact in fp32.  a.b is then taken from the six significant piece products
//   a0 b0 + (a0 b1 + a1 b0) + (a0 b2 + a1 b1 + a2 b0),
// issued smallest first.
//
// The split is written on register pairs, the unit the hardware converts: one v_cvt_pk_bf16_f32
// gives both values' piece as a packed word, each half is widened back to fp32 by one shift (low
// half) or one mask (high half), and the two residuals are plain scalar subtractions:
//   3 conversions + 4 widenings + 4 subtractions = 11 VALU instructions per pair.
// The packed words are the MFMA operand registers as they stand (element 2 j of a bf16x8 is the
// low half of word j), so no instruction assembles the operand.  The subtractions must stay
// scalar: beside MFMAs a packed fp32 op costs more issue cycles than the two scalar ops it
// replaces, so the units that split inside their MFMA loops are built with -fno-slp-vectorize
// (see the Makefile).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dvcp {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// (bf16(lo), bf16(hi)) as one word, round-to-nearest-even: one v_cvt_pk_bf16_f32
__device__ __forceinline__ uint32_t cvt_pk_bf16(float lo, float hi) {
  const f32x2 v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}
// the halves of such a word as fp32 (exact)
__device__ __forceinline__ float bf16_lo_f32(uint32_t w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float bf16_hi_f32(uint32_t w) { return __builtin_bit_cast(float, w & 0xFFFF0000u); }

// the three pieces of a register pair (a, b), as packed words (a's piece in the low half)
__device__ __forceinline__ void split3_pair(float a, float b, uint32_t& p0, uint32_t& p1, uint32_t& p2) {
  p0 = cvt_pk_bf16(a, b);
  const float ra = a - bf16_lo_f32(p0);
  const float rb = b - bf16_hi_f32(p0);
  p1 = cvt_pk_bf16(ra, rb);
  const float sa = ra - bf16_lo_f32(p1);
  const float sb = rb - bf16_hi_f32(p1);
  p2 = cvt_pk_bf16(sa, sb);
}

// x = p0 + p1 + p2 exactly, eight values: one MFMA operand (a 16-deep k-step's half) per piece
struct Split3 {
  bf16x8 p0, p1, p2;
};
__device__ __forceinline__ Split3 split3(const float (&x)[8]) {
  u32x4 w0, w1, w2;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint32_t a, b, c;
    split3_pair(x[2 * j], x[2 * j + 1], a, b, c);
    w0[j] = a;
    w1[j] = b;
    w2[j] = c;
  }
  return Split3{__builtin_bit_cast(bf16x8, w0), __builtin_bit_cast(bf16x8, w1), __builtin_bit_cast(bf16x8, w2)};
}
// The same split of eight values in 12 stages -- pair j = i / 3, piece i % 3 -- of 5, 5 and 1
// instructions, for a caller that places them one by one between MFMAs (sa_mfma_common.h's
// sa_layer2).  Stage i takes the pair (x[2 j], x[2 j + 1]) again; stages of a pair run in order.
struct Split3Stages {
  static constexpr int kStages = 12;
  u32x4 w0, w1, w2;
  float ra[4], rb[4];  // the pairs' residuals so far
  __device__ __forceinline__ void stage(int i, float a, float b) {
    const int j = i / 3;
    if (i % 3 == 0) {
      w0[j] = cvt_pk_bf16(a, b);
      ra[j] = a - bf16_lo_f32(w0[j]);
      rb[j] = b - bf16_hi_f32(w0[j]);
    } else if (i % 3 == 1) {
      w1[j] = cvt_pk_bf16(ra[j], rb[j]);
      ra[j] = ra[j] - bf16_lo_f32(w1[j]);
      rb[j] = rb[j] - bf16_hi_f32(w1[j]);
    } else {
      w2[j] = cvt_pk_bf16(ra[j], rb[j]);
    }
  }
  __device__ __forceinline__ Split3 pieces() const {
    return Split3{__builtin_bit_cast(bf16x8, w0), __builtin_bit_cast(bf16x8, w1), __builtin_bit_cast(bf16x8, w2)};
  }
};
// one value (staging code that scatters single elements)
__device__ __forceinline__ void split3(float x, __bf16& p0, __bf16& p1, __bf16& p2) {
  p0 = static_cast<__bf16>(x);
  const float r1 = x - static_cast<float>(p0);
  p1 = static_cast<__bf16>(r1);
  p2 = static_cast<__bf16>(r1 - static_cast<float>(p1));
}

// acc += a.b over one k-step: the six significant piece products, smallest first
//   m:  0      1      2      3      4      5
//      a2 b0  a1 b1  a0 b2  a1 b0  a0 b1  a0 b0
// on v_mfma_f32_32x32x16_bf16 (16-deep) ...
__device__ __forceinline__ f32x16 mfma_split3_product(int m, const Split3& a, const bf16x8& b0, const bf16x8& b1,
                                                     const bf16x8& b2, f32x16 acc) {
  const bf16x8& x = m == 0 ? a.p2 : (m == 1 || m == 3 ? a.p1 : a.p0);
  const bf16x8& y = m == 2 ? b2 : (m == 1 || m == 4 ? b1 : b0);
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(x, y, acc, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma_split3(const Split3& a, const bf16x8& b0, const bf16x8& b1, const bf16x8& b2,
                                             f32x16 acc) {
#pragma unroll
  for (int m = 0; m < 6; ++m) acc = mfma_split3_product(m, a, b0, b1, b2, acc);
  return acc;
}
// ... and on v_mfma_f32_16x16x32_bf16 (32-deep), the A pieces given one by one
__device__ __forceinline__ f32x4 mfma_split3(const bf16x8& a0, const bf16x8& a1, const bf16x8& a2, const bf16x8& b0,
                                            const bf16x8& b1, const bf16x8& b2, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, b0, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b2, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b0, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b1, acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc, 0, 0, 0);
}

}  // namespace dvcp
