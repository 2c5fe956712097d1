// The split-bf16 scheme, stated once: an f32 x is split round-to-nearest-even on the successive
// residuals into three bf16 terms, x = h + m + l (exact for normal x away from overflow: 3 x 8
// significand bits), so that f32 products run on the bf16 matrix cores at f32 accuracy. The host
// counterpart is ops.split_bf16x3; tests/test_split_host.py holds the two to the same bits.
//
// Every wide conv / GEMM kernel splits with krrn_split3 and only arranges the six packed words
// into its own MFMA operand layout. Self-contained: compiles as device code under hipcc and as
// plain host C++ (clang's __bf16 vectors).
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KRRN_SPLIT_FN __host__ __device__ __forceinline__
#else
#define KRRN_SPLIT_FN static inline
#endif

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x6 __attribute__((ext_vector_type(6)));
typedef unsigned u32x8 __attribute__((ext_vector_type(8)));

// two f32 -> one packed bf16 pair (a in the low half), RNE (v_cvt_pk_bf16_f32 on gfx950)
KRRN_SPLIT_FN unsigned krrn_pk_bf16(float a, float b) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, bf16x2));
}
KRRN_SPLIT_FN float krrn_bf_lo(unsigned p) { return __builtin_bit_cast(float, p << 16); }
KRRN_SPLIT_FN float krrn_bf_hi(unsigned p) { return __builtin_bit_cast(float, p & 0xFFFF0000u); }

// the packed bf16 terms of 4 consecutive values: word 0 of each term holds x[0], x[1], word 1 x[2], x[3]
struct KrrnSplit3 {
  unsigned h0, h1, m0, m1, l0, l1;
};

// (the parameter is krrn_common.h's f32x4, spelled out so that this header stands alone)
KRRN_SPLIT_FN KrrnSplit3 krrn_split3(const float __attribute__((ext_vector_type(4))) x) {
  const unsigned h0 = krrn_pk_bf16(x[0], x[1]), h1 = krrn_pk_bf16(x[2], x[3]);
  const float r0 = x[0] - krrn_bf_lo(h0), r1 = x[1] - krrn_bf_hi(h0);
  const float r2 = x[2] - krrn_bf_lo(h1), r3 = x[3] - krrn_bf_hi(h1);
  const unsigned m0 = krrn_pk_bf16(r0, r1), m1 = krrn_pk_bf16(r2, r3);
  const unsigned l0 = krrn_pk_bf16(r0 - krrn_bf_lo(m0), r1 - krrn_bf_hi(m0));
  const unsigned l1 = krrn_pk_bf16(r2 - krrn_bf_lo(m1), r3 - krrn_bf_hi(m1));
  return KrrnSplit3{h0, h1, m0, m1, l0, l1};
}

// the packed bf16 terms of one pair of values
struct KrrnSplit3Pair {
  unsigned h, m, l;
};

KRRN_SPLIT_FN KrrnSplit3Pair krrn_split3_pair(const f32x2 x) {
  const unsigned h = krrn_pk_bf16(x[0], x[1]);
  const float r0 = x[0] - krrn_bf_lo(h), r1 = x[1] - krrn_bf_hi(h);
  const unsigned m = krrn_pk_bf16(r0, r1);
  return KrrnSplit3Pair{h, m, krrn_pk_bf16(r0 - krrn_bf_lo(m), r1 - krrn_bf_hi(m))};
}

// four packed words as one MFMA operand (8 bf16)
KRRN_SPLIT_FN bf16x8 krrn_op(const u32x4 v) { return __builtin_bit_cast(bf16x8, v); }

// words o .. o + 3 of an operand chain (u32x6 / u32x8) as one MFMA operand
template <typename Chain>
KRRN_SPLIT_FN bf16x8 krrn_sub4(const Chain& c, int o) {
  return __builtin_bit_cast(bf16x8, u32x4{c[o], c[o + 1], c[o + 2], c[o + 3]});
}
