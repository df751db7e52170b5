// The two 16-bit element types of the half-precision MFMA tiles (topk_half_tile.h, softmax_attn_half_tile.h): fp16 and
// bf16 as raw 16-bit patterns, eight of them packed into one 16-byte operand of v_mfma_f32_32x32x16_f16 / _bf16.  Lane
// (l32, kk) feeds A[l32][8 kk .. 8 kk + 8) and B[8 kk .. 8 kk + 8)[l32] of a step's sixteen k, and holds the accumulator as
// mfma_tile.h describes.  A product of two T values is exact in f32; the sum is f32.
#pragma once

#include "mfma_tile.h"

typedef uint32_t v2u __attribute__((ext_vector_type(2)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef __bf16 v8b __attribute__((ext_vector_type(8)));

// the bits of T(f), round to nearest even (NaN is out of scope), the value of such bits, and the MFMA over 16 k
struct TableF16 {
  static __device__ __forceinline__ uint32_t round(float f) {
    return __builtin_bit_cast(uint16_t, static_cast<_Float16>(f));
  }
  static __device__ __forceinline__ float value(uint16_t u) { return static_cast<float>(__builtin_bit_cast(_Float16, u)); }
  static __device__ __forceinline__ v16f mfma(v4u a, v4u b, v16f c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8h, a), __builtin_bit_cast(v8h, b), c, 0, 0, 0);
  }
};
struct TableBf16 {
  static __device__ __forceinline__ uint32_t round(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
  }
  static __device__ __forceinline__ float value(uint16_t u) { return __uint_as_float((uint32_t)u << 16); }
  static __device__ __forceinline__ v16f mfma(v4u a, v4u b, v16f c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8b, a), __builtin_bit_cast(v8b, b), c, 0, 0, 0);
  }
};
