// glb_w4.hpp - what the 4-bit translation units share (glb_quant.hip: format kernels and the few-row GEMM; glb_quant_tiled.hip:
// the many-row GEMM): the block constants, the element load / store with its single rounding, and the expansion of eight
// codes into a lane's B operand of v_mfma_f32_16x16x32.  Everything stays in an unnamed namespace: each unit has its copy.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cmath>
#include <cstdint>

#include "../../include/glb.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

constexpr int QB = 64;             // elements of a block
constexpr int UNIT = QB / 2;       // bytes of a block's codes
constexpr int64_t MAX_ELEMS = (int64_t)1 << 34;

struct Codebook {
  float v[16];
};

__device__ __forceinline__ float load_elem(const void *p, int64_t idx, int dt) {
  if (dt == GLB_F32) return ((const float *)p)[idx];
  const uint16_t h = ((const uint16_t *)p)[idx];
  if (dt == GLB_BF16) return __uint_as_float((uint32_t)h << 16);
  return __half2float(__ushort_as_half(h));
}

__device__ __forceinline__ uint16_t bf16_rne(float f) {
  uint32_t u = __float_as_uint(f);
  u += 0x7fffu + ((u >> 16) & 1u);  // (finite input: absmax is finite and every codebook entry is)
  return (uint16_t)(u >> 16);
}

__device__ __forceinline__ void store_elem(void *p, int64_t idx, int dt, float f) {
  // (the barrier keeps the f32 product: multiply + convert must not become one v_fma_mix*_f16, a single rounding)
  asm volatile("" : "+v"(f));
  if (dt == GLB_F32) ((float *)p)[idx] = f;
  else if (dt == GLB_BF16) ((uint16_t *)p)[idx] = bf16_rne(f);
  else ((uint16_t *)p)[idx] = __half_as_ushort(__float2half_rn(f));
}

// eight codes of one word -> lane's B operand (8 values of the 16-bit dtype), each codebook[code] * absmax rounded once
template <int DT>
__device__ __forceinline__ u32x4 expand8(uint32_t word, float amax, const float *lut) {
  u32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float a = lut[(word >> (8 * i)) & 15u] * amax, b = lut[(word >> (8 * i + 4)) & 15u] * amax;
    if constexpr (DT == GLB_BF16) {
      o[i] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{a, b}, bf16x2));  // v_cvt_pk_bf16_f32 (RNE)
    } else {
      asm volatile("" : "+v"(a), "+v"(b));  // (as store_elem: no fused multiply-convert)
      o[i] = (uint32_t)__half_as_ushort(__float2half_rn(a)) | ((uint32_t)__half_as_ushort(__float2half_rn(b)) << 16);
    }
  }
  return o;
}

template <int DT>
__device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c) {
  if constexpr (DT == GLB_BF16)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

inline bool codebook_ok(const float *cb) {
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(cb[i])) return false;
  return true;
}

inline bool shape_served(int64_t n, int64_t k) { return n > 0 && k > 0 && k % QB == 0 && n <= MAX_ELEMS / k; }
// the GEMMs' shapes: whole row groups of the image, int32 offsets inside a row
inline bool gemm_shape_served(int64_t n, int64_t k) {
  return shape_served(n, k) && n % 16 == 0 && n <= (1 << 24) && k <= (1 << 24);
}

}  // namespace
