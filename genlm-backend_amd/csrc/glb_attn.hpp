// glb_attn.hpp - the DEVICE side the five attention kernels of glb_kv.hip share; included there, and by
// glb_attn_tile.hip for the 16-byte vector and pack16v.  The host side of the five entries - dispatch, checks, the chunk-shaped
// argument block - is glb_attn_host.hpp.
//   WaveShape<DT, DH>   a 16-byte vector is EPV elements, LP = head_dim / EPV lanes are one slot, PP = 64 / LP slots a wave
//   unpack16 / pack16v  a 16-byte vector as float32 and back
//   slot_score          q . k over a slot through __shfl_xor: the wave that is one query (slab, chunk, short)
//   slot_sum            a sum over a slot's lanes through DPP: the wave whose slots are queries (rows, packed)
// Templates and inlined device functions only.  The online softmax and the rows body are NOT here: see glb_kv.hip at
// slab_attention_chunk_kernel and short_attention_packed_kernel for why they stay text.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/glb.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <int DT, int DH>
struct WaveShape {
  static constexpr int ES = DT == GLB_F32 ? 4 : 2, EPV = 16 / ES, LP = DH / EPV, PP = 64 / LP;
  static_assert(LP >= 1 && LP <= 64 && PP * LP == 64, "head_dim / vector width must divide the wave");
};

template <int DT>
__device__ __forceinline__ void unpack16(const u32x4 &w, float *x) {
  const uint32_t v[4] = {w.x, w.y, w.z, w.w};
  if constexpr (DT == GLB_F32) {
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = __uint_as_float(v[k]);
  } else if constexpr (DT == GLB_BF16) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      x[2 * k] = __uint_as_float(v[k] << 16);
      x[2 * k + 1] = __uint_as_float(v[k] & 0xffff0000u);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      x[2 * k] = (float)__builtin_bit_cast(_Float16, (uint16_t)(v[k] & 0xffffu));
      x[2 * k + 1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(v[k] >> 16));
    }
  }
}

template <int DT>
__device__ __forceinline__ u32x4 pack16v(const float *x) {
  if constexpr (DT == GLB_F32) {
    return u32x4{__float_as_uint(x[0]), __float_as_uint(x[1]), __float_as_uint(x[2]), __float_as_uint(x[3])};
  } else {
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if constexpr (DT == GLB_BF16) {
        const __bf16 a = (__bf16)x[2 * k], b = (__bf16)x[2 * k + 1];
        w[k] = (uint32_t)__builtin_bit_cast(uint16_t, a) | ((uint32_t)__builtin_bit_cast(uint16_t, b) << 16);
      } else {
        const _Float16 a = (_Float16)x[2 * k], b = (_Float16)x[2 * k + 1];
        w[k] = (uint32_t)__builtin_bit_cast(uint16_t, a) | ((uint32_t)__builtin_bit_cast(uint16_t, b) << 16);
      }
    }
    return u32x4{w[0], w[1], w[2], w[3]};
  }
}

template <int LP>
__device__ __forceinline__ float slot_sum(float v) {
  // sum over the LP consecutive lanes of a slot, every lane gets it (DPP: quad_perm xor 1, xor 2, row_half_mirror, row_mirror)
  if constexpr (LP >= 2) v += __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(v), 0xB1, 0xf, 0xf, false));
  if constexpr (LP >= 4) v += __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(v), 0x4E, 0xf, 0xf, false));
  if constexpr (LP >= 8) v += __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(v), 0x141, 0xf, 0xf, false));
  if constexpr (LP >= 16) v += __uint_as_float((uint32_t)__builtin_amdgcn_update_dpp(0, (int)__float_as_uint(v), 0x140, 0xf, 0xf, false));
  if constexpr (LP >= 32) v += __shfl_xor(v, 16, 64);
  if constexpr (LP >= 64) v += __shfl_xor(v, 32, 64);
  return v;
}

// q . k over the slot: the lane's chunk in ascending k, then the LP lanes; every lane of the slot gets the score
template <int LP, int EPV>
__device__ __forceinline__ float slot_score(const float *qf, const float *kf) {
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < EPV; ++k) s = __builtin_fmaf(qf[k], kf[k], s);
#pragma unroll
  for (int o = 1; o < LP; o <<= 1) s += __shfl_xor(s, o, 64);
  return s;
}

}  // namespace
