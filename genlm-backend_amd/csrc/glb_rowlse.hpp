// glb_rowlse.hpp - a row's log-sum-exp from its 4096-token chunks, as glb_importance.hip and glb_score.hip take it: a lane's 64
// terms 2^(x log2 e - N - 1) against the chunk's binary scale N (the hardware's v_exp_f32, glb_math.hpp kExpHw) in float32 as
// four chains of sixteen in load order, floor(lane sum * 2^40) summed over the wave as an integer, the chunks' sums folded in
// double against the largest scale, one double logarithm.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "glb_chunk.hpp"

namespace glb {

constexpr double kFixOne = 1099511627776.0;  // 2^40: a lane's float32 sum (< 46) as an integer below 2^46

__device__ __forceinline__ float lane_max64(const float (&x)[64]) {
  float m0 = x[0], m1 = x[1];
#pragma unroll
  for (int j = 2; j < 64; j += 2) {
    m0 = fmaxf(m0, x[j]);
    m1 = fmaxf(m1, x[j + 1]);
  }
  return fmaxf(m0, m1);
}

// a lane's 64 terms against the scale N: four float32 chains (vector i of the lane goes to chain i mod 4, sixteen terms each, in
// load order), added as (c0 + c1) + (c2 + c3)
template <int EPV>
__device__ __forceinline__ float lane_sum64(const float (&x)[64], float N) {
  const float bias = term_bias<kExpHw>(N);
  float c[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int j = 0; j < 64; ++j) c[(j / EPV) & 3] += chunk_term<kExpHw>(x[j], bias);
  return (c[0] + c[1]) + (c[2] + c[3]);
}

__device__ __forceinline__ uint64_t wave_fix_sum(float lane_sum) { return wave_sum_u64((uint64_t)((double)lane_sum * kFixOne)); }

template <int DT>
__device__ __forceinline__ const char *row_ptr(const void *base, int64_t row, int64_t ld) {
  return reinterpret_cast<const char *>(base) + row * ld * ElemTraits<DT>::ES;
}

// S * 2^(N - M) for a record's sum against the unit's scale M >= N (both integer valued or -inf)
__device__ __forceinline__ double rec_mass(uint64_t S, float N, float M) {
  if (S == 0) return 0.0;
  return ldexp((double)S, (int)fmaxf(N - M, -4000.0f));
}

// ln of the sum whose terms were 2^(x log2 e - M - 1) * 2^40
__device__ __forceinline__ double lse_of(double W, float M) {
  return W > 0.0 ? ((double)M - 39.0) * kLn2D + log(W) : (double)kNegInf;
}

}  // namespace glb
