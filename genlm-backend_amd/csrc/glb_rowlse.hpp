// glb_rowlse.hpp - the one reader of [n_rows, vocab] logits rows in 4096-token chunks, for the kernels that add a mask row and
// reduce per row: glb_importance.hip, glb_score.hip, glb_topk.hip, glb_truncate.hip.
//   the chunk     chunk_scaled: y = fl32(x * scale) in 16-byte loads, the lane layout of glb_chunk.hpp (lane l holds vector i =
//                 elements (i * 64 + l) * EPV ..), -inf beyond the row.  chunk_add_mask: y becomes the keys y + m for a
//                 GLB_MASK_* kind; lane_mask_words is the one place that knows which words hold a lane's bits.
//   the sums      chunk_sums: for y and y + m the chunk's binary scale N = exp_n(max) and the integer sum of the terms
//                 2^(x log2 e - N - 1) (the hardware's v_exp_f32, glb_math.hpp kExpHw).  A lane adds its 64 terms in float32 as
//                 four chains of sixteen in load order, the four in a fixed tree; floor(lane sum * 2^40) is summed over the wave
//                 as an integer.  With bit masks whose allowed maximum lies in the chunk's top binade (nearly always) one term
//                 serves both sums: two exponentials an element pair instead of three.
//   the folds     fold_chunk: a chunk's (scale, sum) into a wave's running (scale, double sum), chunk order the caller's.
//                 WaveSums / fold_waves: the waves of a row's workgroup meet in LDS and thread 0 folds them in wave order;
//                 lse_of: one double logarithm.  rec_mass: the same against a unit's scale, for records kept in memory.
//   the launch    RowsParams / row_mask_of: what every kernel of one workgroup per row takes, and the row's mask id.
//                 RowsView / rows_args_ok / rows_params / launch_rows (host): the argument checks glb_score_rows, glb_topk_rows
//                 and glb_truncate_rows share, and the one dispatch over (dtype, mask_kind).
// Which wave holds which chunk and the order of every fold are fixed by the chunk index, not by the grid.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "../../include/glb.h"
#include "glb_chunk.hpp"
#include "glb_common.hpp"

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

// the wave's 64 values a lane of the chunk at e_base: y = fl32(x * scale) (times 1.0f: the same bits), -inf beyond the row
template <int DT>
__device__ __forceinline__ void chunk_scaled(const char *xrow, int e_base, int V, int lane, float scale, float (&y)[64]) {
  constexpr int EPV = ElemTraits<DT>::EPV, NVC = ElemTraits<DT>::NVC;
  u32x4_t raw[NVC];
  load_chunk_raw<DT>(xrow, e_base, V, lane, raw);
#pragma unroll
  for (int i = 0; i < NVC; ++i) unpack_vec<DT>(raw[i], &y[i * EPV]);
#pragma unroll
  for (int j = 0; j < 64; ++j) y[j] *= scale;
}

// the words that hold this lane's bits of mask row `mid`, shifted so that bit q of mw[i] is element q of the lane's vector i:
// vector i covers EPV bits from bit (lane * EPV) % 32 of word e_base / 32 + i * (64 * EPV / 32) + lane * EPV / 32
template <int DT>
__device__ __forceinline__ void lane_mask_words(const void *mask, int mid, int64_t mask_ld, int e_base, int V, int lane,
                                                uint32_t (&mw)[ElemTraits<DT>::NVC]) {
  constexpr int EPV = ElemTraits<DT>::EPV, NVC = ElemTraits<DT>::NVC;
  const uint32_t *mrow = reinterpret_cast<const uint32_t *>(mask) + (int64_t)mid * mask_ld;
  const int nw = (V + 31) >> 5, w0 = (e_base >> 5) + ((lane * EPV) >> 5), sh = (lane * EPV) & 31;
#pragma unroll
  for (int i = 0; i < NVC; ++i) {
    const int wi = w0 + i * (64 * EPV / 32);
    mw[i] = wi < nw ? mrow[wi] >> sh : 0u;
  }
}

// bit e < V of mask row `mid` (bit e % 32 of word e / 32)
__device__ __forceinline__ bool row_bit(const void *mask, int mid, int64_t mask_ld, int e) {
  return (reinterpret_cast<const uint32_t *>(mask)[(int64_t)mid * mask_ld + (e >> 5)] >> (e & 31)) & 1u;
}

template <int EPV, int NVC>
__device__ __forceinline__ bool lane_bit(const uint32_t (&mw)[NVC], int j) {
  return (mw[j / EPV] >> (j % EPV)) & 1u;
}

// y becomes the keys y + m in place: MASK a GLB_MASK_* kind (raw bit rows or float rows), `mid` the row's mask, !mask_ok a
// mask that allows nothing
template <int DT, int MASK>
__device__ __forceinline__ void chunk_add_mask(float (&y)[64], bool mask_ok, const void *mask, int mid, int64_t mask_ld, int e_base,
                                               int V, int lane) {
  constexpr int EPV = ElemTraits<DT>::EPV, NVC = ElemTraits<DT>::NVC;
  if constexpr (MASK == GLB_MASK_NONE) return;
  if (!mask_ok) {
#pragma unroll
    for (int j = 0; j < 64; ++j) y[j] = kNegInf;
  } else if constexpr (MASK == GLB_MASK_BITS) {
    uint32_t mw[NVC];
    lane_mask_words<DT>(mask, mid, mask_ld, e_base, V, lane, mw);
#pragma unroll
    for (int j = 0; j < 64; ++j) y[j] = lane_bit<EPV>(mw, j) ? y[j] : kNegInf;
  } else {  // GLB_MASK_F32: the floats in y's lane layout
    const char *mrow = reinterpret_cast<const char *>(reinterpret_cast<const float *>(mask) + (int64_t)mid * mask_ld);
#pragma unroll
    for (int i = 0; i < NVC; ++i) {
#pragma unroll
      for (int h = 0; h < EPV / 4; ++h) {
        float m[4];
        unpack_vec<kDtF32>(load_vec_guarded<kDtF32>(mrow, e_base + (i * 64 + lane) * EPV + 4 * h, V), m);
#pragma unroll
        for (int q = 0; q < 4; ++q) y[i * EPV + 4 * h + q] += m[q];
      }
    }
  }
}

// a chunk's binary scales and integer sums of y (Ny, Sy) and of the keys y + m (Nz, Sz); y leaves as the keys, as
// chunk_add_mask makes them (a caller that does not read them pays nothing)
template <int DT, int MASK>
__device__ __forceinline__ void chunk_sums(float (&y)[64], bool mask_ok, const void *mask, int mid, int64_t mask_ld, int e_base, int V,
                                           int lane, float &Ny, uint64_t &Sy, float &Nz, uint64_t &Sz) {
  constexpr int EPV = ElemTraits<DT>::EPV, NVC = ElemTraits<DT>::NVC;
  Ny = exp_n(wave_max(lane_max64(y)));
  Nz = kNegInf;
  Sy = Sz = 0;
  if constexpr (MASK == GLB_MASK_NONE) {
    if (Ny != kNegInf) Sy = wave_fix_sum(lane_sum64<EPV>(y, Ny));
    Nz = Ny;
    Sz = Sy;
  } else if (!mask_ok) {
    if (Ny != kNegInf) Sy = wave_fix_sum(lane_sum64<EPV>(y, Ny));
    chunk_add_mask<DT, MASK>(y, false, mask, mid, mask_ld, e_base, V, lane);
  } else if constexpr (MASK == GLB_MASK_BITS) {
    uint32_t mw[NVC];
    lane_mask_words<DT>(mask, mid, mask_ld, e_base, V, lane, mw);
    float zm = kNegInf;
#pragma unroll
    for (int j = 0; j < 64; ++j) zm = fmaxf(zm, lane_bit<EPV>(mw, j) ? y[j] : kNegInf);
    Nz = exp_n(wave_max(zm));
    if (Nz == Ny) {  // the allowed maximum lies in the chunk's top binade: one term serves both sums
      if (Ny != kNegInf) {
        const float bias = term_bias<kExpHw>(Ny);
        float cy[4] = {0.0f, 0.0f, 0.0f, 0.0f}, cz[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < 64; ++j) {
          const float t = chunk_term<kExpHw>(y[j], bias);
          cy[(j / EPV) & 3] += t;
          cz[(j / EPV) & 3] += lane_bit<EPV>(mw, j) ? t : 0.0f;
        }
        Sy = wave_fix_sum((cy[0] + cy[1]) + (cy[2] + cy[3]));
        Sz = wave_fix_sum((cz[0] + cz[1]) + (cz[2] + cz[3]));
      }
#pragma unroll
      for (int j = 0; j < 64; ++j) y[j] = lane_bit<EPV>(mw, j) ? y[j] : kNegInf;
    } else {
      Sy = wave_fix_sum(lane_sum64<EPV>(y, Ny));  // (Nz < Ny: Ny is finite)
#pragma unroll
      for (int j = 0; j < 64; ++j) y[j] = lane_bit<EPV>(mw, j) ? y[j] : kNegInf;
      if (Nz != kNegInf) Sz = wave_fix_sum(lane_sum64<EPV>(y, Nz));
    }
  } else {  // GLB_MASK_F32
    if (Ny != kNegInf) Sy = wave_fix_sum(lane_sum64<EPV>(y, Ny));
    chunk_add_mask<DT, MASK>(y, true, mask, mid, mask_ld, e_base, V, lane);
    Nz = exp_n(wave_max(lane_max64(y)));
    if (Nz != kNegInf) Sz = wave_fix_sum(lane_sum64<EPV>(y, Nz));
  }
}

// a chunk's (scale, integer sum) into a running (scale, double sum); chunk order is the caller's
__device__ __forceinline__ void fold_chunk(float N, uint64_t S, float &M, double &W) {
  if (S == 0) return;
  if (N > M) {
    W = W > 0.0 ? ldexp(W, (int)fmaxf(M - N, -4000.0f)) : 0.0;
    M = N;
  }
  W += rec_mass(S, N, M);
}

struct alignas(16) WaveSums {  // what one wave hands to the row's last fold
  double Wy, Wz;               // sums of the wave's chunks on the scales My, Mz
  float My, Mz;
};

// the waves' sums in wave order against the largest scale of a wave that holds anything: totals Ty, Tz on the scales Ry, Rz
template <int NW>
__device__ __forceinline__ void fold_waves(const WaveSums (&acc)[NW], double &Ty, float &Ry, double &Tz, float &Rz) {
  Ry = Rz = kNegInf;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    Ry = fmaxf(Ry, acc[w].Wy > 0.0 ? acc[w].My : kNegInf);
    Rz = fmaxf(Rz, acc[w].Wz > 0.0 ? acc[w].Mz : kNegInf);
  }
  Ty = Tz = 0.0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {  // wave order
    if (acc[w].Wy > 0.0) Ty += ldexp(acc[w].Wy, (int)fmaxf(acc[w].My - Ry, -4000.0f));
    if (acc[w].Wz > 0.0) Tz += ldexp(acc[w].Wz, (int)fmaxf(acc[w].Mz - Rz, -4000.0f));
  }
}

// what a kernel of one workgroup per logits row takes: its own parameter block derives from this
struct RowsParams {
  const void *x;
  int64_t ld;
  int32_t V, nch;
  float scale;
  int64_t n_rows;
  int32_t n_masks;
  const int32_t *row_mask;  // [n_rows], null = (n_masks == 1 ? 0 : identity)
  const void *mask;
  int64_t mask_ld;
};

// the row's mask id (wave-uniform); false: out of range, a row whose mask allows nothing
template <int MASK>
__device__ __forceinline__ bool row_mask_of(const RowsParams &p, int64_t row, int &mid) {
  mid = 0;
  if constexpr (MASK == GLB_MASK_NONE) return true;
  mid = __builtin_amdgcn_readfirstlane(p.row_mask ? p.row_mask[row] : (p.n_masks == 1 ? 0 : (int)row));
  return mid >= 0 && mid < p.n_masks;
}

// ---- host: the argument fields glb_score_args, glb_topk_args and glb_truncate_args share ----
struct RowsView {
  const void *logits;
  int32_t dtype;
  int64_t n_rows, vocab, ld;
  float logit_scale;
  int32_t mask_kind;
  const void *mask;
  int64_t mask_ld, n_masks;
  const int32_t *row_mask_id;
};

template <class Args>
RowsView rows_view(const Args *a) {
  return RowsView{a->logits, a->dtype,   a->n_rows,  a->vocab,      a->ld, a->logit_scale,
                  a->mask_kind, a->mask, a->mask_ld, a->n_masks, a->row_mask_id};
}

// 0, or the failure's code with its message set
inline int rows_args_ok(const char *what, const RowsView &a) {
  if (a.dtype < GLB_F32 || a.dtype > GLB_F16) return api_fail(GLB_EINVAL, "%s: bad dtype %d", what, a.dtype);
  if (a.n_rows <= 0 || a.vocab <= 0)
    return api_fail(GLB_EINVAL, "%s: n_rows=%lld vocab=%lld must be positive", what, (long long)a.n_rows, (long long)a.vocab);
  if (a.vocab > 0x7fffff00ll || a.n_rows > 0x7fffffffll) return api_fail(GLB_EINVAL, "%s: vocab / n_rows exceed 31 bits", what);
  if (a.ld < a.vocab) return api_fail(GLB_EINVAL, "%s: ld %lld < vocab %lld", what, (long long)a.ld, (long long)a.vocab);
  if (((uintptr_t)a.logits) % (a.dtype == GLB_F32 ? 4 : 2)) return api_fail(GLB_EINVAL, "%s: logits pointer not element aligned", what);
  if (!(a.logit_scale == a.logit_scale)) return api_fail(GLB_EINVAL, "%s: logit_scale is NaN", what);
  if (!(a.logit_scale > 0.0f) || a.logit_scale > 3.0e38f)
    return api_fail(GLB_EINVAL, "%s: logit_scale %g must be positive and finite (0 or a negative scale turns -inf logits into NaN / +inf)", what,
                    (double)a.logit_scale);
  if (a.mask_kind == GLB_MASK_PREPARED)
    return api_fail(GLB_EINVAL, "%s: GLB_MASK_PREPARED is the fused step's layout; give the bit rows (GLB_MASK_BITS)", what);
  if (a.mask_kind < GLB_MASK_NONE || a.mask_kind > GLB_MASK_F32) return api_fail(GLB_EINVAL, "%s: bad mask_kind %d", what, a.mask_kind);
  if (a.mask_kind != GLB_MASK_NONE) {
    if (!a.mask || a.n_masks <= 0) return api_fail(GLB_EINVAL, "%s: mask table missing", what);
    const int64_t need = a.mask_kind == GLB_MASK_BITS ? (a.vocab + 31) / 32 : a.vocab;
    if (a.mask_ld < need) return api_fail(GLB_EINVAL, "%s: mask_ld %lld < %lld", what, (long long)a.mask_ld, (long long)need);
    if (!a.row_mask_id && a.n_masks != 1 && a.n_masks != a.n_rows)
      return api_fail(GLB_EINVAL, "%s: no mask ids given but n_masks is neither 1 nor the number of rows", what);
    if (((uintptr_t)a.mask) % 4) return api_fail(GLB_EINVAL, "%s: mask pointer misaligned", what);
    if (a.n_masks > 0x7fffffffll) return api_fail(GLB_EINVAL, "%s: n_masks exceeds 31 bits", what);
  }
  return 0;
}

inline RowsParams rows_params(const RowsView &a) {  // (of a view that passed rows_args_ok)
  return RowsParams{a.logits, a.ld, (int32_t)a.vocab, (int32_t)((a.vocab + kChunk - 1) / kChunk), a.logit_scale, a.n_rows, (int32_t)a.n_masks,
                    a.mask_kind == GLB_MASK_NONE ? nullptr : a.row_mask_id, a.mask, a.mask_ld};
}

// launch(DT, MASK) with the view's element type and mask kind as std::integral_constant<int, .>, and the launch's geometry:
// one workgroup a row, at most 2^20 of them
template <class F>
void launch_rows(const RowsView &a, F &&launch) {
  const auto with_mask = [&](auto dt) {
    switch (a.mask_kind) {
      case GLB_MASK_NONE: return launch(dt, std::integral_constant<int, GLB_MASK_NONE>{});
      case GLB_MASK_BITS: return launch(dt, std::integral_constant<int, GLB_MASK_BITS>{});
      default: return launch(dt, std::integral_constant<int, GLB_MASK_F32>{});
    }
  };
  switch (a.dtype) {
    case GLB_F32: return with_mask(std::integral_constant<int, kDtF32>{});
    case GLB_BF16: return with_mask(std::integral_constant<int, kDtBf16>{});
    default: return with_mask(std::integral_constant<int, kDtF16>{});
  }
}
inline dim3 rows_grid(int64_t n_rows) { return dim3((unsigned)(n_rows < (1 << 20) ? n_rows : (1 << 20))); }

}  // namespace glb
