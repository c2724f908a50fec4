// glb_score.hip - score given tokens (include/glb.h: glb_score_rows).
//
// Per logits row, with y = fl32(x * scale), t the row's token and m its mask row:
//     lse = lse(y)     logp = y_t - lse(y)     logZ = lse(y + m) - lse(y)     logp_masked = (y_t + m_t) - lse(y + m)
//   score_rows_kernel  one workgroup of four waves per row.  Wave w takes the row's 4096-token chunks w, w + 4, ... in
//                      order: the chunk in 16-byte loads (the lane layout of glb_chunk.hpp), with its mask words or floats,
//                      and for y and y + m the chunk's binary scale and integer sum (glb_rowlse.hpp: glb_importance.hip's
//                      terms, two exponentials an element pair with bit masks whose allowed maximum lies in the chunk's top
//                      binade), folded into the wave's running (scale, double sum).  The wave whose chunk holds index t
//                      takes y_t and y_t + m_t from the lane that loaded them.  The four waves' sums meet in LDS and are
//                      folded in wave order by thread 0, which writes the row's outputs.
//   seq_sums_kernel    (once per sequence sum asked for) one thread per sequence: its rows' values added in double in row order.
// A row's outputs depend on that row's logits, token and mask row only: which wave holds which chunk and the order of every
// fold are fixed by the chunk index, not by the grid, so the bits do not depend on what else the call holds.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/glb.h"
#include "glb_chunk.hpp"
#include "glb_common.hpp"
#include "glb_rowlse.hpp"

namespace {
using namespace glb;

constexpr int kWaves = 4;  // waves per row: part of the reduction tree, not a tuning knob (changing it changes bits)

struct ScoreParams {
  const void *x;
  int64_t ld;
  int32_t V, nch;
  float scale;
  int64_t n_rows;
  int32_t n_masks;
  const int32_t *token;
  const int32_t *row_mask;  // [n_rows], null = (n_masks == 1 ? 0 : identity)
  const void *mask;
  int64_t mask_ld;
  float *out_logp, *out_lse, *out_logZ, *out_logp_masked;
};

struct alignas(16) WaveAcc {  // what one wave hands to the row's last fold
  double Wy, Wz;              // sums of the wave's chunks on the scales My, Mz
  float My, Mz;
  float yt, zt;  // y_t and y_t + m_t when one of the wave's chunks holds index t, else -inf
};

// the element of chunk index tl among a lane's 64 (vector i of the lane holds indices (i * 64 + lane) * EPV ..), -inf on the
// lanes that do not hold it; compared by index, element by element: a wave-uniform register number would make the
// compiler keep the 64 values in scratch
template <int EPV>
__device__ __forceinline__ float pick_index(const float (&x)[64], int lane, int tl) {
  float v = kNegInf;
#pragma unroll
  for (int j = 0; j < 64; ++j) v = ((j / EPV) * 64 + lane) * EPV + j % EPV == tl ? x[j] : v;
  return v;
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

template <int DT, int MASK>
__global__ __launch_bounds__(64 * kWaves) void score_rows_kernel(const ScoreParams a) {
  constexpr int EPV = ElemTraits<DT>::EPV, NVC = ElemTraits<DT>::NVC;
  __shared__ WaveAcc acc[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, V = a.V;
  for (int64_t row = blockIdx.x; row < a.n_rows; row += gridDim.x) {  // (the same trip count for the whole workgroup)
    const int t = __builtin_amdgcn_readfirstlane(a.token[row]);
    int mid = 0;
    bool mask_ok = true;
    if constexpr (MASK != GLB_MASK_NONE) {
      mid = __builtin_amdgcn_readfirstlane(a.row_mask ? a.row_mask[row] : (a.n_masks == 1 ? 0 : (int)row));
      mask_ok = mid >= 0 && mid < a.n_masks;  // out of range: a row whose mask allows nothing
    }
    const char *xrow = row_ptr<DT>(a.x, row, a.ld);
    float My = kNegInf, Mz = kNegInf, yt = kNegInf, zt = kNegInf;
    double Wy = 0.0, Wz = 0.0;
    for (int c = wave; c < a.nch; c += kWaves) {
      const int e_base = c * kChunk;
      float y[64];
      {
        u32x4_t raw[NVC];
        load_chunk_raw<DT>(xrow, e_base, V, lane, raw);
#pragma unroll
        for (int i = 0; i < NVC; ++i) unpack_vec<DT>(raw[i], &y[i * EPV]);
      }
#pragma unroll
      for (int j = 0; j < 64; ++j) y[j] *= a.scale;  // (times 1.0f: the same bits)
      // index t, when this chunk holds it, is taken from the lane that loaded it (every other lane offers -inf)
      const bool here = t >= e_base && t < e_base + kChunk && t < V;  // (wave-uniform)
      const int tl = t - e_base;
      float ytl = kNegInf;
      if (here) {
        ytl = pick_index<EPV>(y, lane, tl);
        yt = wave_max(ytl);
      }
      const float Ny = exp_n(wave_max(lane_max64(y)));
      float Nz = kNegInf;
      uint64_t Sy = 0, Sz = 0;
      if constexpr (MASK == GLB_MASK_NONE) {
        if (Ny != kNegInf) Sy = wave_fix_sum(lane_sum64<EPV>(y, Ny));
        Nz = Ny;
        Sz = Sy;
        if (here) zt = yt;
      } else if (!mask_ok) {
        if (Ny != kNegInf) Sy = wave_fix_sum(lane_sum64<EPV>(y, Ny));
      } else if constexpr (MASK == GLB_MASK_BITS) {
        // the words that hold this lane's bits: vector i covers EPV bits from bit (lane * EPV) % 32 of word
        // e_base / 32 + i * (64 * EPV / 32) + lane * EPV / 32
        const uint32_t *mrow = reinterpret_cast<const uint32_t *>(a.mask) + (int64_t)mid * a.mask_ld;
        const int nw = (V + 31) >> 5, w0 = (e_base >> 5) + ((lane * EPV) >> 5), sh = (lane * EPV) & 31;
        uint32_t mw[NVC];
#pragma unroll
        for (int i = 0; i < NVC; ++i) {
          const int wi = w0 + i * (64 * EPV / 32);
          mw[i] = wi < nw ? mrow[wi] >> sh : 0u;
        }
        if (here) {
          float ztl = kNegInf;
#pragma unroll
          for (int j = 0; j < 64; ++j)
            ztl = (((j / EPV) * 64 + lane) * EPV + j % EPV == tl && ((mw[j / EPV] >> (j % EPV)) & 1u)) ? y[j] : ztl;
          zt = wave_max(ztl);
        }
        float zm = kNegInf;
#pragma unroll
        for (int j = 0; j < 64; ++j) zm = fmaxf(zm, ((mw[j / EPV] >> (j % EPV)) & 1u) ? y[j] : kNegInf);
        Nz = exp_n(wave_max(zm));
        if (Nz == Ny) {  // the allowed maximum lies in the chunk's top binade: one term serves both sums
          if (Ny != kNegInf) {
            const float bias = term_bias<kExpHw>(Ny);
            float cy[4] = {0.0f, 0.0f, 0.0f, 0.0f}, cz[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < 64; ++j) {
              const float tm = chunk_term<kExpHw>(y[j], bias);
              cy[(j / EPV) & 3] += tm;
              cz[(j / EPV) & 3] += ((mw[j / EPV] >> (j % EPV)) & 1u) ? tm : 0.0f;
            }
            Sy = wave_fix_sum((cy[0] + cy[1]) + (cy[2] + cy[3]));
            Sz = wave_fix_sum((cz[0] + cz[1]) + (cz[2] + cz[3]));
          }
        } else {
          Sy = wave_fix_sum(lane_sum64<EPV>(y, Ny));  // (Nz < Ny: Ny is finite)
#pragma unroll
          for (int j = 0; j < 64; ++j) y[j] = ((mw[j / EPV] >> (j % EPV)) & 1u) ? y[j] : kNegInf;
          if (Nz != kNegInf) Sz = wave_fix_sum(lane_sum64<EPV>(y, Nz));
        }
      } else {  // GLB_MASK_F32: z = y + m, the floats in y's lane layout
        if (Ny != kNegInf) Sy = wave_fix_sum(lane_sum64<EPV>(y, Ny));
        const char *mrow = reinterpret_cast<const char *>(reinterpret_cast<const float *>(a.mask) + (int64_t)mid * a.mask_ld);
#pragma unroll
        for (int i = 0; i < NVC; ++i) {
#pragma unroll
          for (int h = 0; h < EPV / 4; ++h) {
            float m[4];
            unpack_vec<kDtF32>(load_vec_guarded<kDtF32>(mrow, e_base + (i * 64 + lane) * EPV + 4 * h, V), m);
#pragma unroll
            for (int k = 0; k < 4; ++k) y[i * EPV + 4 * h + k] += m[k];
          }
        }
        if (here) zt = wave_max(pick_index<EPV>(y, lane, tl));
        Nz = exp_n(wave_max(lane_max64(y)));
        if (Nz != kNegInf) Sz = wave_fix_sum(lane_sum64<EPV>(y, Nz));
      }
      fold_chunk(Ny, Sy, My, Wy);
      fold_chunk(Nz, Sz, Mz, Wz);
    }
    if (lane == 0) acc[wave] = WaveAcc{Wy, Wz, My, Mz, yt, zt};
    __syncthreads();
    if (threadIdx.x == 0) {
      float Ry = kNegInf, Rz = kNegInf, ytr = kNegInf, ztr = kNegInf;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        Ry = fmaxf(Ry, acc[w].Wy > 0.0 ? acc[w].My : kNegInf);
        Rz = fmaxf(Rz, acc[w].Wz > 0.0 ? acc[w].Mz : kNegInf);
        ytr = fmaxf(ytr, acc[w].yt);  // (-inf from every wave but the one that held index t)
        ztr = fmaxf(ztr, acc[w].zt);
      }
      double Ty = 0.0, Tz = 0.0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {  // wave order
        if (acc[w].Wy > 0.0) Ty += ldexp(acc[w].Wy, (int)fmaxf(acc[w].My - Ry, -4000.0f));
        if (acc[w].Wz > 0.0) Tz += ldexp(acc[w].Wz, (int)fmaxf(acc[w].Mz - Rz, -4000.0f));
      }
      const double lse_y = lse_of(Ty, Ry), lse_z = lse_of(Tz, Rz);
      if (a.out_lse) a.out_lse[row] = (float)lse_y;
      if (a.out_logp) a.out_logp[row] = (ytr == kNegInf || !(Ty > 0.0)) ? kNegInf : (float)((double)ytr - lse_y);
      if (a.out_logZ) a.out_logZ[row] = Tz > 0.0 ? (float)(lse_z - lse_y) : kNegInf;
      if (a.out_logp_masked)
        a.out_logp_masked[row] = (ztr == kNegInf || !(Tz > 0.0)) ? kNegInf : (float)((double)ztr - lse_z);
    }
    __syncthreads();  // (acc is written again for the workgroup's next row)
  }
}

// rows [lo, hi) of one per-row output, added in double in row order and rounded once (-inf + finite = -inf; none: 0)
__device__ __forceinline__ float seq_sum(const float *v, int64_t lo, int64_t hi) {
  double s = 0.0;
  for (int64_t r = lo; r < hi; ++r) s += (double)v[r];
  return (float)s;
}

__global__ __launch_bounds__(256) void seq_sums_kernel(const float *v, int64_t n_rows, const int64_t *seq_start, int64_t n_seq,
                                                       float *out) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= n_seq) return;
  const auto clip = [&](int64_t r) { return r < 0 ? (int64_t)0 : (r > n_rows ? n_rows : r); };
  out[s] = seq_sum(v, clip(seq_start[s]), clip(seq_start[s + 1]));
}

template <int DT>
void launch_rows(int mask_kind, const ScoreParams &p, hipStream_t s) {
  const dim3 grid((unsigned)(p.n_rows < (1 << 20) ? p.n_rows : (1 << 20))), block(64 * kWaves);
  switch (mask_kind) {
    case GLB_MASK_NONE: hipLaunchKernelGGL((score_rows_kernel<DT, GLB_MASK_NONE>), grid, block, 0, s, p); break;
    case GLB_MASK_BITS: hipLaunchKernelGGL((score_rows_kernel<DT, GLB_MASK_BITS>), grid, block, 0, s, p); break;
    default: hipLaunchKernelGGL((score_rows_kernel<DT, GLB_MASK_F32>), grid, block, 0, s, p); break;
  }
}

}  // namespace

extern "C" {

int glb_score_rows(const glb_score_args *a, void *stream) {
  const char *const what = "glb_score_rows";
  if (const int rc = glb::block_ok(a, what, "glb_score_args")) return rc;
  if (!a->logits) return api_fail(GLB_EINVAL, "%s: logits is null", what);
  if (!a->token) return api_fail(GLB_EINVAL, "%s: token is null", what);
  if (a->dtype < GLB_F32 || a->dtype > GLB_F16) return api_fail(GLB_EINVAL, "%s: bad dtype %d", what, a->dtype);
  if (a->n_rows <= 0 || a->vocab <= 0)
    return api_fail(GLB_EINVAL, "%s: n_rows=%lld vocab=%lld must be positive", what, (long long)a->n_rows, (long long)a->vocab);
  if (a->vocab > 0x7fffff00ll || a->n_rows > 0x7fffffffll) return api_fail(GLB_EINVAL, "%s: vocab / n_rows exceed 31 bits", what);
  if (a->ld < a->vocab) return api_fail(GLB_EINVAL, "%s: ld %lld < vocab %lld", what, (long long)a->ld, (long long)a->vocab);
  if (((uintptr_t)a->logits) % (a->dtype == GLB_F32 ? 4 : 2)) return api_fail(GLB_EINVAL, "%s: logits pointer not element aligned", what);
  if (!(a->logit_scale == a->logit_scale)) return api_fail(GLB_EINVAL, "%s: logit_scale is NaN", what);
  if (!(a->logit_scale > 0.0f) || a->logit_scale > 3.0e38f)
    return api_fail(GLB_EINVAL, "%s: logit_scale %g must be positive and finite (0 or a negative scale turns -inf logits into NaN / +inf)", what,
                    (double)a->logit_scale);
  if (a->mask_kind == GLB_MASK_PREPARED)
    return api_fail(GLB_EINVAL, "%s: GLB_MASK_PREPARED is the fused step's layout; give the bit rows (GLB_MASK_BITS)", what);
  if (a->mask_kind < GLB_MASK_NONE || a->mask_kind > GLB_MASK_F32) return api_fail(GLB_EINVAL, "%s: bad mask_kind %d", what, a->mask_kind);
  if (a->mask_kind != GLB_MASK_NONE) {
    if (!a->mask || a->n_masks <= 0) return api_fail(GLB_EINVAL, "%s: mask table missing", what);
    const int64_t need = a->mask_kind == GLB_MASK_BITS ? (a->vocab + 31) / 32 : a->vocab;
    if (a->mask_ld < need) return api_fail(GLB_EINVAL, "%s: mask_ld %lld < %lld", what, (long long)a->mask_ld, (long long)need);
    if (!a->row_mask_id && a->n_masks != 1 && a->n_masks != a->n_rows)
      return api_fail(GLB_EINVAL, "%s: no mask ids given but n_masks is neither 1 nor the number of rows", what);
    if (((uintptr_t)a->mask) % 4) return api_fail(GLB_EINVAL, "%s: mask pointer misaligned", what);
    if (a->n_masks > 0x7fffffffll) return api_fail(GLB_EINVAL, "%s: n_masks exceeds 31 bits", what);
  }
  if (a->seq_start) {
    if (a->n_seq < 0) return api_fail(GLB_EINVAL, "%s: n_seq %lld is negative", what, (long long)a->n_seq);
    if (a->n_seq > 0x7fffffffll) return api_fail(GLB_EINVAL, "%s: n_seq exceeds 31 bits", what);
    if ((a->out_seq_logp && !a->out_logp) || (a->out_seq_logZ && !a->out_logZ) || (a->out_seq_logp_masked && !a->out_logp_masked))
      return api_fail(GLB_EINVAL, "%s: a sequence sum needs its per-row output (out_seq_logp: out_logp, ...)", what);
  } else if (a->out_seq_logp || a->out_seq_logZ || a->out_seq_logp_masked) {
    return api_fail(GLB_EINVAL, "%s: sequence outputs given without seq_start", what);
  }

  ScoreParams p{};
  p.x = a->logits;
  p.ld = a->ld;
  p.V = (int32_t)a->vocab;
  p.nch = (int32_t)((a->vocab + kChunk - 1) / kChunk);
  p.scale = a->logit_scale;
  p.n_rows = a->n_rows;
  p.n_masks = (int32_t)a->n_masks;
  p.token = a->token;
  p.row_mask = a->mask_kind == GLB_MASK_NONE ? nullptr : a->row_mask_id;
  p.mask = a->mask;
  p.mask_ld = a->mask_ld;
  p.out_logp = a->out_logp;
  p.out_lse = a->out_lse;
  p.out_logZ = a->out_logZ;
  p.out_logp_masked = a->out_logp_masked;
  hipStream_t s = (hipStream_t)stream;
  switch (a->dtype) {
    case GLB_F32: launch_rows<kDtF32>(a->mask_kind, p, s); break;
    case GLB_BF16: launch_rows<kDtBf16>(a->mask_kind, p, s); break;
    default: launch_rows<kDtF16>(a->mask_kind, p, s); break;
  }
  if (a->seq_start && a->n_seq > 0) {
    const float *const rows[3] = {a->out_logp, a->out_logZ, a->out_logp_masked};
    float *const sums[3] = {a->out_seq_logp, a->out_seq_logZ, a->out_seq_logp_masked};
    for (int k = 0; k < 3; ++k)
      if (sums[k])
        hipLaunchKernelGGL(seq_sums_kernel, dim3(blocks_for(a->n_seq, 256)), dim3(256), 0, s, rows[k], a->n_rows, a->seq_start, a->n_seq,
                           sums[k]);
  }
  return glb::launched(what);
}

int glb_score_seq_sums(const float *values, int64_t n_rows, const int64_t *seq_start, int64_t n_seq, float *out, void *stream) {
  const char *const what = "glb_score_seq_sums";
  if (!values || !seq_start || !out) return api_fail(GLB_EINVAL, "%s: null values, seq_start or out", what);
  if (n_rows < 0 || n_seq < 0 || n_rows > 0x7fffffffll || n_seq > 0x7fffffffll)
    return api_fail(GLB_EINVAL, "%s: n_rows=%lld n_seq=%lld negative or beyond 31 bits", what, (long long)n_rows, (long long)n_seq);
  if (n_seq == 0) return GLB_OK;
  hipLaunchKernelGGL(seq_sums_kernel, dim3(blocks_for(n_seq, 256)), dim3(256), 0, (hipStream_t)stream, values, n_rows, seq_start, n_seq,
                     out);
  return glb::launched(what);
}

}  // extern "C"
