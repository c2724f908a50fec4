// glb_score.hip - score given tokens (include/glb.h: glb_score_rows).
//
// Per logits row, with y = fl32(x * scale), t the row's token and m its mask row:
//     lse = lse(y)     logp = y_t - lse(y)     logZ = lse(y + m) - lse(y)     logp_masked = (y_t + m_t) - lse(y + m)
//   score_rows_kernel  one workgroup of four waves per row.  Wave w takes the row's 4096-token chunks w, w + 4, ... in
//                      order: the chunk, its sums for y and y + m and every fold are glb_rowlse.hpp's.  The wave whose chunk
//                      holds index t takes y_t and y_t + m_t from the lane that loaded them.  The four waves' sums meet in
//                      LDS and are folded in wave order by thread 0, which writes the row's outputs.
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

struct ScoreParams : RowsParams {
  const int32_t *token;
  float *out_logp, *out_lse, *out_logZ, *out_logp_masked;
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

template <int DT, int MASK>
__global__ __launch_bounds__(64 * kWaves) void score_rows_kernel(const ScoreParams a) {
  constexpr int EPV = ElemTraits<DT>::EPV;
  __shared__ WaveSums acc[kWaves];
  __shared__ float acc_t[kWaves][2];  // y_t and y_t + m_t when one of the wave's chunks holds index t, else -inf
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, V = a.V;
  for (int64_t row = blockIdx.x; row < a.n_rows; row += gridDim.x) {  // (the same trip count for the whole workgroup)
    const int t = __builtin_amdgcn_readfirstlane(a.token[row]);
    int mid;
    const bool mask_ok = row_mask_of<MASK>(a, row, mid);
    const char *xrow = row_ptr<DT>(a.x, row, a.ld);
    float My = kNegInf, Mz = kNegInf, yt = kNegInf, zt = kNegInf;
    double Wy = 0.0, Wz = 0.0;
    for (int c = wave; c < a.nch; c += kWaves) {
      const int e_base = c * kChunk;
      float y[64];
      chunk_scaled<DT>(xrow, e_base, V, lane, a.scale, y);
      // index t, when this chunk holds it, is taken from the lane that loaded it (every other lane offers -inf)
      const bool here = t >= e_base && t < e_base + kChunk && t < V;  // (wave-uniform)
      if (here) yt = wave_max(pick_index<EPV>(y, lane, t - e_base));
      float Ny, Nz;
      uint64_t Sy, Sz;
      chunk_sums<DT, MASK>(y, mask_ok, a.mask, mid, a.mask_ld, e_base, V, lane, Ny, Sy, Nz, Sz);  // y becomes the keys y + m
      if (here) {  // (bit masks: y_t or -inf by the one bit - picking among the keys would hold all 64 to the chunk's end)
        if constexpr (MASK == GLB_MASK_F32) zt = wave_max(pick_index<EPV>(y, lane, t - e_base));
        else zt = MASK == GLB_MASK_NONE || (mask_ok && row_bit(a.mask, mid, a.mask_ld, t)) ? yt : kNegInf;
      }
      fold_chunk(Ny, Sy, My, Wy);
      fold_chunk(Nz, Sz, Mz, Wz);
    }
    if (lane == 0) {
      acc[wave] = WaveSums{Wy, Wz, My, Mz};
      acc_t[wave][0] = yt;
      acc_t[wave][1] = zt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      float Ry, Rz, ytr = kNegInf, ztr = kNegInf;
      double Ty, Tz;
      fold_waves(acc, Ty, Ry, Tz, Rz);
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        ytr = fmaxf(ytr, acc_t[w][0]);  // (-inf from every wave but the one that held index t)
        ztr = fmaxf(ztr, acc_t[w][1]);
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

}  // namespace

extern "C" {

int glb_score_rows(const glb_score_args *a, void *stream) {
  const char *const what = "glb_score_rows";
  if (const int rc = glb::block_ok(a, what, "glb_score_args")) return rc;
  if (!a->logits) return api_fail(GLB_EINVAL, "%s: logits is null", what);
  if (!a->token) return api_fail(GLB_EINVAL, "%s: token is null", what);
  const RowsView v = rows_view(a);
  if (const int rc = rows_args_ok(what, v)) return rc;
  if (a->seq_start) {
    if (a->n_seq < 0) return api_fail(GLB_EINVAL, "%s: n_seq %lld is negative", what, (long long)a->n_seq);
    if (a->n_seq > 0x7fffffffll) return api_fail(GLB_EINVAL, "%s: n_seq exceeds 31 bits", what);
    if ((a->out_seq_logp && !a->out_logp) || (a->out_seq_logZ && !a->out_logZ) || (a->out_seq_logp_masked && !a->out_logp_masked))
      return api_fail(GLB_EINVAL, "%s: a sequence sum needs its per-row output (out_seq_logp: out_logp, ...)", what);
  } else if (a->out_seq_logp || a->out_seq_logZ || a->out_seq_logp_masked) {
    return api_fail(GLB_EINVAL, "%s: sequence outputs given without seq_start", what);
  }

  const ScoreParams p{rows_params(v), a->token, a->out_logp, a->out_lse, a->out_logZ, a->out_logp_masked};
  hipStream_t s = (hipStream_t)stream;
  launch_rows(v, [&](auto dt, auto mk) {
    hipLaunchKernelGGL((score_rows_kernel<decltype(dt)::value, decltype(mk)::value>), rows_grid(p.n_rows), dim3(64 * kWaves), 0, s, p);
  });
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
