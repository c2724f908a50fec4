// glb_topk.hip - the k most probable tokens of every logits row, and a beam step's selection (include/glb.h: glb_topk_rows,
// glb_beam_select).
//
// Per logits row, with y = fl32(x * scale), m its mask row and key = fl32(y + m):
//   topk_rows_kernel    one workgroup of four waves per row: wave w takes the row's 4096-token chunks w, w + 4, ... in
//                       order - the chunk, its sums for y and y + m and every fold are glb_rowlse.hpp's - and offers the
//                       chunk's keys to the wave's sorted list of its k best (glb_topk.hpp).  The four lists meet in LDS: an
//                       entry's rank is the number of entries above it, ranks below k are written.  Thread 0 folds the four
//                       waves' sums in wave order.
//   beam_select_kernel  one wave per group of B beams: the at most B * k <= 4096 candidates (score + logp of every live beam's
//                       candidates, a finished beam's own score) are one chunk of the same core, the list's first B entries
//                       are the group's next beams.
// A row's (a group's) outputs depend on that row (group) alone: which wave holds which chunk and the order of every fold are
// fixed by the chunk index, and the list is a function of the keys offered.  Nothing waits on another workgroup.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/glb.h"
#include "glb_chunk.hpp"
#include "glb_common.hpp"
#include "glb_rowlse.hpp"
#include "glb_topk.hpp"

namespace {
using namespace glb;

constexpr int kWaves = 4;  // waves per row: part of the reduction tree, not a tuning knob (changing it changes bits)

struct TopkParams : RowsParams {
  int32_t k;
  int32_t *out_token;
  float *out_logp, *out_logp_masked, *out_lse, *out_logZ;
};

template <int DT, int MASK>
__global__ __launch_bounds__(64 * kWaves) void topk_rows_kernel(const TopkParams a) {
  constexpr int EPV = ElemTraits<DT>::EPV;
  __shared__ WaveSums acc[kWaves];
  __shared__ uint64_t lists[kWaves * 64];
  __shared__ double row_lse[2];
  __shared__ int row_has[2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, V = a.V, k = a.k;
  for (int64_t row = blockIdx.x; row < a.n_rows; row += gridDim.x) {  // (the same trip count for the whole workgroup)
    int mid;
    const bool mask_ok = row_mask_of<MASK>(a, row, mid);
    const char *xrow = row_ptr<DT>(a.x, row, a.ld);
    float My = kNegInf, Mz = kNegInf;
    double Wy = 0.0, Wz = 0.0;
    uint64_t L = 0;  // this lane's entry of the wave's list
    for (int c = wave; c < a.nch; c += kWaves) {
      const int e_base = c * kChunk;
      float y[64];
      chunk_scaled<DT>(xrow, e_base, V, lane, a.scale, y);
      // (not chunk_sums: its one-term form for bit masks costs this kernel scalar registers - profiles/r33)
      const float Ny = exp_n(wave_max(lane_max64(y)));
      float Nz = kNegInf;
      uint64_t Sy = 0, Sz = 0;
      if (Ny != kNegInf) Sy = wave_fix_sum(lane_sum64<EPV>(y, Ny));
      if constexpr (MASK == GLB_MASK_NONE) {
        Nz = Ny;
        Sz = Sy;
      } else {
        chunk_add_mask<DT, MASK>(y, mask_ok, a.mask, mid, a.mask_ld, e_base, V, lane);  // y becomes the keys y + m in place
        Nz = exp_n(wave_max(lane_max64(y)));
        if (Nz != kNegInf) Sz = wave_fix_sum(lane_sum64<EPV>(y, Nz));
      }
      fold_chunk(Ny, Sy, My, Wy);
      fold_chunk(Nz, Sz, Mz, Wz);
      select_chunk<EPV>(y, e_base, lane, k, L);
    }
    lists[wave * 64 + lane] = lane < k ? L : 0ull;
    if (lane == 0) acc[wave] = WaveSums{Wy, Wz, My, Mz};
    __syncthreads();
    if (threadIdx.x == 0) {
      float Ry, Rz;
      double Ty, Tz;
      fold_waves(acc, Ty, Ry, Tz, Rz);
      const double lse_y = lse_of(Ty, Ry), lse_z = lse_of(Tz, Rz);
      row_lse[0] = lse_y;
      row_lse[1] = lse_z;
      row_has[0] = Ty > 0.0;
      row_has[1] = Tz > 0.0;
      if (a.out_lse) a.out_lse[row] = (float)lse_y;
      if (a.out_logZ) a.out_logZ[row] = Tz > 0.0 ? (float)(lse_z - lse_y) : kNegInf;
    }
    // an entry's rank among the four lists: the number of entries above it (the entries differ: an index occurs once)
    const uint64_t e = lists[threadIdx.x];
    int rank = 0;
    for (int i = 0; i < 64 * kWaves; ++i) rank += lists[i] > e ? 1 : 0;
    const int found = __syncthreads_count(e != 0ull);  // (also: row_lse is written)
    const int64_t o = row * k;
    if (e != 0ull && rank < k) {
      const float key = entry_key(e);
      a.out_token[o + rank] = entry_index(e);
      if (a.out_logp) a.out_logp[o + rank] = row_has[0] ? (float)((double)key - row_lse[0]) : kNegInf;
      if (a.out_logp_masked) a.out_logp_masked[o + rank] = row_has[1] ? (float)((double)key - row_lse[1]) : kNegInf;
    }
    if ((int)threadIdx.x < k && (int)threadIdx.x >= found) {  // positions beyond the finite keys
      a.out_token[o + threadIdx.x] = -1;
      if (a.out_logp) a.out_logp[o + threadIdx.x] = kNegInf;
      if (a.out_logp_masked) a.out_logp_masked[o + threadIdx.x] = kNegInf;
    }
    __syncthreads();  // (the shared arrays are written again for the workgroup's next row)
  }
}

struct BeamParams {
  const float *score;
  const int32_t *alive, *cand_token;
  const float *cand_logp;
  int64_t n_groups;
  int32_t B, k;
  int32_t *out_parent, *out_token;
  float *out_score;
};

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < __builtin_huge_valf(); }  // (false for NaN)

__global__ __launch_bounds__(64) void beam_select_kernel(const BeamParams a) {
  const int lane = threadIdx.x, B = a.B, k = a.k, n_cand = B * k;
  for (int64_t g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
    const int64_t b0 = g * B;
    float z[64];
#pragma unroll
    for (int j = 0; j < 64; ++j) {  // candidate s = b * k + jj on lane s % 64, element s / 64
      const int s = j * 64 + lane;
      float v = kNegInf;
      if (s < n_cand) {
        const int b = s / k, jj = s - b * k;
        const float sc = a.score[b0 + b];
        if (finite_f(sc)) {
          if (a.alive[b0 + b] != 0) {
            const float w = sc + a.cand_logp[b0 * k + s];
            if (a.cand_token[b0 * k + s] >= 0 && finite_f(w)) v = w;
          } else if (jj == 0) {
            v = sc;  // a finished hypothesis: one candidate, its own score
          }
        }
      }
      z[j] = v;
    }
    uint64_t L = 0;
    select_chunk<1>(z, 0, lane, B, L);
    if (lane < B) {
      int parent = -1, token = -1;
      float sc = kNegInf;
      if (L != 0ull) {
        const int s = entry_index(L);
        parent = s / k;
        token = a.alive[b0 + parent] != 0 ? a.cand_token[b0 * k + s] : -1;
        sc = entry_key(L);
      }
      a.out_parent[b0 + lane] = parent;
      a.out_token[b0 + lane] = token;
      a.out_score[b0 + lane] = sc;
    }
  }
}

}  // namespace

extern "C" {

int glb_topk_rows(const glb_topk_args *a, void *stream) {
  const char *const what = "glb_topk_rows";
  if (const int rc = glb::block_ok(a, what, "glb_topk_args")) return rc;
  if (!a->logits) return api_fail(GLB_EINVAL, "%s: logits is null", what);
  if (!a->out_token) return api_fail(GLB_EINVAL, "%s: out_token is null", what);
  if (a->k < 1 || a->k > kTopkMax) return api_fail(GLB_EINVAL, "%s: k %d outside 1..%d", what, a->k, kTopkMax);
  const RowsView v = rows_view(a);
  if (const int rc = rows_args_ok(what, v)) return rc;

  const TopkParams p{rows_params(v), a->k, a->out_token, a->out_logp, a->out_logp_masked, a->out_lse, a->out_logZ};
  launch_rows(v, [&](auto dt, auto mk) {
    hipLaunchKernelGGL((topk_rows_kernel<decltype(dt)::value, decltype(mk)::value>), rows_grid(p.n_rows), dim3(64 * kWaves), 0,
                       (hipStream_t)stream, p);
  });
  return glb::launched(what);
}

int glb_beam_select(const float *score, const int32_t *alive, const int32_t *cand_token, const float *cand_logp, int64_t n_groups,
                    int32_t width, int32_t k, int32_t *out_parent, int32_t *out_token, float *out_score, void *stream) {
  const char *const what = "glb_beam_select";
  if (!score || !alive || !cand_token || !cand_logp) return api_fail(GLB_EINVAL, "%s: null score, alive, cand_token or cand_logp", what);
  if (!out_parent || !out_token || !out_score) return api_fail(GLB_EINVAL, "%s: null out_parent, out_token or out_score", what);
  if (width < 1 || width > kTopkMax) return api_fail(GLB_EINVAL, "%s: width %d outside 1..%d", what, width, kTopkMax);
  if (k < 1 || k > kTopkMax) return api_fail(GLB_EINVAL, "%s: k %d outside 1..%d", what, k, kTopkMax);
  if (n_groups <= 0 || n_groups > (0x7fffffffll >> 12))
    return api_fail(GLB_EINVAL, "%s: n_groups=%lld must be positive and below 2^19", what, (long long)n_groups);
  BeamParams p{score, alive, cand_token, cand_logp, n_groups, width, k, out_parent, out_token, out_score};
  hipLaunchKernelGGL(beam_select_kernel, dim3((unsigned)n_groups), dim3(64), 0, (hipStream_t)stream, p);
  return glb::launched(what);
}

}  // extern "C"
