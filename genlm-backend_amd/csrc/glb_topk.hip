// glb_topk.hip - the k most probable tokens of every logits row, and a beam step's selection (include/glb.h: glb_topk_rows,
// glb_beam_select).
//
// Per logits row, with y = fl32(x * scale), m its mask row and key = fl32(y + m):
//   topk_rows_kernel    one workgroup of four waves per row, glb_score.hip's geometry: wave w takes the row's 4096-token
//                       chunks w, w + 4, ... in order - the chunk in 16-byte loads with its mask words or floats, for y and
//                       y + m the chunk's binary scale and integer sum (glb_rowlse.hpp) folded into the wave's running
//                       (scale, double sum), and the chunk's keys offered to the wave's sorted list of its k best
//                       (glb_topk.hpp).  The four lists meet in LDS: an entry's rank is the number of entries above it, ranks
//                       below k are written.  Thread 0 folds the four waves' sums in wave order.
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

struct TopkParams {
  const void *x;
  int64_t ld;
  int32_t V, nch;
  float scale;
  int64_t n_rows;
  int32_t n_masks, k;
  const int32_t *row_mask;  // [n_rows], null = (n_masks == 1 ? 0 : identity)
  const void *mask;
  int64_t mask_ld;
  int32_t *out_token;
  float *out_logp, *out_logp_masked, *out_lse, *out_logZ;
};

struct alignas(16) WaveAcc {  // what one wave hands to the row's last fold
  double Wy, Wz;              // sums of the wave's chunks on the scales My, Mz
  float My, Mz;
};

// a chunk's (scale, integer sum) into a running (scale, double sum); chunk order is the caller's (glb_score.hip's fold)
__device__ __forceinline__ void fold_chunk(float N, uint64_t S, float &M, double &W) {
  if (S == 0) return;
  if (N > M) {
    W = W > 0.0 ? ldexp(W, (int)fmaxf(M - N, -4000.0f)) : 0.0;
    M = N;
  }
  W += rec_mass(S, N, M);
}

template <int DT, int MASK>
__global__ __launch_bounds__(64 * kWaves) void topk_rows_kernel(const TopkParams a) {
  constexpr int EPV = ElemTraits<DT>::EPV;
  __shared__ WaveAcc acc[kWaves];
  __shared__ uint64_t lists[kWaves * 64];
  __shared__ double row_lse[2];
  __shared__ int row_has[2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, V = a.V, k = a.k;
  for (int64_t row = blockIdx.x; row < a.n_rows; row += gridDim.x) {  // (the same trip count for the whole workgroup)
    int mid = 0;
    bool mask_ok = true;
    if constexpr (MASK != GLB_MASK_NONE) {
      mid = __builtin_amdgcn_readfirstlane(a.row_mask ? a.row_mask[row] : (a.n_masks == 1 ? 0 : (int)row));
      mask_ok = mid >= 0 && mid < a.n_masks;  // out of range: a row whose mask allows nothing
    }
    const char *xrow = row_ptr<DT>(a.x, row, a.ld);
    float My = kNegInf, Mz = kNegInf;
    double Wy = 0.0, Wz = 0.0;
    uint64_t L = 0;  // this lane's entry of the wave's list
    for (int c = wave; c < a.nch; c += kWaves) {
      const int e_base = c * kChunk;
      float y[64];
      chunk_scaled<DT>(xrow, e_base, V, lane, a.scale, y);
      const float Ny = exp_n(wave_max(lane_max64(y)));
      float Nz = kNegInf;
      uint64_t Sy = 0, Sz = 0;
      if (Ny != kNegInf) Sy = wave_fix_sum(lane_sum64<EPV>(y, Ny));
      if constexpr (MASK == GLB_MASK_NONE) {
        Nz = Ny;
        Sz = Sy;
      } else {
        chunk_add_mask<DT, MASK>(y, mask_ok, a.mask, mid, a.mask_ld, e_base, V, lane);  // y becomes the keys y + m in place
        Nz =exp_n(wave_max(lane_max64(y)));
        if (Nz != kNegInf) Sz = wave_fix_sum(lane_sum64<EPV>(y, Nz));
      }
      fold_chunk(Ny, Sy, My, Wy);
      fold_chunk(Nz, Sz, Mz, Wz);
      select_chunk<EPV>(y, e_base, lane, k, L);
    }
    lists[wave * 64 + lane] = lane < k ? L : 0ull;
    if (lane == 0) acc[wave] = WaveAcc{Wy, Wz, My, Mz};
    __syncthreads();
    if (threadIdx.x == 0) {
      float Ry = kNegInf, Rz = kNegInf;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        Ry = fmaxf(Ry, acc[w].Wy > 0.0 ? acc[w].My : kNegInf);
        Rz = fmaxf(Rz, acc[w].Wz > 0.0 ? acc[w].Mz : kNegInf);
      }
      double Ty = 0.0, Tz = 0.0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {  // wave order
        if (acc[w].Wy > 0.0) Ty += ldexp(acc[w].Wy, (int)fmaxf(acc[w].My - Ry, -4000.0f));
        if (acc[w].Wz > 0.0) Tz += ldexp(acc[w].Wz, (int)fmaxf(acc[w].Mz - Rz, -4000.0f));
      }
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

template <int DT>
void launch_rows(int mask_kind, const TopkParams &p, hipStream_t s) {
  const dim3 grid((unsigned)(p.n_rows < (1 << 20) ? p.n_rows : (1 << 20))), block(64 * kWaves);
  switch (mask_kind) {
    case GLB_MASK_NONE: hipLaunchKernelGGL((topk_rows_kernel<DT, GLB_MASK_NONE>), grid, block, 0, s, p); break;
    case GLB_MASK_BITS: hipLaunchKernelGGL((topk_rows_kernel<DT, GLB_MASK_BITS>), grid, block, 0, s, p); break;
    default: hipLaunchKernelGGL((topk_rows_kernel<DT, GLB_MASK_F32>), grid, block, 0, s, p); break;
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

  TopkParams p{};
  p.x = a->logits;
  p.ld = a->ld;
  p.V = (int32_t)a->vocab;
  p.nch = (int32_t)((a->vocab + kChunk - 1) / kChunk);
  p.scale = a->logit_scale;
  p.n_rows = a->n_rows;
  p.n_masks = (int32_t)a->n_masks;
  p.k = a->k;
  p.row_mask = a->mask_kind == GLB_MASK_NONE ? nullptr : a->row_mask_id;
  p.mask = a->mask;
  p.mask_ld = a->mask_ld;
  p.out_token = a->out_token;
  p.out_logp = a->out_logp;
  p.out_logp_masked = a->out_logp_masked;
  p.out_lse = a->out_lse;
  p.out_logZ = a->out_logZ;
  hipStream_t s = (hipStream_t)stream;
  switch (a->dtype) {
    case GLB_F32: launch_rows<kDtF32>(a->mask_kind, p, s); break;
    case GLB_BF16: launch_rows<kDtBf16>(a->mask_kind, p, s); break;
    default: launch_rows<kDtF16>(a->mask_kind, p, s); break;
  }
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
