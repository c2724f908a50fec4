// glb_packed_plan.hip - the plan of a row-packed encoding (include/glb.h: glb_packed_plan; kv.encode_packed)
// in two plain launches instead of two dozen index ops:
//   packed_plan_scan_kernel  one workgroup: the tails t_u = lengths[sel[u]] - P_grp[u] of the U contexts, their inclusive
//                            int32 sums `ends` (strides of the workgroup with a carry), the contexts' segments and last rows,
//                            and the G prompts' segments copied in front;
//   packed_plan_rows_kernel  one thread per row of M: a prompt row copies its token and position, a tail row finds its
//                            context by binary search in `ends` and gathers its token.
// Every value is what the torch ops of encode_packed(native_plan=False) give, for every input: int32 arithmetic wraps as
// theirs does (computed unsigned here), `ends` of hostile lengths need not be sorted and the search is torch.searchsorted's
// own (right = True: lo = 0, hi = U; mid = lo + (hi - lo) / 2; ends[mid] > r ? hi = mid : lo = mid + 1), and every index is
// clamped where that code clamps.  No workgroup waits on another, nothing is allocated or read back.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/glb.h"
#include "glb_common.hpp"

namespace {

constexpr int SCAN_THREADS = 1024, ROW_THREADS = 256;

__device__ __forceinline__ int32_t wrap_add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
__device__ __forceinline__ int32_t wrap_sub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }

// an index into `lengths` / `starts` as torch's indexing reads it (negative: from the end), kept inside [0, n)
__device__ __forceinline__ int64_t ctx_index(int32_t s, int64_t n) {
  int64_t i = s < 0 ? (int64_t)s + n : (int64_t)s;
  return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

__global__ __launch_bounds__(SCAN_THREADS) void packed_plan_scan_kernel(glb_packed_plan_args a) {
  __shared__ int32_t wave_sum[SCAN_THREADS / 64];
  __shared__ int32_t carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t G = a.n_groups, U = a.n_sel;
  for (int64_t i = tid; i < G * 4; i += SCAN_THREADS) a.segments[i] = a.group_segments[i];
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int64_t base = 0; base < U; base += SCAN_THREADS) {
    const int64_t u = base + tid;
    int32_t pre_len = 0, pre_start = 0, tail = 0;
    if (u < U) {
      int64_t g = a.grp[u];
      g = g < 0 ? 0 : (g > G - 1 ? G - 1 : g);
      pre_len = a.group_lens[g];
      pre_start = a.group_starts[g];
      tail = wrap_sub(a.lengths[ctx_index(a.sel[u], a.n_contexts)], pre_len);
    }
    // inclusive scan of the stride: within the wave, then over the waves' sums, on top of the strides before
    int32_t x = tail;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int32_t y = __shfl_up(x, d, 64);
      if (lane >= d) x = wrap_add(x, y);
    }
    if (lane == 63) wave_sum[wave] = x;
    __syncthreads();
    int32_t before = carry_s;
    for (int w = 0; w < wave; ++w) before = wrap_add(before, wave_sum[w]);
    const int32_t end = wrap_add(before, x);
    if (u < U) {
      const int32_t tail_start = wrap_sub(wrap_add((int32_t)a.n_pre, end), tail);
      a.ends[u] = end;
      int32_t *seg = a.segments + (G + u) * 4;
      seg[0] = pre_start;
      seg[1] = pre_len;
      seg[2] = tail_start;
      seg[3] = tail;
      const int64_t last = (int64_t)wrap_sub(wrap_add(tail_start, tail), 1), m = a.n_pre + a.n_tail_rows;
      a.last[u] = last < 0 ? 0 : (last > m - 1 ? m - 1 : last);
    }
    __syncthreads();  // (every wave has read carry_s and the sums)
    if (tid == SCAN_THREADS - 1) carry_s = end;  // (threads past U carry a zero tail: the stride's total)
    __syncthreads();
  }
}

__global__ __launch_bounds__(ROW_THREADS) void packed_plan_rows_kernel(glb_packed_plan_args a) {
  const int64_t row = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x;
  if (row >= a.n_pre + a.n_tail_rows) return;
  if (row < a.n_pre) {
    a.ids[row] = a.group_ids[row];
    a.pos[row] = a.group_pos[row];
    return;
  }
  const int64_t U = a.n_sel;
  const int32_t r = (int32_t)(row - a.n_pre);
  int64_t lo = 0, hi = U;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (a.ends[mid] > r) hi = mid; else lo = mid + 1;
  }
  const int64_t u = lo > U - 1 ? U - 1 : lo;
  const int32_t *seg = a.segments + (a.n_groups + u) * 4;  // (written by the scan kernel: pre_len, tail)
  const int32_t pos_t = wrap_add(seg[1], wrap_sub(r, wrap_sub(a.ends[u], seg[3])));
  int64_t at = a.starts[ctx_index(a.sel[u], a.n_contexts)] + (int64_t)pos_t;
  at = at < 0 ? 0 : (at > a.n_tokens - 1 ? a.n_tokens - 1 : at);
  a.ids[row] = (int64_t)a.tokens[at];
  const int64_t p = pos_t;
  a.pos[row] = p < 0 ? 0 : (p > a.pos_cap - 1 ? a.pos_cap - 1 : p);
}

}  // namespace

extern "C" int glb_packed_plan(const glb_packed_plan_args *args, void *stream) {
  if (!args) return glb::api_fail(GLB_EINVAL, "glb_packed_plan: null argument block");
  if (args->struct_size != sizeof(glb_packed_plan_args))
    return glb::api_fail(GLB_EINVAL, "glb_packed_plan_args.struct_size %u != %zu (ABI mismatch)", args->struct_size,
                         sizeof(glb_packed_plan_args));
  const glb_packed_plan_args &a = *args;
  if (a.n_groups < 1 || a.n_sel < 1 || a.n_pre < 1 || a.n_tail_rows < a.n_sel || a.n_contexts < 1 || a.n_tokens < 1 ||
      a.pos_cap < 1 || a.n_sel > INT32_MAX || a.n_pre + a.n_tail_rows > INT32_MAX)
    return glb::api_fail(GLB_EINVAL, "glb_packed_plan: bad sizes (G %lld, U %lld, prompt rows %lld, tail rows %lld, contexts %lld, "
                         "tokens %lld, position cap %lld)", (long long)a.n_groups, (long long)a.n_sel, (long long)a.n_pre,
                         (long long)a.n_tail_rows, (long long)a.n_contexts, (long long)a.n_tokens, (long long)a.pos_cap);
  if (!a.tokens || !a.starts || !a.lengths || !a.sel || !a.grp || !a.group_starts || !a.group_lens || !a.group_segments ||
      !a.group_ids || !a.group_pos)
    return glb::api_fail(GLB_EINVAL, "glb_packed_plan: null input");
  if (!a.segments || !a.ids || !a.pos || !a.last || !a.ends) return glb::api_fail(GLB_EINVAL, "glb_packed_plan: null output");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(packed_plan_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return glb::api_hip_fail(e, "glb_packed_plan scan launch");
  hipLaunchKernelGGL(packed_plan_rows_kernel, dim3(blocks_for(a.n_pre + a.n_tail_rows, ROW_THREADS)), dim3(ROW_THREADS), 0, s, a);
  e = hipGetLastError();
  if (e != hipSuccess) return glb::api_hip_fail(e, "glb_packed_plan rows launch");
  return GLB_OK;
}
