// glb_dfa_push.hip — weight pushing (include/glb.h: glb_dfa_backward / glb_dfa_push_weights): Jacobi sweeps for
// the backward weights, a wave per state, the stop rule decided on the device; then the automaton reweighted by them, elementwise.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/glb.h"
#include "glb_common.hpp"

namespace {

enum { P_SWEEPS = 0, P_CONVERGED = 1, P_FLAGS = 2, P_CALL = 3, P_MARK = 4 };  // glb_dfa_push_args.status; marks: P_MARK + {0, 1, 2}
constexpr int PUSH_THREADS = 256;      // four waves, a state each; push_weights: the 256 arcs of one state
constexpr int PUSH_MAX_SWEEPS = 65536; // launches one call may enqueue

__global__ void dfa_backward_init_kernel(int32_t n_states, const float *final_logw, float *beta, int32_t *status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_states) beta[i] = final_logw[i];
  if (i < GLB_DFA_PUSH_STATUS) status[i] = 0;
}

// the wave's 64 values combined by one fixed butterfly: every lane ends with the same bits
template <bool MAX>
__device__ inline float wave_combine(float x) {
  for (int d = 32; d >= 1; d >>= 1) {
    const float y = __shfl_xor(x, d);
    x = MAX ? fmaxf(x, y) : x + y;
  }
  return x;
}

// Sweep j of a call: beta_{k+1} (dst) from beta_k (src), a wave per state.  Whether the iteration still runs is read from a
// word no workgroup of this launch writes: the converged word (j = 0), else the mark of sweep j - 1; the marks rotate over
// three words - this launch sets word j % 3 (plain stores of 1) and clears word (j + 1) % 3 for the next
template <int SEMIRING>
__global__ __launch_bounds__(PUSH_THREADS) void dfa_backward_kernel(int32_t n_states, const int32_t *delta, const float *arc_logw,
                                                                   const float *final_logw, const float *src, float *dst,
                                                                   int32_t *status, int32_t j, float tol) {
  const bool go = j == 0 ? status[P_CONVERGED] == 0 : status[P_MARK + (j - 1) % 3] != 0;  // (uniform over the grid)
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    status[P_MARK + (j + 1) % 3] = 0;
    if (go) {
      status[P_SWEEPS] += 1;
      status[P_CALL] = j + 1;
    } else if (j == 0) {
      status[P_CALL] = 0;
    }
  }
  if (!go) return;
  const int lane = (int)threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * (PUSH_THREADS / 64) + (threadIdx.x >> 6);
  if (s >= n_states) return;  // (a whole wave)
  const float ninf = -__builtin_inff();
  const int32_t *drow = delta + s * 256;
  const float *arow = arc_logw + s * 256;
  float t[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int32_t d = drow[lane + 64 * k];
    const float a = arow[lane + 64 * k];
    t[k] = d >= 0 && d < n_states ? a + src[d] : ninf;
  }
  const float fin = final_logw[s], old = src[s];
  const float m = fmaxf(wave_combine<true>(fmaxf(fmaxf(t[0], t[1]), fmaxf(t[2], t[3]))), fin);
  float r = m;
  bool changed;
  if constexpr (SEMIRING == GLB_DFA_PUSH_LOG) {
    if (m > ninf) {  // (m = -inf: no term is finite, and (-inf) - (-inf) is never formed)
      const float sum = wave_combine<false>((expf(t[0] - m) + expf(t[1] - m)) + (expf(t[2] - m) + expf(t[3] - m)));
      r = m + logf(sum + expf(fin - m));
    }
    changed = !(r == old) && fabsf(r - old) > tol * fmaxf(1.0f, fabsf(r));
  } else {
    changed = r != old;
  }
  if (lane == 0) {
    dst[s] = r;
    if (changed) status[P_MARK + j % 3] = 1;
    if (!(r < __builtin_inff())) status[P_FLAGS] = 1;  // +inf or NaN
  }
}

// the call's last launch: the result into `beta` when the last sweep performed wrote `scratch`; thread 0 settles the words
__global__ void dfa_backward_end_kernel(int32_t n_states, float *beta, const float *scratch, int32_t *status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int32_t p = status[P_CALL];  // (no thread of this launch writes it)
  if ((p & 1) && i < n_states) beta[i] = scratch[i];
  if (i == 0) {
    if (p > 0) status[P_CONVERGED] = status[P_MARK + (p - 1) % 3] == 0;
    status[P_MARK] = status[P_MARK + 1] = status[P_MARK + 2] = 0;
  }
}

__global__ __launch_bounds__(PUSH_THREADS) void dfa_push_weights_kernel(int32_t n_states, const int32_t *delta, const float *arc_logw,
                                                                       const float *final_logw, const float *beta, float *arc_out,
                                                                       float *final_out) {
  const int64_t s = blockIdx.x;
  const int b = (int)threadIdx.x;
  const float ninf = -__builtin_inff();
  const float bs = beta[s];
  const int32_t d = delta[s * 256 + b];
  float w = ninf;
  if (bs > ninf && d >= 0 && d < n_states) w = (arc_logw[s * 256 + b] + beta[d]) - bs;
  arc_out[s * 256 + b] = w;
  if (b == 0) final_out[s] = bs > ninf ? final_logw[s] - bs : ninf;
}

// the block of glb_dfa_backward (`backward`) / glb_dfa_push_weights: the same checks, each call's own tables
int dfa_push_check(const glb_dfa_push_args *p, const char *what, bool backward) {
  if (const int rc = glb::block_ok(p, what, "glb_dfa_push_args")) return rc;
  if (p->n_states < 1 || p->n_states > 0x7fffff00) return glb::api_fail(GLB_EINVAL, "%s: n_states %d outside [1, 2^31 - 256]", what, p->n_states);
  if (p->start < 0 || p->start >= p->n_states)
    return glb::api_fail(GLB_EINVAL, "%s: start %d outside [0, %d)", what, p->start, p->n_states);
  if (p->semiring != GLB_DFA_PUSH_LOG && p->semiring != GLB_DFA_PUSH_MAX)
    return glb::api_fail(GLB_EINVAL, "%s: semiring %d is neither GLB_DFA_PUSH_LOG nor GLB_DFA_PUSH_MAX", what, p->semiring);
  if (p->sweeps < 1 || p->sweeps > PUSH_MAX_SWEEPS)
    return glb::api_fail(GLB_EINVAL, "%s: sweeps %d outside [1, %d]", what, p->sweeps, PUSH_MAX_SWEEPS);
  if (!(p->tol >= 0.0f)) return glb::api_fail(GLB_EINVAL, "%s: tol %g is negative or NaN", what, (double)p->tol);
  if (!p->delta) return glb::api_fail(GLB_EINVAL, "%s: delta is null", what);
  if (!p->arc_logw) return glb::api_fail(GLB_EINVAL, "%s: arc_logw is null", what);
  if (!p->final_logw) return glb::api_fail(GLB_EINVAL, "%s: final_logw is null", what);
  if (!p->beta) return glb::api_fail(GLB_EINVAL, "%s: beta is null", what);
  if (backward) {
    if (!p->scratch) return glb::api_fail(GLB_EINVAL, "%s: scratch is null", what);
    if (!p->status) return glb::api_fail(GLB_EINVAL, "%s: status is null", what);
  } else {
    if (!p->arc_out) return glb::api_fail(GLB_EINVAL, "%s: arc_out is null", what);
    if (!p->final_out) return glb::api_fail(GLB_EINVAL, "%s: final_out is null", what);
  }
  return GLB_OK;
}

template <int SEMIRING>
void backward_sweeps(const glb_dfa_push_args *p, hipStream_t st) {
  const unsigned grid = blocks_for(p->n_states, PUSH_THREADS / 64);
  for (int32_t j = 0; j < p->sweeps; ++j)
    hipLaunchKernelGGL(dfa_backward_kernel<SEMIRING>, dim3(grid), dim3(PUSH_THREADS), 0, st, p->n_states, p->delta, p->arc_logw,
                       p->final_logw, j & 1 ? p->scratch : p->beta, j & 1 ? p->beta : p->scratch, p->status, j, p->tol);
}

}  // namespace

extern "C" {

int glb_dfa_backward(const glb_dfa_push_args *p, void *stream) {
  if (const int rc = dfa_push_check(p, "glb_dfa_backward", true)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  const int64_t items = p->n_states > GLB_DFA_PUSH_STATUS ? p->n_states : GLB_DFA_PUSH_STATUS;
  if (p->restart)
    hipLaunchKernelGGL(dfa_backward_init_kernel, dim3(blocks_for(items, 256)), dim3(256), 0, st, p->n_states, p->final_logw, p->beta,
                       p->status);
  if (p->semiring == GLB_DFA_PUSH_MAX) backward_sweeps<GLB_DFA_PUSH_MAX>(p, st);
  else backward_sweeps<GLB_DFA_PUSH_LOG>(p, st);
  hipLaunchKernelGGL(dfa_backward_end_kernel, dim3(blocks_for(p->n_states, 256)), dim3(256), 0, st, p->n_states, p->beta, p->scratch,
                     p->status);
  return glb::launched("dfa_backward launch");
}

int glb_dfa_push_weights(const glb_dfa_push_args *p, void *stream) {
  if (const int rc = dfa_push_check(p, "glb_dfa_push_weights", false)) return rc;
  hipLaunchKernelGGL(dfa_push_weights_kernel, dim3((unsigned)p->n_states), dim3(PUSH_THREADS), 0, (hipStream_t)stream, p->n_states,
                     p->delta, p->arc_logw, p->final_logw, p->beta, p->arc_out, p->final_out);
  return glb::launched("dfa_push_weights launch");
}

}  // extern "C"
