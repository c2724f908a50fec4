// glb_dfa_min.hip — byte automata minimised on the device (include/glb.h: glb_dfa_refine / glb_dfa_quotient).
// Moore's refinement: a round gives every kept state the smallest state that shares its signature - its own class, the class
// behind each of its 256 arcs (-1 where the arc is absent) and, with weights, the arcs' bit patterns.  A wave per state, lane l
// the bytes l, l + 64, l + 128, l + 192 as in glb_dfa_backward; the signatures meet in an open-addressing table keyed by a
// 64-bit hash, and every state checks its signature element by element against the member the table elected.  The stop rule
// is the device's: a round that leaves the number of classes as it was has changed nothing.  Then the quotient, elementwise.
// Everything read from device memory is range-checked.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/glb.h"
#include "glb_block.hpp"  // (mix64)
#include "glb_common.hpp"

namespace {

enum { M_ROUNDS = 0, M_CONVERGED = 1, M_FLAGS = 2, M_CLASSES = 3, M_COUNT = 4, M_CALL = 7 };  // status; counts: M_COUNT + {0, 1, 2}
enum { F_COLLISION = 1, F_TABLE = 2 };
constexpr int MIN_THREADS = 256;       // four waves, a state each; the quotient: the 256 arcs of one state
constexpr int MIN_MAX_ROUNDS = 65536;  // rounds one call may enqueue
constexpr int32_t NO_MEMBER = 0x7fffffff;

struct Min {
  const int32_t *delta;
  const uint8_t *keep;
  const uint32_t *final_bits, *arc_bits;
  int32_t n_states;
  unsigned long long *keys;  // [slots]; 0: empty
  int32_t *members;          // [slots]; the smallest state that brought the key
  uint64_t mask;             // slots - 1
  int32_t *status;
};

// The lane's share of state s's signature under the classes `src`: succ[k] the class behind byte lane + 64 k (-1: the arc is
// absent - delta has none, its destination lies outside [0, n_states) or is not kept), w[k] the arc's bits (0 where absent
// or without arc_bits)
__device__ inline void lane_signature(const Min &m, const int32_t *src, int64_t s, int lane, int32_t succ[4], uint32_t w[4]) {
  const int32_t *drow = m.delta + s * 256;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int32_t d = drow[lane + 64 * k];
    const bool present = d >= 0 && d < m.n_states && m.keep[d];
    succ[k] = present ? src[d] : -1;
    w[k] = present && m.arc_bits ? m.arc_bits[s * 256 + lane + 64 * k] : 0u;
  }
}

// The 64-bit hash of a signature: every (byte, class, bits) element and the state's own class mixed on its own, the 257
// values summed modulo 2^64 - a sum of integers, so the butterfly's order does not matter and every lane ends with the same
// bits.  0 is the table's empty key and never returned.  INIT: the signature is the final label alone
template <bool INIT>
__device__ inline uint64_t wave_hash(const Min &m, int32_t own, const int32_t succ[4], const uint32_t w[4], int lane) {
  uint64_t h = 0;
  if constexpr (INIT) {
    h = mix64(0x9e3779b97f4a7c15ull ^ (uint32_t)own);  // (own: the final label)
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      h += mix64((((uint64_t)(uint32_t)succ[k] << 32) | w[k]) ^ ((uint64_t)(lane + 64 * k + 1) * 0x9e3779b97f4a7c15ull));
    for (int d = 32; d >= 1; d >>= 1) h += (uint64_t)__shfl_xor((unsigned long long)h, d);
    h += mix64(0xd1b54a32d192ed03ull ^ (uint32_t)own);
  }
  return h ? h : 1;
}

// whether round j of a call runs, from words that no launch of round j writes: the converged word (j = 0), else whether
// round j - 1 changed the number of classes.  A round that does not run hands its predecessor's count on (min_assign_kernel), so
// every later round of the call finds no change either
__device__ inline bool round_goes(const int32_t *status, int32_t j) {
  if (j == 0) return status[M_CONVERGED] == 0;
  const int32_t before = j == 1 ? status[M_CLASSES] : status[M_COUNT + (j - 2) % 3];
  return status[M_COUNT + (j - 1) % 3] != before;
}

// the table emptied for round j (j < 0: for the initial classes, and status zeroed)
__global__ void min_clear_kernel(Min m, int32_t j) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < 0) {
    if (i < GLB_DFA_MIN_STATUS) m.status[i] = 0;
  } else if (!round_goes(m.status, j)) {
    return;
  }
  if (i <= m.mask) {
    m.keys[i] = 0;
    m.members[i] = NO_MEMBER;
  }
}

// Every kept state's hash into the table: lane 0 claims the first slot from the hash's own that is empty or holds the same
// key (a 64-bit compare-and-swap) and lowers the slot's member to its state (an atomic minimum).  Whatever order the atomics
// take, the launch ends with the same set of keys, each with the smallest of its states: a key may land in another slot, but
// a slot is never emptied while keys arrive, so the probe of min_assign_kernel finds it wherever it lies
template <bool INIT>
__global__ __launch_bounds__(MIN_THREADS) void min_insert_kernel(Min m, const int32_t *src, int32_t j) {
  if constexpr (!INIT) {
    const bool go = round_goes(m.status, j);  // (uniform over the grid)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      m.status[M_COUNT + j % 3] = 0;
      if (go) {
        m.status[M_ROUNDS] += 1;
        m.status[M_CALL] = j + 1;
      } else if (j == 0) {
        m.status[M_CALL] = 0;
      }
    }
    if (!go) return;
  }
  const int lane = (int)threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * (MIN_THREADS / 64) + (threadIdx.x >> 6);
  if (s >= m.n_states || !m.keep[s]) return;  // (a whole wave)
  int32_t succ[4] = {-1, -1, -1, -1};
  uint32_t w[4] = {0, 0, 0, 0};
  int32_t own;
  if constexpr (INIT) {
    own = (int32_t)m.final_bits[s];
  } else {
    own = src[s];
    lane_signature(m, src, s, lane, succ, w);
  }
  const uint64_t h = wave_hash<INIT>(m, own, succ, w, lane);
  if (lane != 0) return;
  uint64_t slot = h & m.mask;
  for (uint64_t probe = 0; probe <= m.mask; ++probe, slot = (slot + 1) & m.mask) {
    const unsigned long long old = atomicCAS(&m.keys[slot], 0ull, (unsigned long long)h);
    if (old == 0ull || old == h) {
      atomicMin(&m.members[slot], (int32_t)s);
      return;
    }
  }
  atomicOr(&m.status[M_FLAGS], F_TABLE);  // (a table of fewer slots than kept states: refused on the host side of the call)
}

// Every state's new class: the member its hash's slot elected, after the state's signature has been compared with that
// member's element by element - a difference is a hash collision: the sticky flag is set and the state stays alone, never
// merged.  States that are their own class's smallest member are counted into the round's word.  dst[s] = -1 where !keep[s]
template <bool INIT>
__global__ __launch_bounds__(MIN_THREADS) void min_assign_kernel(Min m, const int32_t *src, int32_t *dst, int32_t j) {
  int32_t *count = &m.status[INIT ? M_CLASSES : M_COUNT + j % 3];
  if constexpr (!INIT) {
    if (!round_goes(m.status, j)) {
      if (blockIdx.x == 0 && threadIdx.x == 0) *count = j == 0 ? m.status[M_CLASSES] : m.status[M_COUNT + (j - 1) % 3];
      return;
    }
  }
  const int lane = (int)threadIdx.x & 63;
  const int64_t s = (int64_t)blockIdx.x * (MIN_THREADS / 64) + (threadIdx.x >> 6);
  if (s >= m.n_states) return;  // (a whole wave)
  if (!m.keep[s]) {
    if (lane == 0) dst[s] = -1;
    return;
  }
  int32_t succ[4] = {-1, -1, -1, -1};
  uint32_t w[4] = {0, 0, 0, 0};
  int32_t own;
  if constexpr (INIT) {
    own = (int32_t)m.final_bits[s];
  } else {
    own = src[s];
    lane_signature(m, src, s, lane, succ, w);
  }
  const uint64_t h = wave_hash<INIT>(m, own, succ, w, lane);
  int32_t member = -1;  // (every lane walks the same slots: h is the wave's)
  uint64_t slot = h & m.mask;
  for (uint64_t probe = 0; probe <= m.mask; ++probe, slot = (slot + 1) & m.mask) {
    const unsigned long long key = m.keys[slot];
    if (key == h) member = m.members[slot];
    if (key == h || key == 0ull) break;
  }
  int32_t flags = 0;
  if (member < 0 || member > s || !m.keep[member]) {  // the key is not there, or its member is no state that could have brought it
    flags = F_TABLE;
    member = (int32_t)s;
  } else if (member != s) {
    bool same;
    if constexpr (INIT) {
      same = (int32_t)m.final_bits[member] == own;
    } else {
      int32_t msucc[4];
      uint32_t mw[4];
      lane_signature(m, src, member, lane, msucc, mw);
      same = src[member] == own;
#pragma unroll
      for (int k = 0; k < 4; ++k) same = same && msucc[k] == succ[k] && mw[k] == w[k];
    }
    if (!__all(same)) {
      flags = F_COLLISION;
      member = (int32_t)s;
    }
  }
  if (lane == 0) {
    dst[s] = member;
    if (member == s) atomicAdd(count, 1);
    if (flags) atomicOr(&m.status[M_FLAGS], flags);
  }
}

// the call's last launch: the result into `cls` when the last round performed wrote `scratch`; thread 0 settles the words
__global__ void min_end_kernel(int32_t n_states, int32_t *cls, const int32_t *scratch, int32_t *status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int32_t p = status[M_CALL];  // (no thread of this launch writes it)
  if ((p & 1) && i < n_states) cls[i] = scratch[i];
  if (i == 0) {
    if (p > 0) {
      const int32_t before = p == 1 ? status[M_CLASSES] : status[M_COUNT + (p - 2) % 3];
      const int32_t now = status[M_COUNT + (p - 1) % 3];
      status[M_CONVERGED] = now == before;
      status[M_CLASSES] = now;
    }
    status[M_COUNT] = status[M_COUNT + 1] = status[M_COUNT + 2] = 0;
  }
}

// quotient state j: the row of rep[j] relabelled through new_id, an arc kept where it is present and leads to a quotient state
__global__ __launch_bounds__(MIN_THREADS) void min_quotient_kernel(int32_t n_states, int32_t n_new, const int32_t *delta, const uint8_t *keep,
                                                                  const int32_t *new_id, const int32_t *rep, const float *arc_logw,
                                                                  const float *final_logw, const uint8_t *accepting, int32_t *delta_out,
                                                                  float *arc_out, float *final_out, uint8_t *accepting_out) {
  const int64_t j = blockIdx.x;
  const int b = (int)threadIdx.x;
  const float ninf = -__builtin_inff();
  const int32_t r = rep[j];
  const bool valid = r >= 0 && r < n_states;
  int32_t to = -1;
  if (valid) {
    const int32_t d = delta[(int64_t)r * 256 + b];
    if (d >= 0 && d < n_states && keep[d]) to = new_id[d];
    if (to < 0 || to >= n_new) to = -1;
  }
  delta_out[j * 256 + b] = to;
  if (arc_out) arc_out[j * 256 + b] = to >= 0 ? arc_logw[(int64_t)r * 256 + b] : ninf;
  if (b == 0) {
    if (final_out) final_out[j] = valid ? final_logw[r] : ninf;
    if (accepting_out) accepting_out[j] = valid ? accepting[r] : (uint8_t)0;
  }
}

// the block of glb_dfa_refine (`refine`) / glb_dfa_quotient: the same checks, each call's own tables
int dfa_min_check(const glb_dfa_min_args *p, const char *what, bool refine) {
  if (const int rc = glb::block_ok(p, what, "glb_dfa_min_args")) return rc;
  if (p->n_states < 1 || p->n_states > 0x7fffff00) return glb::api_fail(GLB_EINVAL, "%s: n_states %d outside [1, 2^31 - 256]", what, p->n_states);
  if (!p->delta) return glb::api_fail(GLB_EINVAL, "%s: delta is null", what);
  if (!p->keep) return glb::api_fail(GLB_EINVAL, "%s: keep is null", what);
  if (refine) {
    if (p->rounds < 1 || p->rounds > MIN_MAX_ROUNDS)
      return glb::api_fail(GLB_EINVAL, "%s: rounds %d outside [1, %d]", what, p->rounds, MIN_MAX_ROUNDS);
    if (p->table_slots < 2 * (int64_t)p->n_states || p->table_slots > ((int64_t)1 << 33) || (p->table_slots & (p->table_slots - 1)))
      return glb::api_fail(GLB_EINVAL, "%s: table_slots %lld is not a power of two in [2 n_states = %lld, 2^33]", what,
                           (long long)p->table_slots, 2 * (long long)p->n_states);
    if (!p->final_bits) return glb::api_fail(GLB_EINVAL, "%s: final_bits is null", what);
    if (!p->cls) return glb::api_fail(GLB_EINVAL, "%s: cls is null", what);
    if (!p->scratch) return glb::api_fail(GLB_EINVAL, "%s: scratch is null", what);
    if (!p->table) return glb::api_fail(GLB_EINVAL, "%s: table is null", what);
    if ((uintptr_t)p->table & 7) return glb::api_fail(GLB_EINVAL, "%s: table is not aligned to 8 bytes", what);
    if (!p->status) return glb::api_fail(GLB_EINVAL, "%s: status is null", what);
  } else {
    if (p->n_new < 1 || p->n_new > p->n_states)
      return glb::api_fail(GLB_EINVAL, "%s: n_new %d outside [1, n_states = %d]", what, p->n_new, p->n_states);
    if (!p->new_id) return glb::api_fail(GLB_EINVAL, "%s: new_id is null", what);
    if (!p->rep) return glb::api_fail(GLB_EINVAL, "%s: rep is null", what);
    if (!p->delta_out) return glb::api_fail(GLB_EINVAL, "%s: delta_out is null", what);
    if (p->arc_out && !p->arc_logw) return glb::api_fail(GLB_EINVAL, "%s: arc_logw is null beside arc_out", what);
    if (p->final_out && !p->final_logw) return glb::api_fail(GLB_EINVAL, "%s: final_logw is null beside final_out", what);
    if (p->accepting_out && !p->accepting) return glb::api_fail(GLB_EINVAL, "%s: accepting is null beside accepting_out", what);
  }
  return GLB_OK;
}

}  // namespace

extern "C" {

int glb_dfa_refine(const glb_dfa_min_args *p, void *stream) {
  if (const int rc = dfa_min_check(p, "glb_dfa_refine", true)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  const Min m{p->delta, p->keep, p->final_bits, p->arc_bits, p->n_states, (unsigned long long *)p->table,
              (int32_t *)((unsigned long long *)p->table + p->table_slots), (uint64_t)p->table_slots - 1, p->status};
  const dim3 waves(blocks_for(p->n_states, MIN_THREADS / 64)), slots(blocks_for(p->table_slots, 256)), block(MIN_THREADS);
  if (p->restart) {
    hipLaunchKernelGGL(min_clear_kernel, slots, dim3(256), 0, st, m, -1);
    hipLaunchKernelGGL(min_insert_kernel<true>, waves, block, 0, st, m, (const int32_t *)nullptr, 0);
    hipLaunchKernelGGL(min_assign_kernel<true>, waves, block, 0, st, m, (const int32_t *)nullptr, p->cls, 0);
  }
  for (int32_t j = 0; j < p->rounds; ++j) {
    const int32_t *src = j & 1 ? p->scratch : p->cls;
    int32_t *dst = j & 1 ? p->cls : p->scratch;
    hipLaunchKernelGGL(min_clear_kernel, slots, dim3(256), 0, st, m, j);
    hipLaunchKernelGGL(min_insert_kernel<false>, waves, block, 0, st, m, src, j);
    hipLaunchKernelGGL(min_assign_kernel<false>, waves, block, 0, st, m, src, dst, j);
  }
  hipLaunchKernelGGL(min_end_kernel, dim3(blocks_for(p->n_states, 256)), dim3(256), 0, st, p->n_states, p->cls, p->scratch, p->status);
  return glb::launched("dfa_refine launch");
}

int glb_dfa_quotient(const glb_dfa_min_args *p, void *stream) {
  if (const int rc = dfa_min_check(p, "glb_dfa_quotient", false)) return rc;
  hipLaunchKernelGGL(min_quotient_kernel, dim3((unsigned)p->n_new), dim3(MIN_THREADS), 0, (hipStream_t)stream, p->n_states, p->n_new,
                     p->delta, p->keep, p->new_id, p->rep, p->arc_logw, p->final_logw, p->accepting, p->delta_out, p->arc_out,
                     p->final_out, p->accepting_out);
  return glb::launched("dfa_quotient launch");
}

}  // extern "C"
