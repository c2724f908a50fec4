// glb_fsa_product.hip — the product of two byte automata on the device (include/glb.h: glb_fsa_product_round / glb_fsa_live;
// DESIGN.md §22).  A breadth-first search over the pairs of states: the queue search of glb_search.hpp with the whole of the
// queue a round (chunk = max_states), so a round expands the frontier - the states the round before numbered - a block per
// state, a thread per byte: a wave reads 64 consecutive entries of a delta row of either operand.  A target pair meets its
// equals in an open-addressing table keyed by the full 64-bit pair (no collisions to flag); a new pair's slot keeps the
// smallest arc index (frontier position * 256 + byte) that found it, and count, scan, number, resolve and advance - the
// shared kernels - hand out the ids: the numbering is the host queue search's, whatever order the atomics take.  This file
// keeps the table, the expansion and what a pair is.  Then liveness, swept in place to its fixed point.  Everything read
// from device memory is range-checked.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/glb.h"
#include "glb_common.hpp"
#include "glb_search.hpp"

namespace {

constexpr int FSA_THREADS = SEARCH_THREADS;  // the 256 bytes of one state; liveness: four waves, a state each

struct Prod {
  int32_t op, n_a, n_b;
  const int32_t *delta_a, *delta_b;
  const uint8_t *acc_a, *acc_b, *live_a, *live_b;
  const float *arc_a, *final_a, *arc_b, *final_b;
  int32_t max_states, chunk;  // (chunk = max_states: a round takes all of the queue)
  unsigned long long *keys;  // [slots]; 0: empty
  int32_t *arcmin;           // [slots]; the smallest arc index of the round that brought the key
  int32_t *ids;              // [slots]; -1 until the key's state is numbered
  uint64_t mask;             // slots - 1
  int32_t *pairs, *delta_out, *cnt;
  uint8_t *accepting_out;
  float *arc_out, *final_out;
  int32_t *status;

  // the winning arc's target becomes state `id`: the slot's id, and the pair read back from the key
  static __device__ bool number(const Prod &p, int64_t id, int32_t, int, int64_t slot) {
    const uint64_t key = p.keys[slot], nb = (uint64_t)p.n_b + 1;
    p.ids[slot] = (int32_t)id;
    p.pairs[2 * id] = (int32_t)(key / nb) - 1;
    p.pairs[2 * id + 1] = (int32_t)(key % nb) - 1;
    return true;
  }
  static __device__ int32_t id_of(const Prod &p, int64_t slot) { return p.ids[slot]; }
};

// a component that is not a live state of its automaton is out: -1
__device__ inline int32_t side(int32_t s, int32_t n, const uint8_t *live) { return s >= 0 && s < n && live[s] ? s : -1; }

// the key of a normalised pair, 0 where the pair does not exist under `op`
__device__ inline uint64_t pair_key(const Prod &p, int32_t a, int32_t b) {
  const bool exists = p.op == GLB_FSA_AND ? (a >= 0 && b >= 0) : p.op == GLB_FSA_SUB ? a >= 0 : (a >= 0 || b >= 0);
  return exists ? (uint64_t)(a + 1) * ((uint64_t)p.n_b + 1) + (uint64_t)(b + 1) : 0ull;
}

// the slot of `key`: the first from its hash's own that is empty or holds it, `fresh` where this call put the key there;
// -1 when the table is full, -2 when a flag went up while probing (looked at every 32 slots: nothing of the round counts then)
__device__ inline int64_t claim_slot(const Prod &p, uint64_t key, bool &fresh) {
  uint64_t slot = mix64(key) & p.mask;
  for (uint64_t probe = 0; probe <= p.mask; ++probe, slot = (slot + 1) & p.mask) {
    const unsigned long long old = atomicCAS(&p.keys[slot], 0ull, (unsigned long long)key);
    fresh = old == 0ull;
    if (fresh || old == key) return (int64_t)slot;
    if ((probe & 31) == 31 && flags_now(p.status)) return -2;
  }
  return -1;
}

// n more pairs entered; past max_states that is the overflow
__device__ inline void count_entered(const Prod &p, int32_t n) {
  const int64_t total = (int64_t)atomicAdd(&p.status[P_ENTERED], n) + n;
  if (total > p.max_states) overflow(p.status, total);
}

// accepting and the final weight of the pair (a, b), either side -1 when out
__device__ inline void pair_final(const Prod &p, int32_t a, int32_t b, bool &acc, float &fin) {
  const bool fa = a >= 0 && p.acc_a[a], fb = b >= 0 && p.acc_b[b];
  acc = p.op == GLB_FSA_AND ? (fa && fb) : p.op == GLB_FSA_SUB ? (fa && !fb) : (fa || fb);
  fin = -__builtin_inff();
  if (acc) {
    fin = 0.0f;
    if (p.final_a && p.final_b && p.op == GLB_FSA_AND) fin = p.final_a[a] + p.final_b[b];
    else if (p.final_a) fin = p.final_a[a];
    else if (p.final_b && p.op == GLB_FSA_AND) fin = p.final_b[b];
  }
}

// the table emptied and the status zeroed
__global__ void fsa_clear_kernel(Prod p) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < GLB_FSA_STATUS) p.status[i] = 0;
  if (i <= p.mask) {
    p.keys[i] = 0;
    p.arcmin[i] = NO_ARC;
    p.ids[i] = -1;
  }
}

// state 0: the start pair (a pair that does not exist is (-1, -1): no arcs, not accepting); the first frontier
__global__ void fsa_seed_kernel(Prod p, int32_t start_a, int32_t start_b) {
  int32_t a = side(start_a, p.n_a, p.live_a), b = side(start_b, p.n_b, p.live_b);
  const uint64_t key = pair_key(p, a, b);
  if (!key) a = b = -1;
  if (key) {
    bool fresh;
    const int64_t slot = claim_slot(p, key, fresh);
    if (slot >= 0) p.ids[slot] = 0;
  }
  p.pairs[0] = a;
  p.pairs[1] = b;
  p.status[P_COUNT] = p.status[P_HI] = p.status[P_NEXT] = p.status[P_ENTERED] = 1;
}

// Every arc of the frontier: the target pair normalised, its weight written, its key entered.  delta_out takes the target's
// id where an earlier round numbered it, -1 where the arc does not exist, else -2 - slot until search_resolve_kernel; thread 0
// writes the state's own accepting / final weight.  The pairs entered are counted as they come: a wave adds its own to the
// block's count in LDS, and the block hands the count on to the status word in steps of 2^shift = max_states / 4096 or so
// (atomics on one word from every CU cost tens of nanoseconds each: one a wave would double the search's time) and what is
// left when it ends - the word is exact between launches.  Past max_states the overflow flag goes up in the middle of the
// launch, and every block leaves at its next state and every probe within 32 slots: a round of a wide frontier can bring
// 256 new pairs a state, many times the table, and must not fill it first.  What the blocks hold back is at most a quarter
// of max_states; a table that is full all the same holds table_slots >= 2 max_states distinct pairs: overflow too
__global__ __launch_bounds__(FSA_THREADS) void fsa_expand_kernel(Prod p) {
  __shared__ int32_t block_new, stop;  // (one read of the words for the block: it meets at barriers)
  if (threadIdx.x == 0) {
    block_new = 0;
    stop = stopped(p.status);
  }
  __syncthreads();
  if (stop) return;
  const int shift = max(0, 19 - __clz(p.max_states));  // (2^shift <= max_states / 4096)
  int32_t lo;
  const int32_t nk = round_states(p, lo);
  const int byte = (int)threadIdx.x;
  const float ninf = -__builtin_inff();
  for (int32_t k = (int32_t)blockIdx.x; k < nk; k += (int32_t)gridDim.x) {
    if (flags_now(p.status)) break;
    const int64_t s = (int64_t)lo + k;
    int32_t a = p.pairs[2 * s], b = p.pairs[2 * s + 1];  // (numbered pairs are normalised; checked all the same)
    a = a >= 0 && a < p.n_a ? a : -1;
    b = b >= 0 && b < p.n_b ? b : -1;
    const int32_t ta = a >= 0 ? side(p.delta_a[(int64_t)a * 256 + byte], p.n_a, p.live_a) : -1;
    const int32_t tb = b >= 0 ? side(p.delta_b[(int64_t)b * 256 + byte], p.n_b, p.live_b) : -1;
    const uint64_t key = pair_key(p, ta, tb);
    int32_t out = -1;
    bool fresh = false;
    if (key) {
      const int64_t slot = claim_slot(p, key, fresh);
      if (slot < 0) {
        fresh = false;
        if (slot == -1) overflow(p.status, (int64_t)p.mask + 1);
      } else {
        const int32_t id = p.ids[slot];  // (no launch of this round has written it)
        if (id >= 0) {
          out = id;
        } else {
          atomicMin(&p.arcmin[slot], k * 256 + byte);
          out = -2 - (int32_t)slot;
        }
      }
    }
    const int entered = __popcll(__ballot(fresh));  // (every lane of the wave is here: the loop's bounds are the block's)
    if (entered && (threadIdx.x & 63) == 0) {
      const int32_t before = atomicAdd(&block_new, entered);
      const int32_t steps = ((before + entered) >> shift) - (before >> shift);
      if (steps) count_entered(p, steps << shift);
    }
    p.delta_out[s * 256 + byte] = out;
    if (p.arc_out) {
      float w = ninf;
      if (key) {
        if (p.arc_a && p.arc_b && p.op == GLB_FSA_AND) w = p.arc_a[(int64_t)a * 256 + byte] + p.arc_b[(int64_t)b * 256 + byte];
        else if (p.arc_a) w = p.arc_a[(int64_t)a * 256 + byte];
        else if (p.arc_b && p.op == GLB_FSA_AND) w = p.arc_b[(int64_t)b * 256 + byte];
        else w = 0.0f;
      }
      p.arc_out[s * 256 + byte] = w;
    }
    if (byte == 0) {
      bool acc;
      float fin;
      pair_final(p, a, b, acc, fin);
      p.accepting_out[s] = acc ? 1 : 0;
      if (p.final_out) p.final_out[s] = fin;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && (block_new & ((1 << shift) - 1))) count_entered(p, block_new & ((1 << shift) - 1));
}

// ---- liveness ---------------------------------------------------------------------------------------------------------------
__global__ void live_init_kernel(int32_t n, const uint8_t *accepting, uint8_t *live, int32_t *status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 4) status[X_SWEEPS + i] = 0;
  if (i < n) live[i] = accepting[i] ? 1 : 0;
}

// a sweep, a wave per state: a state with a live successor is live.  In place: the rule only ever adds, so whatever a wave
// sees of the others' stores, the fixed point is the same set
__global__ __launch_bounds__(FSA_THREADS) void live_sweep_kernel(int32_t n, const int32_t *delta, uint8_t *live, int32_t *status) {
  if (status[X_CONVERGED]) return;
  const int lane = (int)threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (FSA_THREADS / 64);
  for (int64_t s = (int64_t)blockIdx.x * (FSA_THREADS / 64) + (threadIdx.x >> 6); s < n; s += waves) {
    if (live[s]) continue;  // (a whole wave)
    bool any = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int32_t d = delta[s * 256 + lane + 64 * k];
      any = any || (d >= 0 && d < n && live[d]);
    }
    if (__any(any) && lane == 0) {
      live[s] = 1;
      atomicOr(&status[X_CHANGED], 1);
    }
  }
}

int fsa_check(const glb_fsa_product_args *p, const char *what, bool round) {
  if (const int rc = glb::block_ok(p, what, "glb_fsa_product_args")) return rc;
  if (const int rc = check_max_states(what, p->max_states)) return rc;
  if (const int rc = check_rounds(what, p->rounds)) return rc;
  if (!p->delta_out) return glb::api_fail(GLB_EINVAL, "%s: delta_out is null", what);
  if (!p->accepting_out) return glb::api_fail(GLB_EINVAL, "%s: accepting_out is null", what);
  if (const int rc = check_status(what, p->status)) return rc;
  if (!round) {
    if (p->n_states < 1 || p->n_states > p->max_states)
      return glb::api_fail(GLB_EINVAL, "%s: n_states %d outside [1, max_states = %d]", what, p->n_states, p->max_states);
    if (!p->live) return glb::api_fail(GLB_EINVAL, "%s: live is null", what);
    return GLB_OK;
  }
  if (p->op != GLB_FSA_AND && p->op != GLB_FSA_OR && p->op != GLB_FSA_SUB) return glb::api_fail(GLB_EINVAL, "%s: op %d is none of and, or, sub", what, p->op);
  if (p->n_a < 1 || p->n_a > 0x7fffff00) return glb::api_fail(GLB_EINVAL, "%s: n_a %d outside [1, 2^31 - 256]", what, p->n_a);
  if (p->n_b < 1 || p->n_b > 0x7fffff00) return glb::api_fail(GLB_EINVAL, "%s: n_b %d outside [1, 2^31 - 256]", what, p->n_b);
  if (p->start_a < 0 || p->start_a >= p->n_a) return glb::api_fail(GLB_EINVAL, "%s: start_a %d outside [0, n_a = %d)", what, p->start_a, p->n_a);
  if (p->start_b < 0 || p->start_b >= p->n_b) return glb::api_fail(GLB_EINVAL, "%s: start_b %d outside [0, n_b = %d)", what, p->start_b, p->n_b);
  if (!p->delta_a || !p->delta_b) return glb::api_fail(GLB_EINVAL, "%s: delta_a or delta_b is null", what);
  if (!p->accepting_a || !p->accepting_b) return glb::api_fail(GLB_EINVAL, "%s: accepting_a or accepting_b is null", what);
  if (!p->live_a || !p->live_b) return glb::api_fail(GLB_EINVAL, "%s: live_a or live_b is null", what);
  if (!p->arc_a != !p->final_a) return glb::api_fail(GLB_EINVAL, "%s: arc_a and final_a go together", what);
  if (!p->arc_b != !p->final_b) return glb::api_fail(GLB_EINVAL, "%s: arc_b and final_b go together", what);
  if (p->arc_b && p->op != GLB_FSA_AND) return glb::api_fail(GLB_EINVAL, "%s: arc_b is given: only and takes a weighted second operand", what);
  if (p->arc_a && p->op == GLB_FSA_OR) return glb::api_fail(GLB_EINVAL, "%s: arc_a is given: or takes no weights", what);
  if (!p->arc_out != !(p->arc_a || p->arc_b)) return glb::api_fail(GLB_EINVAL, "%s: arc_out goes with the operands' weights", what);
  if (!p->arc_out != !p->final_out) return glb::api_fail(GLB_EINVAL, "%s: arc_out and final_out go together", what);
  if (const int rc = check_table(what, p->table_slots, p->max_states, p->table)) return rc;
  if (!p->pairs) return glb::api_fail(GLB_EINVAL, "%s: pairs is null", what);
  if (!p->counts) return glb::api_fail(GLB_EINVAL, "%s: counts is null", what);
  return GLB_OK;
}

}  // namespace

extern "C" {

int glb_fsa_product_round(const glb_fsa_product_args *a, void *stream) {
  if (const int rc = fsa_check(a, "glb_fsa_product_round", true)) return rc;
  unsigned blocks = 0;
  if (const int rc = stride_grid("fsa: the device's CU count", &blocks)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  unsigned long long *keys = (unsigned long long *)a->table;
  int32_t *arcmin = (int32_t *)(keys + a->table_slots);
  const Prod p{a->op, a->n_a, a->n_b, a->delta_a, a->delta_b, a->accepting_a, a->accepting_b, a->live_a, a->live_b,
               a->arc_a, a->final_a, a->arc_b, a->final_b, a->max_states, a->max_states, keys, arcmin, arcmin + a->table_slots,
               (uint64_t)a->table_slots - 1, a->pairs, a->delta_out, a->counts, a->accepting_out, a->arc_out, a->final_out, a->status};
  const dim3 grid(blocks), block(FSA_THREADS);
  if (a->restart) {
    hipLaunchKernelGGL(fsa_clear_kernel, dim3(blocks_for(a->table_slots, 256)), dim3(256), 0, st, p);
    hipLaunchKernelGGL(fsa_seed_kernel, dim3(1), dim3(1), 0, st, p, a->start_a, a->start_b);
  }
  for (int32_t j = 0; j < a->rounds; ++j) {
    hipLaunchKernelGGL(fsa_expand_kernel, grid, block, 0, st, p);
    round_tail(p, blocks, st);
  }
  return glb::launched("fsa_product_round launch");
}

int glb_fsa_live(const glb_fsa_product_args *a, void *stream) {
  if (const int rc = fsa_check(a, "glb_fsa_live", false)) return rc;
  unsigned blocks = 0;
  if (const int rc = stride_grid("fsa: the device's CU count", &blocks, a->n_states, FSA_THREADS / 64)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  if (a->restart)
    hipLaunchKernelGGL(live_init_kernel, dim3(blocks_for(a->n_states < 4 ? 4 : a->n_states, 256)), dim3(256), 0, st, a->n_states,
                       a->accepting_out, a->live, a->status);
  for (int32_t j = 0; j < a->rounds; ++j) {
    hipLaunchKernelGGL(live_sweep_kernel, dim3(blocks), dim3(FSA_THREADS), 0, st, a->n_states, a->delta_out, a->live, a->status);
    hipLaunchKernelGGL(fixpoint_end_kernel, dim3(1), dim3(1), 0, st, a->status + X_SWEEPS);
  }
  return glb::launched("fsa_live launch");
}

}  // extern "C"
