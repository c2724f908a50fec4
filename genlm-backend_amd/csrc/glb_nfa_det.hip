// glb_nfa_det.hip — a byte NFA with empty arcs made deterministic on the device (include/glb.h: glb_nfa_closure /
// glb_nfa_subset_round).  A state of the result is a SET of important NFA states, W = n_words 64-bit words: a
// wave holds one, a lane a word, lanes >= W zero - so OR-ing a closure row into a set is one load and one OR a lane, equality
// a compare and a ballot, the hash a wave reduction.  The search is the queue search of glb_search.hpp over chunks of the
// queue: a round takes the next `chunk` numbered states, seven launches - this file's two: the target set of every (state,
// byte group) written to `cand`, every target entered into the table; then the shared five: the winning arcs counted,
// scanned, numbered; delta_out resolved; the queue moved on.  The table cannot hold a set: a slot is ONE 64-bit word, a
// 31-bit hash and a reference - the arc of this round that claimed the slot (compare against that arc's row of `cand`,
// written by the launch BEFORE the one that probes: no wave ever waits for another's stores) or, once numbered, the state's
// id (compare against sets[id]).  The claimant is fixed by its compare-and-swap; equal hash with unequal set probes on; the
// smallest arc index to find a new set numbers it, so the arrays do not depend on the order the atomics take.  Everything
// read from device memory is range-checked.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/glb.h"
#include "glb_common.hpp"
#include "glb_search.hpp"
#include "glb_set.hpp"

namespace {

constexpr int NFA_THREADS = SEARCH_THREADS;  // four waves, an item each
constexpr int NFA_WAVES = NFA_THREADS / 64;
constexpr int32_t NFA_MAX_NFA_STATES = 1 << 24;
constexpr uint32_t REF_ARC = 0x80000000u;   // the low half: this bit and an arc index of the round, else the id of a numbered state

struct Det {
  int32_t n, start, n_imp, W, n_arcs, n_eps, G, chunk;
  const int32_t *eps_off, *eps_to, *bit_of, *arc_off, *arc_dst;
  const uint64_t *arc_bytes, *acc_mask;
  const int32_t *group_of, *group_lo;
  uint64_t *eclose;
  uint64_t hash_mask;
  int32_t max_states;
  unsigned long long *words;  // [slots]; 0: empty
  int32_t *arcmin;            // [slots]; the smallest arc index of the round that brought the slot's set
  uint64_t mask;              // slots - 1
  uint64_t *cand, *sets;
  int32_t *delta_out, *cnt;
  uint8_t *accepting_out;
  int32_t *status;

  // the winning arc's target becomes state `id`: the set copied from `cand`, its accepting bit, and the slot's reference
  // turned into the id (an arc index is made of its group's lowest byte, so no other byte of the group wins)
  static __device__ bool number(const Det &p, int64_t id, int32_t k, int byte, int64_t slot) {
    const int32_t g = p.group_of[byte];
    if (g < 0 || g >= p.G) return false;
    const uint64_t *row = p.cand + ((int64_t)k * p.G + g) * p.W;
    bool acc = false;
    for (int j = 0; j < p.W; ++j) {
      const uint64_t word = row[j];
      p.sets[id * p.W + j] = word;
      acc = acc || (word & p.acc_mask[j]) != 0;
    }
    p.accepting_out[id] = acc ? 1 : 0;
    p.words[slot] = (p.words[slot] & 0xffffffff00000000ull) | (unsigned long long)id;
    return true;
  }
  // the low half of the slot's word, once it is no arc of the round
  static __device__ int32_t id_of(const Det &p, int64_t slot) {
    const uint32_t ref = (uint32_t)p.words[slot];
    return ref & REF_ARC ? -1 : (int32_t)ref;
  }
};

// ---- the closure --------------------------------------------------------------------------------------------------------------
// eclose[v] = {v} where v is important, else empty; the closure's status words zeroed
__global__ void closure_init_kernel(Det p) {
  const int64_t total = (int64_t)p.n * p.W;
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (first < 4) p.status[X_SWEEPS + first] = 0;
  for (int64_t i = first; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t b = p.bit_of[i / p.W];
    p.eclose[i] = b >= 0 && b < p.n_imp && (b >> 6) == (int32_t)(i % p.W) ? 1ull << (b & 63) : 0ull;
  }
}

// a sweep, a wave per NFA state: eclose[v] |= eclose[u] over v's empty arcs.  In place: a row has one writer, the rule only
// adds, so whatever a wave sees of the others' stores the fixed point is the same - and a sweep that changed no row read
// nothing but final rows
__global__ __launch_bounds__(NFA_THREADS) void closure_sweep_kernel(Det p) {
  if (p.status[X_CONVERGED]) return;
  const int lane = (int)threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * NFA_WAVES;
  for (int64_t v = (int64_t)blockIdx.x * NFA_WAVES + (threadIdx.x >> 6); v < p.n; v += waves) {
    const int32_t e0 = p.eps_off[v], e1 = p.eps_off[v + 1];
    if (e0 < 0 || e1 > p.n_eps || e1 <= e0) continue;  // (a whole wave)
    unsigned long long *mine = (unsigned long long *)p.eclose + v * p.W + lane;
    const unsigned long long old = lane < p.W ? word_now(mine) : 0ull;
    unsigned long long row = old;
    for (int32_t e = e0; e < e1; ++e) {
      const int32_t u = p.eps_to[e];
      if (u >= 0 && u < p.n && lane < p.W) row |= word_now((const unsigned long long *)p.eclose + (int64_t)u * p.W + lane);
    }
    if (row != old) __hip_atomic_store(mine, row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (__any(row != old) && lane == 0) atomicOr(&p.status[X_CHANGED], 1);
  }
}

// ---- the search ---------------------------------------------------------------------------------------------------------------
// the table emptied and the search's status words zeroed (the closure's stay)
__global__ void nfa_clear_kernel(Det p) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < GLB_NFA_STATUS && !(i >= X_SWEEPS && i <= X_CHANGED)) p.status[i] = 0;
  if (i <= p.mask) {
    p.words[i] = 0;
    p.arcmin[i] = NO_ARC;
  }
}

// whether the set a wave holds has an accepting member, the same in every lane
__device__ inline bool set_accepts(const Det &p, uint64_t word, int lane) { return __any(lane < p.W && (word & p.acc_mask[lane]) != 0); }

// where the probing of a set starts, and the high half of its slot
__device__ inline void set_key(const Det &p, uint64_t word, int lane, uint64_t &slot, uint32_t &high) {
  set_key(p.hash_mask, p.mask, word, lane, slot, high);
}

// state 0: the closure of the start, one wave; an empty set is a state here and nowhere else, and stays out of the table
__global__ __launch_bounds__(64) void nfa_seed_kernel(Det p) {
  const int lane = (int)threadIdx.x;
  const uint64_t word = lane < p.W ? p.eclose[(int64_t)p.start * p.W + lane] : 0ull;
  if (lane < p.W) p.sets[lane] = word;
  const bool acc = set_accepts(p, word, lane), some = __any(word != 0);
  uint64_t slot;
  uint32_t high;
  set_key(p, word, lane, slot, high);
  if (lane == 0) {
    p.accepting_out[0] = acc ? 1 : 0;
    if (some) p.words[slot] = (unsigned long long)high << 32;  // (id 0; the table is empty)
    p.status[P_COUNT] = p.status[P_HI] = p.status[P_NEXT] = p.status[P_ENTERED] = 1;
  }
}

// cand[k][g]: the set that byte group g leads to from queue state lo + k - over the members of the state, by bit scan, and
// each member's byte arcs, the closure row of every arc that reads the group's lowest byte.  A wave per (k, g)
__global__ __launch_bounds__(NFA_THREADS) void nfa_expand_kernel(Det p) {
  if (stopped(p.status)) return;
  int32_t lo;
  const int32_t nk = round_states(p, lo);
  const int lane = (int)threadIdx.x & 63;
  const int64_t items = (int64_t)nk * p.G, waves = (int64_t)gridDim.x * NFA_WAVES;
  for (int64_t it = (int64_t)blockIdx.x * NFA_WAVES + (threadIdx.x >> 6); it < items; it += waves) {
    const int64_t s = (int64_t)lo + it / p.G;
    const int32_t byte = p.group_lo[it % p.G];
    const uint64_t mine = lane < p.W ? p.sets[s * p.W + lane] : 0ull;
    uint64_t target = 0;
    for (int w = 0; w < p.W && byte >= 0 && byte < 256; ++w) {
      uint64_t word = bcast64(mine, w);  // (the same in every lane: the loops below are the wave's)
      while (word) {
        const int32_t m = w * 64 + __ffsll((unsigned long long)word) - 1;
        word &= word - 1;
        if (m >= p.n_imp) break;
        const int32_t a0 = p.arc_off[m], a1 = p.arc_off[m + 1];
        if (a0 < 0 || a1 > p.n_arcs) continue;
        for (int32_t a = a0; a < a1; ++a) {
          if (!((p.arc_bytes[4 * (int64_t)a + (byte >> 6)] >> (byte & 63)) & 1ull)) continue;
          const int32_t d = p.arc_dst[a];
          if (d >= 0 && d < p.n && lane < p.W) target |= p.eclose[(int64_t)d * p.W + lane];
        }
      }
    }
    if (lane < p.W) p.cand[it * p.W + lane] = target;
  }
}

// the row of the set behind a slot's reference: cand of the arc that claimed it this round, or sets of its id; null: a bug
__device__ inline const uint64_t *behind(const Det &p, uint32_t ref, int32_t nk) {
  if (ref & REF_ARC) {
    const int32_t arc = (int32_t)(ref & 0x7fffffffu), k = arc >> 8;
    const int32_t g = p.group_of[arc & 255];
    return k < nk && g >= 0 && g < p.G ? p.cand + ((int64_t)k * p.G + g) * p.W : nullptr;
  }
  return (int32_t)ref < p.max_states ? p.sets + (int64_t)ref * p.W : nullptr;
}

// Every target set enters the table, a wave per (k, g): delta_out of the group's bytes takes the set's id where an earlier
// round numbered it, -1 where the set is empty, else -2 - slot until search_resolve_kernel.  A new set's slot is claimed by one
// compare-and-swap and counted; past max_states the overflow flag goes up in the middle of the launch and every wave leaves
// at its next item or within 32 slots
__global__ __launch_bounds__(NFA_THREADS) void nfa_enter_kernel(Det p) {
  if (stopped(p.status)) return;
  int32_t lo;
  const int32_t nk = round_states(p, lo);
  const int lane = (int)threadIdx.x & 63;
  const int64_t items = (int64_t)nk * p.G, waves = (int64_t)gridDim.x * NFA_WAVES;
  for (int64_t it = (int64_t)blockIdx.x * NFA_WAVES + (threadIdx.x >> 6); it < items; it += waves) {
    if (flags_now(p.status)) break;
    const int32_t k = (int32_t)(it / p.G), g = (int32_t)(it % p.G);
    const int32_t byte = p.group_lo[g];
    const uint64_t target = lane < p.W ? p.cand[it * p.W + lane] : 0ull;
    int32_t out = -1;
    if (__any(target != 0) && byte >= 0 && byte < 256) {
      const int32_t arc = k * 256 + byte;
      uint64_t slot;
      uint32_t high;
      set_key(p, target, lane, slot, high);
      const unsigned long long claim = ((unsigned long long)high << 32) | REF_ARC | (uint32_t)arc;
      uint64_t probe = 0;
      for (; probe <= p.mask; ++probe, slot = (slot + 1) & p.mask) {
        unsigned long long cur = word_now(&p.words[slot]);  // (one address: the same in every lane)
        if (cur == 0ull) {
          unsigned long long old = 0ull;
          if (lane == 0) old = atomicCAS(&p.words[slot], 0ull, claim);
          old = bcast64(old, 0);
          if (old == 0ull) {  // this wave's: a new set
            if (lane == 0) {
              atomicMin(&p.arcmin[slot], arc);
              const int64_t total = (int64_t)atomicAdd(&p.status[P_ENTERED], 1) + 1;
              if (total > p.max_states) overflow(p.status, total);
            }
            out = -2 - (int32_t)slot;
            break;
          }
          cur = old;
        }
        if ((uint32_t)(cur >> 32) == high) {
          const uint32_t ref = (uint32_t)cur;
          const uint64_t *row = behind(p, ref, nk);
          if (!row) {
            if (lane == 0) atomicOr(&p.status[P_FLAGS], F_TABLE);
            break;
          }
          const uint64_t other = lane < p.W ? row[lane] : 0ull;
          if (!__any(other != target)) {
            if (ref & REF_ARC) {
              if (lane == 0) atomicMin(&p.arcmin[slot], arc);
              out = -2 - (int32_t)slot;
            } else {
              out = (int32_t)ref;
            }
            break;
          }
        }
        if ((probe & 31) == 31 && flags_now(p.status)) break;
      }
      if (probe > p.mask && lane == 0) overflow(p.status, (int64_t)p.mask + 1);  // (a full table holds >= 2 max_states sets)
    }
    const int64_t s = (int64_t)lo + k;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (p.group_of[lane + 64 * j] == g) p.delta_out[s * 256 + lane + 64 * j] = out;
  }
}

int nfa_check(const glb_nfa_args *p, const char *what, bool round) {
  if (const int rc = glb::block_ok(p, what, "glb_nfa_args")) return rc;
  if (p->n_states < 1 || p->n_states > NFA_MAX_NFA_STATES)
    return glb::api_fail(GLB_EINVAL, "%s: n_states %d outside [1, %d]", what, p->n_states, NFA_MAX_NFA_STATES);
  if (p->n_important < 0 || p->n_important > GLB_NFA_MAX_IMPORTANT || p->n_important > p->n_states)
    return glb::api_fail(GLB_EINVAL, "%s: n_important %d outside [0, min(n_states, %d)]: a set is one wave, a 64-bit word a lane", what,
                         p->n_important, GLB_NFA_MAX_IMPORTANT);
  const int32_t words = p->n_important > 64 ? (p->n_important + 63) / 64 : 1;
  if (p->n_words != words) return glb::api_fail(GLB_EINVAL, "%s: n_words %d is not max(1, ceil(n_important / 64)) = %d", what, p->n_words, words);
  if (p->start < 0 || p->start >= p->n_states) return glb::api_fail(GLB_EINVAL, "%s: start %d outside [0, n_states = %d)", what, p->start, p->n_states);
  if (const int rc = check_rounds(what, p->rounds)) return rc;
  if (!p->eclose) return glb::api_fail(GLB_EINVAL, "%s: eclose is null", what);
  if (const int rc = check_status(what, p->status)) return rc;
  if (!round) {
    if (p->n_eps < 0) return glb::api_fail(GLB_EINVAL, "%s: n_eps %d is negative", what, p->n_eps);
    if (!p->eps_off || !p->eps_to) return glb::api_fail(GLB_EINVAL, "%s: eps_off or eps_to is null", what);
    if (!p->bit_of) return glb::api_fail(GLB_EINVAL, "%s: bit_of is null", what);
    return GLB_OK;
  }
  if (p->n_arcs < 0) return glb::api_fail(GLB_EINVAL, "%s: n_arcs %d is negative", what, p->n_arcs);
  if (p->n_groups < 1 || p->n_groups > 256) return glb::api_fail(GLB_EINVAL, "%s: n_groups %d outside [1, 256]", what, p->n_groups);
  if (const int rc = check_max_states(what, p->max_states)) return rc;
  if (p->chunk < 1 || p->chunk > p->max_states) return glb::api_fail(GLB_EINVAL, "%s: chunk %d outside [1, max_states = %d]", what, p->chunk, p->max_states);
  if (!p->arc_off || !p->arc_dst || !p->arc_bytes) return glb::api_fail(GLB_EINVAL, "%s: arc_off, arc_dst or arc_bytes is null", what);
  if (!p->accepting_mask) return glb::api_fail(GLB_EINVAL, "%s: accepting_mask is null", what);
  if (!p->group_of || !p->group_lo) return glb::api_fail(GLB_EINVAL, "%s: group_of or group_lo is null", what);
  if (const int rc = check_table(what, p->table_slots, p->max_states, p->table)) return rc;
  if (!p->cand) return glb::api_fail(GLB_EINVAL, "%s: cand is null", what);
  if (!p->sets) return glb::api_fail(GLB_EINVAL, "%s: sets is null", what);
  if (!p->delta_out) return glb::api_fail(GLB_EINVAL, "%s: delta_out is null", what);
  if (!p->accepting_out) return glb::api_fail(GLB_EINVAL, "%s: accepting_out is null", what);
  if (!p->counts) return glb::api_fail(GLB_EINVAL, "%s: counts is null", what);
  return GLB_OK;
}

Det det_of(const glb_nfa_args *a) {
  unsigned long long *words = (unsigned long long *)a->table;
  return Det{a->n_states, a->start, a->n_important, a->n_words, a->n_arcs, a->n_eps, a->n_groups, a->chunk,
             a->eps_off, a->eps_to, a->bit_of, a->arc_off, a->arc_dst, a->arc_bytes, a->accepting_mask, a->group_of, a->group_lo,
             a->eclose, a->hash_mask, a->max_states, words, (int32_t *)(words + a->table_slots), (uint64_t)a->table_slots - 1, a->cand,
             a->sets, a->delta_out, a->counts, a->accepting_out, a->status};
}

}  // namespace

extern "C" {

int glb_nfa_closure(const glb_nfa_args *a, void *stream) {
  if (const int rc = nfa_check(a, "glb_nfa_closure", false)) return rc;
  unsigned blocks = 0;
  if (const int rc = stride_grid("nfa: the device's CU count", &blocks)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  Det p{};
  p.n = a->n_states, p.n_imp = a->n_important, p.W = a->n_words, p.n_eps = a->n_eps;
  p.eps_off = a->eps_off, p.eps_to = a->eps_to, p.bit_of = a->bit_of, p.eclose = a->eclose, p.status = a->status;
  const unsigned need = blocks_for(a->n_states, NFA_WAVES);
  const dim3 grid(need < blocks ? need : blocks), block(NFA_THREADS);
  if (a->restart) hipLaunchKernelGGL(closure_init_kernel, dim3(blocks), dim3(256), 0, st, p);
  for (int32_t j = 0; j < a->rounds; ++j) {
    hipLaunchKernelGGL(closure_sweep_kernel, grid, block, 0, st, p);
    hipLaunchKernelGGL(fixpoint_end_kernel, dim3(1), dim3(1), 0, st, a->status + X_SWEEPS);
  }
  return glb::launched("nfa_closure launch");
}

int glb_nfa_subset_round(const glb_nfa_args *a, void *stream) {
  if (const int rc = nfa_check(a, "glb_nfa_subset_round", true)) return rc;
  unsigned blocks = 0;
  if (const int rc = stride_grid("nfa: the device's CU count", &blocks)) return rc;
  const hipStream_t st = (hipStream_t)stream;
  const Det p = det_of(a);
  const dim3 grid(blocks), block(NFA_THREADS);
  if (a->restart) {
    hipLaunchKernelGGL(nfa_clear_kernel, dim3(blocks_for(a->table_slots, 256)), dim3(256), 0, st, p);
    hipLaunchKernelGGL(nfa_seed_kernel, dim3(1), dim3(64), 0, st, p);
  }
  for (int32_t j = 0; j < a->rounds; ++j) {
    hipLaunchKernelGGL(nfa_expand_kernel, grid, block, 0, st, p);
    hipLaunchKernelGGL(nfa_enter_kernel, grid, block, 0, st, p);
    round_tail(p, blocks, st);
  }
  return glb::launched("nfa_subset_round launch");
}

}  // extern "C"
