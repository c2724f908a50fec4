// glb_search.hpp — the breadth-first queue search that builds an automaton on the device: what
// glb_fsa_product.hip (a state is a pair of states) and glb_nfa_det.hip (a set of NFA states) share.  The states are numbered
// in the order a host queue search meets them.  A round takes the next `chunk` states of the queue; the unit's own launches
// write, for every arc (queue position k of the round, byte), delta_out = the target's id where an earlier round numbered it,
// -1 where there is no target, else -2 - slot of the target in the unit's table, and lower arcmin[slot] to the arc's index
// k * 256 + byte.  Then the five launches here: count (the arcs that hold their slot's minimum are the winners, one a new
// state), scan, number (id = the states numbered + the prefix of state k + the rank among its winners: the order (k, byte)),
// resolve (-2 - slot becomes the id) and advance.  The queue's bounds live in the status words and every grid strides over
// them: no launch depends on a host read; with the converged word or a flag set every launch leaves at once.
//
// The kernels are templates over the unit's parameter struct P, passed by value.  P has: max_states, chunk, arcmin, mask,
// delta_out, cnt, status, and
//   static __device__ bool number(const P &p, int64_t id, int32_t k, int byte, int64_t slot)
// that writes what the unit keeps of new state `id`, found by arc (k, byte), and makes `slot` name it; false: a bug, and
//   static __device__ int32_t id_of(const P &p, int64_t slot)
// the id `slot` names, negative where it names none.
// The scan, the rank and the launch grid are glb_block.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/glb.h"
#include "glb_block.hpp"
#include "glb_common.hpp"

namespace {

// status: the search [0 .. 7] and [12]; [8 .. 11] the four words of a sweep to a fixed point (liveness, the closure)
enum { P_ROUNDS = 0, P_CONVERGED = 1, P_FLAGS = 2, P_COUNT = 3, P_LO = 4, P_HI = 5, P_NEXT = 6, P_REACHED = 7,
       X_SWEEPS = 8, X_CONVERGED = 9, X_FLAGS = 10, X_CHANGED = 11, P_ENTERED = 12 };
enum { F_OVERFLOW = 1, F_TABLE = 2 };
static_assert(P_ENTERED < GLB_FSA_STATUS && GLB_FSA_STATUS == GLB_NFA_STATUS, "");
static_assert(X_SWEEPS == 8 && X_CHANGED == X_SWEEPS + 3, "include/glb.h: glb_fsa_live and glb_nfa_closure own status[8 .. 11]");
constexpr int SEARCH_THREADS = 256;  // the 256 bytes of one state
constexpr int SEARCH_MAX_ROUNDS = 65536;        // rounds / sweeps one call may enqueue
constexpr int32_t SEARCH_MAX_STATES = 1 << 22;  // (an arc index queue position * 256 + byte stays an int32)
constexpr int32_t NO_ARC = 0x7fffffff;

// the flag word as it is now, whatever this thread read before (another block of the same launch may have raised a flag)
__device__ inline int32_t flags_now(const int32_t *status) {
  return __hip_atomic_load(&status[P_FLAGS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ inline bool stopped(const int32_t *status) { return status[P_CONVERGED] != 0 || status[P_FLAGS] != 0; }

// more than max_states states: flag bit 0 and the count that passed it
__device__ inline void overflow(int32_t *status, int64_t reached) {
  atomicMax(&status[P_REACHED], (int32_t)(reached < 0x7fffffff ? reached : 0x7fffffff));
  atomicOr(&status[P_FLAGS], F_OVERFLOW);
}

// the states of the queue this round takes: [lo, lo + the value returned).  What the kernels below rely on: a unit's seed
// leaves P_LO = 0 and P_COUNT = P_HI = P_NEXT = 1, and the scan never lets P_NEXT pass max_states; so behind every advance
// the states numbered are P_COUNT <= max_states - the base of the round's ids - and P_HI = min(P_COUNT, P_LO + chunk).  A unit
// whose chunk is max_states (the product) takes all of the queue: P_HI == P_COUNT, a round's states are those the round
// before numbered, and the search has converged when P_LO == P_HI
template <typename P>
__device__ inline int32_t round_states(const P &p, int32_t &lo) {
  lo = p.status[P_LO];
  const int32_t hi = min(p.status[P_HI], p.max_states);
  return lo >= 0 ? max(0, min(hi - lo, p.chunk)) : 0;
}

// whether the arc (queue position k, byte) is the one that numbers its target: the smallest arc of the round to find it
template <typename P>
__device__ inline bool wins(const P &p, int32_t code, int32_t arc, int64_t &slot) {
  slot = -2 - (int64_t)code;
  return code <= -2 && (uint64_t)slot <= p.mask && p.arcmin[slot] == arc;
}

// cnt[k]: the states that queue state lo + k is the first to reach
template <typename P>
__global__ __launch_bounds__(SEARCH_THREADS) void search_count_kernel(P p) {
  if (stopped(p.status)) return;
  int32_t lo;
  const int32_t nk = round_states(p, lo);
  for (int32_t k = (int32_t)blockIdx.x; k < nk; k += (int32_t)gridDim.x) {
    int64_t slot;
    const bool w = wins(p, p.delta_out[((int64_t)lo + k) * 256 + threadIdx.x], k * 256 + (int)threadIdx.x, slot);
    const int n = __syncthreads_count(w);
    if (threadIdx.x == 0) p.cnt[k] = n;
  }
}

// one block: cnt becomes its exclusive prefix sums over the round's states; P_NEXT = the states after this round; past
// max_states the overflow flag and the count reached (P_REACHED is 0 until then: overflow() raises it only with a flag, and
// this kernel leaves when one is up)
template <typename P>
__global__ __launch_bounds__(SCAN_THREADS) void search_scan_kernel(P p) {
  __shared__ int32_t wave_sum[SCAN_THREADS / 64];
  __shared__ int32_t carry;
  if (stopped(p.status)) return;  // (uniform: the block's one writer of the words comes behind the last barrier)
  int32_t lo;
  const int32_t nk = round_states(p, lo);
  const int32_t total = scan_exclusive(p.cnt, nk, wave_sum, &carry);
  if (threadIdx.x == 0) {
    const int64_t next = (int64_t)p.status[P_COUNT] + total;  // (total <= 256 * chunk <= 2^30)
    if (next > p.max_states) overflow(p.status, next);
    else p.status[P_NEXT] = (int32_t)next;
  }
}

// the winning arcs number their targets: id = P_COUNT + cnt[k] + the winners of state k at smaller bytes; P::number writes
// the state
template <typename P>
__global__ __launch_bounds__(SEARCH_THREADS) void search_number_kernel(P p) {
  __shared__ int32_t wave_n[SEARCH_THREADS / 64];
  __shared__ int32_t stop;  // (one read for the block: a thread of this launch may raise a flag, and the block meets at barriers)
  if (threadIdx.x == 0) stop = stopped(p.status);
  __syncthreads();
  if (stop) return;
  int32_t lo;
  const int32_t nk = round_states(p, lo), count = p.status[P_COUNT];
  for (int32_t k = (int32_t)blockIdx.x; k < nk; k += (int32_t)gridDim.x) {
    int64_t slot;
    const bool w = wins(p, p.delta_out[((int64_t)lo + k) * 256 + threadIdx.x], k * 256 + (int)threadIdx.x, slot);
    const int32_t rank = block_rank(w, wave_n);
    if (w) {
      const int64_t id = (int64_t)count + p.cnt[k] + rank;
      if (!(id >= 0 && id < p.max_states && P::number(p, id, k, (int)threadIdx.x, slot))) atomicOr(&p.status[P_FLAGS], F_TABLE);
    }
    __syncthreads();
  }
}

// delta_out of the round's states: -2 - slot becomes the id its slot was given
template <typename P>
__global__ __launch_bounds__(SEARCH_THREADS) void search_resolve_kernel(P p) {
  if (stopped(p.status)) return;
  int32_t lo;
  const int32_t nk = round_states(p, lo);
  for (int32_t k = (int32_t)blockIdx.x; k < nk; k += (int32_t)gridDim.x) {
    int32_t *cell = &p.delta_out[((int64_t)lo + k) * 256 + threadIdx.x];
    const int32_t code = *cell;
    if (code > -2) continue;
    const int64_t slot = -2 - (int64_t)code;
    int32_t id = -1;
    if ((uint64_t)slot <= p.mask) id = P::id_of(p, slot);
    if (id < 0 || id >= p.max_states) {
      atomicOr(&p.status[P_FLAGS], F_TABLE);
      id = -1;
    }
    *cell = id;
  }
}

// the round's last launch, one thread: the queue moves on by the states taken; with nothing left in it the search is over
__global__ void search_advance_kernel(int32_t *status, int32_t chunk) {
  if (stopped(status)) return;
  status[P_ROUNDS] += 1;
  status[P_LO] = status[P_HI];
  status[P_COUNT] = status[P_NEXT];
  status[P_HI] = min(status[P_COUNT], status[P_LO] + chunk);
  if (status[P_LO] >= status[P_COUNT]) status[P_CONVERGED] = 1;
}

// behind a sweep to a fixed point, one thread; status4: sweeps, converged, flags, changed.  A sweep that changed nothing
// was the last
__global__ void fixpoint_end_kernel(int32_t *status4) {
  if (status4[X_CONVERGED - X_SWEEPS]) return;
  status4[0] += 1;
  if (!status4[X_CHANGED - X_SWEEPS]) status4[X_CONVERGED - X_SWEEPS] = 1;
  status4[X_CHANGED - X_SWEEPS] = 0;
}

// ---- the host side -----------------------------------------------------------------------------------------------------------------
// the launches of a round behind the unit's own: count, scan, number, resolve, advance
template <typename P>
void round_tail(const P &p, unsigned blocks, hipStream_t st) {
  const dim3 grid(blocks), block(SEARCH_THREADS);
  hipLaunchKernelGGL(search_count_kernel<P>, grid, block, 0, st, p);
  hipLaunchKernelGGL(search_scan_kernel<P>, dim3(1), dim3(SCAN_THREADS), 0, st, p);
  hipLaunchKernelGGL(search_number_kernel<P>, grid, block, 0, st, p);
  hipLaunchKernelGGL(search_resolve_kernel<P>, grid, block, 0, st, p);
  hipLaunchKernelGGL(search_advance_kernel, dim3(1), dim3(1), 0, st, p.status, p.chunk);
}

// what both argument blocks are refused for alike; each unit calls them in its own order, among its own checks
inline int check_max_states(const char *what, int32_t max_states) {
  if (max_states >= 1 && max_states <= SEARCH_MAX_STATES) return GLB_OK;
  return glb::api_fail(GLB_EINVAL, "%s: max_states %d outside [1, %d]", what, max_states, SEARCH_MAX_STATES);
}

inline int check_rounds(const char *what, int32_t rounds) {
  if (rounds >= 1 && rounds <= SEARCH_MAX_ROUNDS) return GLB_OK;
  return glb::api_fail(GLB_EINVAL, "%s: rounds %d outside [1, %d]", what, rounds, SEARCH_MAX_ROUNDS);
}

inline int check_status(const char *what, const int32_t *status) {
  return status ? GLB_OK : glb::api_fail(GLB_EINVAL, "%s: status is null", what);
}

inline int check_table(const char *what, int64_t table_slots, int32_t max_states, const void *table) {
  if (table_slots < 2 * (int64_t)max_states || table_slots > ((int64_t)1 << 30) || (table_slots & (table_slots - 1)))
    return glb::api_fail(GLB_EINVAL, "%s: table_slots %lld is not a power of two in [2 max_states = %lld, 2^30]", what,
                         (long long)table_slots, 2 * (long long)max_states);
  if (!table) return glb::api_fail(GLB_EINVAL, "%s: table is null", what);
  if ((uintptr_t)table & 7) return glb::api_fail(GLB_EINVAL, "%s: table is not aligned to 8 bytes", what);
  return GLB_OK;
}

}  // namespace
