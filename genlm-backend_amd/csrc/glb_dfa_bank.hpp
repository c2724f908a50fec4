// glb_dfa_bank.hpp — the bank of rows behind a constraint: its first two rows, the claim of a row by a state,
// the filled mark, every particle's row id, and the eviction of the least recently requested rows.  These kernels read
// n_states, accepting and row_of_state of their automaton and nothing else, so they serve the tables of glb_dfa.hip and the
// sets of glb_lazy.hip (§24) alike; each translation unit brings its own fill.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/glb.h"

namespace {

enum { C_ROWS = 0, C_FILLED = 1, C_OVERFLOW = 2, C_RESERVED = 3 };
enum { E_CLAIMANTS = 0, E_TAKEN = 1, E_FILLS = 2, E_EVICTIONS = 3 };  // glb_dfa_evict_args.ecounters
constexpr int SELECT_THREADS = 1024;  // the selection's one workgroup
constexpr int FILL_THREADS = 256;    // four waves: 256 consecutive tokens of one state
constexpr int FILL_MAX_ENTRIES = 64; // grid.y: work entries served side by side (a block loops over the rest)

// rows 0 (nothing) and 1 (EOS alone) of a bank of bit words (T = int32_t: `elems` words) or of log-weights (float: `elems`
// tokens), no state with a row
template <typename T>
__global__ void dfa_bank_init_kernel(int32_t n_states, int32_t eos_id, int64_t vocab, T *bank, int64_t bank_ld, int64_t elems,
                                     int32_t *row_of_state, int32_t *counters) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_states) row_of_state[i] = -1;
  if (i < elems) {
    if constexpr (std::is_same_v<T, float>) {
      bank[i] = -__builtin_inff();
      bank[bank_ld + i] = i == eos_id ? 0.0f : -__builtin_inff();
    } else {
      bank[i] = 0;
      const bool eos_here = eos_id >= 0 && eos_id < vocab && (eos_id >> 5) == i;
      bank[bank_ld + i] = eos_here ? (int32_t)(1u << (eos_id & 31)) : 0;
    }
  }
  if (i == 0) {
    counters[C_ROWS] = 2;
    counters[C_FILLED] = 0;
    counters[C_OVERFLOW] = 0;
    counters[C_RESERVED] = 0;
  }
}

__global__ void dfa_claim_kernel(int32_t n_states, int64_t n, const int32_t *states, int32_t capacity, int32_t *row_of_state,
                                 int32_t *work, int32_t *counters) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t s = states[i];
  if (s < 0 || s >= n_states) return;
  if (__hip_atomic_load(&row_of_state[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != -1) return;
  if (atomicCAS(&row_of_state[s], -1, -2) != -1) return;  // somebody else claims for this state
  const int32_t r = atomicAdd(&counters[C_ROWS], 1);
  if (r >= 2 && r < capacity) {
    work[2 * (int64_t)(r - 2)] = s;
    work[2 * (int64_t)(r - 2) + 1] = r;
    atomicExch(&row_of_state[s], r);
  } else {  // the bank is full: the state stays without a row, the counter where it was
    atomicSub(&counters[C_ROWS], 1);
    atomicExch(&row_of_state[s], -1);
    atomicOr(&counters[C_OVERFLOW], 1);
  }
}

// The entries of the work list to fill, read by one thread of a fill's block from `counters`: the claim path's
// [counters[C_FILLED], counters[C_ROWS] - 2); EVICT (`counters` the block's ecounters): a serve call's [0, ecounters[E_TAKEN])
template <bool EVICT>
__device__ inline void fill_range(const int32_t *counters, int32_t capacity, int32_t *range) {
  if constexpr (EVICT) {
    const int32_t t = __hip_atomic_load(&counters[E_TAKEN], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    range[0] = 0;
    range[1] = t > capacity - 2 ? capacity - 2 : t;
  } else {
    int32_t begin = __hip_atomic_load(&counters[C_FILLED], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int32_t end = __hip_atomic_load(&counters[C_ROWS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    end = (end > capacity ? capacity : end) - 2;
    if (begin < 0) begin = 0;
    range[0] = begin;
    range[1] = end;
  }
}

// after the fill (same stream): the filled mark moves up.  A launch of its own: a count of arrived workgroups on one word
// costs more than this once the grid has thousands of them
__global__ void dfa_commit_kernel(int32_t capacity, int32_t *counters) {
  const int32_t rows = counters[C_ROWS];
  const int32_t end = (rows > capacity ? capacity : rows) - 2;
  if (end > counters[C_FILLED]) counters[C_FILLED] = end;
}

// the id of one particle: row 0 for a dead state or one without a row; `done`: row 1 if the state is accepting, else 0
__device__ inline int32_t dfa_mask_id(int32_t n_states, const uint8_t *accepting, int32_t s, bool done, const int32_t *row_of_state,
                                      int32_t capacity) {
  const bool ok = s >= 0 && s < n_states;
  if (done) return ok && accepting[s] ? 1 : 0;
  if (!ok) return 0;
  const int32_t r = row_of_state[s];
  return r < 2 || r >= capacity ? 0 : r;
}

// with `ecounters` and `epoch` (a serve call) the call ends here: the epoch moves on, the call's two counts go back to zero
__global__ void dfa_mask_ids_kernel(int32_t n_states, const uint8_t *accepting, int64_t n, const int32_t *states, const int32_t *done,
                                    const int32_t *row_of_state, int32_t capacity, int32_t *out, int32_t *ecounters, int32_t *epoch) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 && ecounters && epoch) {  // (no launch of this call reads either after the selection)
    if (*epoch < 0x7fffffff) *epoch += 1;
    ecounters[E_CLAIMANTS] = 0;
    ecounters[E_TAKEN] = 0;
  }
  if (i >= n) return;
  out[i] = dfa_mask_id(n_states, accepting, states[i], done && done[i], row_of_state, capacity);
}

// ---- a bank smaller than the automaton (glb_dfa_evict_*) -------------------------------------------------------
__global__ void dfa_evict_init_kernel(int32_t capacity, int32_t *row_state, int32_t *row_stamp, int32_t *ecounters, int32_t *epoch) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < capacity) {
    row_state[i] = -1;
    row_stamp[i] = 0;
  }
  if (i < GLB_DFA_EVICT_COUNTERS) ecounters[i] = 0;
  if (i == 0) *epoch = 1;
}

// touch: the rows asked for are stamped; a state without a row is elected once (the claim kernel's CAS) and listed
__global__ void dfa_evict_touch_kernel(int32_t n_states, int64_t n, const int32_t *states, int32_t capacity, int32_t *row_of_state,
                                       int32_t *row_stamp, int32_t *claimants, int32_t *counters, int32_t *ecounters,
                                       const int32_t *epoch) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t s = states[i];
  if (s < 0 || s >= n_states) return;
  const int32_t r = __hip_atomic_load(&row_of_state[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (r >= 2 && r < capacity) {
    row_stamp[r] = *epoch;
    return;
  }
  if (r != -1 || atomicCAS(&row_of_state[s], -1, -2) != -1) return;  // somebody else claims for this state
  const int32_t j = atomicAdd(&ecounters[E_CLAIMANTS], 1);
  if (j >= 0 && j < capacity) {
    claimants[j] = s;
  } else {  // more claimants than the list (and so the bank) holds: the counter where it was, the state without a row
    atomicSub(&ecounters[E_CLAIMANTS], 1);
    atomicExch(&row_of_state[s], -1);
    atomicOr(&counters[C_OVERFLOW], 1);
  }
}

// One workgroup: the `take` rows of [2, capacity) with the smallest stamps among those not stamped with this call's epoch
// (a radix select, eight bits a pass, the histogram in LDS), then the rows handed to the claimants.  The stamps are read from
// L2 five times at the most: capacity <= 65535, 64 loads a thread and pass
__global__ __launch_bounds__(SELECT_THREADS) void dfa_evict_select_kernel(int32_t n_states, int32_t capacity, int32_t *row_of_state,
                                                                         int32_t *row_state, int32_t *row_stamp,
                                                                         const int32_t *claimants, int32_t *victims, int32_t *work,
                                                                         int32_t *counters, int32_t *ecounters, const int32_t *epoch_p) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t pick[3];   // the digit of the k-th smallest stamp, k among the stamps of that digit; the rows to take
  __shared__ uint32_t found[3];  // victims with a stamp below the threshold, with the threshold's stamp; rows taken from a state
  int32_t claim = ecounters[E_CLAIMANTS];
  if (claim <= 0) return;  // (uniform) the steady state: every state asked for has its row
  if (claim > capacity) claim = capacity;
  const int32_t epoch = *epoch_p;
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int32_t sweeps = (capacity - 2 + SELECT_THREADS - 1) / SELECT_THREADS;  // (uniform: the ballots want whole waves)
  if (tid == 0) found[0] = found[1] = found[2] = 0;
  uint32_t prefix = 0, mask = 0, k = 0, take = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    for (int32_t j = 0; j < sweeps; ++j) {
      const int32_t r = 2 + j * SELECT_THREADS + tid;
      const uint32_t st = r < capacity ? (uint32_t)row_stamp[r] : 0u;
      const bool in = r < capacity && st != (uint32_t)epoch && (st & mask) == prefix;
      const uint32_t digit = (st >> shift) & 255u;
      // stamps are call numbers, mostly close together: a wave whose candidates share the digit adds once
      const uint64_t m = __ballot(in);
      if (m) {
        const int leader = __ffsll((unsigned long long)m) - 1;
        const uint32_t d0 = (uint32_t)__shfl((int)digit, leader);
        if (__ballot(in && digit == d0) == m) {
          if (lane == leader) atomicAdd(&hist[d0], (uint32_t)__popcll(m));
        } else if (in) {
          atomicAdd(&hist[digit], 1u);
        }
      }
    }
    __syncthreads();
    if (tid < 64) {  // the bin that holds the k-th smallest: four bins a lane, a scan over the wave
      const uint32_t c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
      uint32_t incl = c0 + c1 + c2 + c3;
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, d);
        if (lane >= d) incl += up;
      }
      uint32_t want = k;
      if (shift == 24) {  // the first pass counts the candidates: no more rows are taken than there are
        const uint32_t total = (uint32_t)__shfl((int)incl, 63);
        want = (uint32_t)claim < total ? (uint32_t)claim : total;
        if (lane == 0) pick[2] = want;
      }
      uint32_t below = incl - (c0 + c1 + c2 + c3);
      if (want > below && want <= incl) {  // (one lane)
        uint32_t bin = 4 * lane;
        if (want > below + c0) {
          below += c0, ++bin;
          if (want > below + c1) {
            below += c1, ++bin;
            if (want > below + c2) below += c2, ++bin;
          }
        }
        pick[0] = bin;
        pick[1] = want - below;
      }
    }
    __syncthreads();
    take = pick[2];
    if (take == 0) break;  // (uniform) no row may be taken
    prefix |= pick[0] << shift;
    mask |= 255u << shift;
    k = pick[1];
  }
  // `prefix` is the take-th smallest stamp; k of the rows that carry it are wanted, and every row below it
  if (take > 0) {
    const uint32_t n_below = take - k;
    for (int32_t j = 0; j < sweeps; ++j) {
      const int32_t r = 2 + j * SELECT_THREADS + tid;
      const uint32_t st = r < capacity ? (uint32_t)row_stamp[r] : 0u;
      const bool cand = r < capacity && st != (uint32_t)epoch;
      const bool lo = cand && st < prefix, eq = cand && st == prefix;
      const uint64_t ml = __ballot(lo), me = __ballot(eq);
      const uint64_t before = ((uint64_t)1 << lane) - 1;
      if (ml) {
        const int leader = __ffsll((unsigned long long)ml) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&found[0], (uint32_t)__popcll(ml));
        base = (uint32_t)__shfl((int)base, leader);
        const uint32_t at = base + (uint32_t)__popcll(ml & before);
        if (lo && at < n_below) victims[at] = r;
      }
      if (me) {
        const int leader = __ffsll((unsigned long long)me) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&found[1], (uint32_t)__popcll(me));
        base = (uint32_t)__shfl((int)base, leader);
        const uint32_t at = base + (uint32_t)__popcll(me & before);
        if (eq && at < k) victims[n_below + at] = r;
      }
    }
    __syncthreads();  // (the list is read back by other waves of this workgroup: one CU, one L1)
  }
  // reassign: claimant j takes victims[j]; the claimants beyond the rows taken stay without one
  for (int32_t j = tid; j < claim; j += SELECT_THREADS) {
    const int32_t s = claimants[j];
    if (s < 0 || s >= n_states) continue;
    const int32_t v = j < (int32_t)take ? victims[j] : -1;
    if (v < 2 || v >= capacity) {
      row_of_state[s] = -1;
      continue;
    }
    const int32_t old = row_state[v];
    if (old >= 0 && old < n_states) {
      row_of_state[old] = -1;
      atomicAdd(&found[2], 1u);
    }
    row_state[v] = s;
    row_of_state[s] = v;
    row_stamp[v] = epoch;
    work[2 * (int64_t)j] = s;
    work[2 * (int64_t)j + 1] = v;
  }
  __syncthreads();
  if (tid == 0) {
    const int32_t evicted = (int32_t)found[2];
    ecounters[E_TAKEN] = (int32_t)take;
    ecounters[E_FILLS] += (int32_t)take;
    ecounters[E_EVICTIONS] += evicted;
    counters[C_ROWS] += (int32_t)take - evicted;
    if ((int32_t)take < claim) atomicOr(&counters[C_OVERFLOW], 1);
  }
}

}  // namespace
