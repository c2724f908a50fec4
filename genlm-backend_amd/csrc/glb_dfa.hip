// glb_dfa.hip — byte-level DFA constraints on the device (include/glb.h: glb_dfa_*): automaton states advance
// token by token, every distinct state claims one row of a mask bank, and the rows are filled from the automaton - a wave
// per (state, 64 consecutive tokens), the 64 bits by one ballot.  Everything read from device memory is range-checked.
// Weighted automata (glb_dfa_weight_*, glb_dfa_fill_weights): the same walk summing float32 arc weights, the
// rows 64 consecutive floats a wave.  A bank smaller than the automaton (glb_dfa_evict_*): rows stamped with
// the call that last asked for them, the oldest selected by one workgroup and filled again by the same fill.  (Weight
// pushing, DESIGN.md §20: glb_dfa_push.hip; minimisation, §21: glb_dfa_min.hip.)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/glb.h"
#include "glb_common.hpp"

namespace {

enum { C_ROWS = 0, C_FILLED = 1, C_OVERFLOW = 2, C_RESERVED = 3 };
enum { E_CLAIMANTS = 0, E_TAKEN = 1, E_FILLS = 2, E_EVICTIONS = 3 };  // glb_dfa_evict_args.ecounters
constexpr int SELECT_THREADS = 1024;  // the selection's one workgroup
constexpr int FILL_THREADS = 256;    // four waves: 256 consecutive tokens of one state
constexpr int FILL_MAX_ENTRIES = 64; // grid.y: work entries served side by side (a block loops over the rest)

struct Dfa {
  const int32_t *delta;
  const uint8_t *accepting, *live;
  int32_t n_states, start, eos_id;
  const uint8_t *bytes;
  int64_t n_bytes;
  const int32_t *ptr;
  const uint8_t *skip;
  int64_t vocab;
};

// next(s, t) of include/glb.h; WEIGHTED: the weight of token t from state s instead - the float32 sum of the arcs' weights
// in byte order, -inf where next(s, t) is dead.  One walk, one set of checks; without weights no float is loaded or carried
template <bool WEIGHTED>
__device__ inline std::conditional_t<WEIGHTED, float, int32_t> dfa_walk(const Dfa &d, const float *arc_logw, int32_t s, int64_t t) {
  std::conditional_t<WEIGHTED, float, int32_t> dead = -1;
  if constexpr (WEIGHTED) dead = -__builtin_inff();
  if (s < 0 || s >= d.n_states || t < 0 || t >= d.vocab) return dead;
  if (d.skip[t]) return dead;
  const int64_t p0 = d.ptr[t], p1 = d.ptr[t + 1];
  if (p0 < 0 || p1 <= p0 || p1 > d.n_bytes) return dead;  // an empty token, or offsets that are not the vocabulary's
  int32_t cur = s;
  [[maybe_unused]] float w = 0.0f;
  for (int64_t p = p0; p < p1; ++p) {
    const int64_t arc = (int64_t)cur * 256 + d.bytes[p];
    if constexpr (WEIGHTED) w = w + arc_logw[arc];
    cur = d.delta[arc];
    if (cur < 0 || cur >= d.n_states) return dead;
  }
  if (!d.live[cur]) return dead;
  if constexpr (WEIGHTED) return w;
  else return cur;
}

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

__global__ void dfa_advance_kernel(Dfa d, int64_t n, const int32_t *tokens, int64_t ld, const int32_t *from, const int32_t *to,
                                   const int32_t *state_in, int32_t *state_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int32_t cur = state_in ? state_in[i] : d.start;
  if (cur < 0 || cur >= d.n_states) cur = -1;
  const int64_t f = from[i], t = to[i];
  if (f < 0 || t > ld || f > t) cur = -1;
  for (int64_t j = f; j < t && cur >= 0; ++j) cur = dfa_walk<false>(d, nullptr, cur, tokens[i * ld + j]);
  state_out[i] = cur;
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

// A wave per (work entry, 64 consecutive tokens), a workgroup looping over the entries it owns.  Bit rows: lane 0 writes the
// wave's two words from one ballot; float rows (WEIGHTED): a lane keeps its token's sum and the wave stores 64 consecutive
// floats (256 bytes), no ballot
template <bool WEIGHTED>
__device__ inline void dfa_fill_entries(const Dfa &d, const float *arc_logw, const float *final_logw,
                                        std::conditional_t<WEIGHTED, float, int32_t> *bank, int64_t bank_ld, int32_t capacity,
                                        const int32_t *work, int32_t begin, int32_t end) {
  const int64_t words = (d.vocab + 31) / 32;
  const int64_t t = (int64_t)blockIdx.x * FILL_THREADS + threadIdx.x;  // (a wave: 64 consecutive tokens, two words)
  const int64_t w0 = (t >> 6) * 2;
  // who leaves: a float lane past the vocabulary (no barrier and no cross-lane operation below), but of the bit rows only a
  // whole wave past the last word - the ballot wants every lane of the others
  if (WEIGHTED ? t >= d.vocab : w0 >= words) return;
  for (int32_t e = begin + (int32_t)blockIdx.y; e < end; e += (int32_t)gridDim.y) {
    const int32_t s = work[2 * (int64_t)e], r = work[2 * (int64_t)e + 1];
    if (s < 0 || s >= d.n_states || r < 2 || r >= capacity) continue;  // (uniform over the block)
    if constexpr (WEIGHTED) {
      bank[(int64_t)r * bank_ld + t] = t == d.eos_id ? final_logw[s] : dfa_walk<true>(d, arc_logw, s, t);
    } else {
      bool bit = false;
      if (t < d.vocab) bit = t == d.eos_id ? d.accepting[s] != 0 : dfa_walk<false>(d, nullptr, s, t) >= 0;
      const uint64_t b = __ballot(bit);
      if ((threadIdx.x & 63) == 0) {
        int32_t *row = bank + (int64_t)r * bank_ld;
        row[w0] = (int32_t)(uint32_t)b;
        if (w0 + 1 < words) row[w0 + 1] = (int32_t)(uint32_t)(b >> 32);
      }
    }
  }
}

// The entries of the work list to fill, read by thread 0 from `counters`: the claim path's [counters[C_FILLED],
// counters[C_ROWS] - 2); EVICT (`counters` the block's ecounters): a serve call's [0, ecounters[E_TAKEN])
template <bool WEIGHTED, bool EVICT>
__global__ __launch_bounds__(FILL_THREADS) void dfa_fill_kernel(Dfa d, const float *arc_logw, const float *final_logw,
                                                               std::conditional_t<WEIGHTED, float, int32_t> *bank,
                                                               int64_t bank_ld, int32_t capacity, const int32_t *work,
                                                               const int32_t *counters) {
  __shared__ int32_t range[2];
  if (threadIdx.x == 0) {
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
  __syncthreads();
  dfa_fill_entries<WEIGHTED>(d, arc_logw, final_logw, bank, bank_ld, capacity, work, range[0], range[1]);
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

// NEED_ROWS: the bank's bookkeeping (capacity, row_of_state, work, counters) without its bit rows - a weight bank's calls
constexpr int NEED_VOCAB = 1, NEED_BANK = 2, NEED_N = 4, NEED_ROWS = 8;

int dfa_check(const glb_dfa_args *a, const char *what, int need) {
  if (const int rc = glb::block_ok(a, what, "glb_dfa_args")) return rc;
  if (a->n_states <= 0) return glb::api_fail(GLB_EINVAL, "%s: n_states %d <= 0", what, a->n_states);
  if (a->start < 0 || a->start >= a->n_states)
    return glb::api_fail(GLB_EINVAL, "%s: start %d outside [0, %d)", what, a->start, a->n_states);
  if (a->vocab <= 0 || a->vocab > 0x7fffff00ll) return glb::api_fail(GLB_EINVAL, "%s: vocab %lld", what, (long long)a->vocab);
  if (need & (NEED_BANK | NEED_ROWS)) {
    if ((need & NEED_BANK) && a->bank_ld < (a->vocab + 31) / 32)
      return glb::api_fail(GLB_EINVAL, "%s: bank_ld %lld < %lld words", what, (long long)a->bank_ld, (long long)((a->vocab + 31) / 32));
    if (a->capacity < 2 || a->capacity > 0x7fffffffll)
      return glb::api_fail(GLB_EINVAL, "%s: capacity %lld (rows 0 and 1 are the bank's own)", what, (long long)a->capacity);
    if (((need & NEED_BANK) && !a->bank) || !a->row_of_state || !a->work || !a->counters) return glb::api_fail(GLB_EINVAL, "%s: null bank pointer", what);
  }
  if (!a->delta || !a->accepting || !a->live) return glb::api_fail(GLB_EINVAL, "%s: null automaton pointer", what);
  if (need & NEED_VOCAB) {
    if (!a->tok_bytes || !a->tok_ptr || !a->skip || a->n_bytes < 0 || a->n_bytes > 0x7fffffffll)
      return glb::api_fail(GLB_EINVAL, "%s: vocabulary bytes missing", what);
  }
  if (need & NEED_N) {
    if (a->n <= 0) return glb::api_fail(GLB_EINVAL, "%s: n %lld <= 0", what, (long long)a->n);
  }
  return GLB_OK;
}

Dfa dfa_of(const glb_dfa_args *a) {
  return Dfa{a->delta, a->accepting, a->live, a->n_states, a->start, a->eos_id, a->tok_bytes, a->n_bytes, a->tok_ptr, a->skip, a->vocab};
}

// a float bank and the weights it is filled from, of either block that carries them
int float_bank_check(const float *arc_logw, const float *final_logw, const float *wbank, int64_t wbank_ld, int64_t vocab, const char *what) {
  if (!wbank || !arc_logw || !final_logw) return glb::api_fail(GLB_EINVAL, "%s: null weight table", what);
  if (wbank_ld < vocab) return glb::api_fail(GLB_EINVAL, "%s: wbank_ld %lld < vocab %lld", what, (long long)wbank_ld, (long long)vocab);
  return GLB_OK;
}

int dfa_weight_check(const glb_dfa_weight_args *w, const char *what, int need) {
  if (const int rc = glb::block_ok(w, what, "glb_dfa_weight_args")) return rc;
  if (const int rc = dfa_check(&w->dfa, what, need | NEED_ROWS)) return rc;
  return float_bank_check(w->arc_logw, w->final_logw, w->wbank, w->wbank_ld, w->dfa.vocab, what);
}

// an evicting bank's block: the embedded block's checks (a bit bank's `bank` only where there is no float bank), then its own
int dfa_evict_check(const glb_dfa_evict_args *e, const char *what, int need) {
  if (const int rc = glb::block_ok(e, what, "glb_dfa_evict_args")) return rc;
  const bool weighted = e->wbank || e->arc_logw || e->final_logw;
  if (const int rc = dfa_check(&e->dfa, what, need | (weighted ? NEED_ROWS : NEED_BANK))) return rc;
  if (e->dfa.capacity < 3 || e->dfa.capacity > 65535)
    return glb::api_fail(GLB_EINVAL, "%s: capacity %lld outside [3, 65535]", what, (long long)e->dfa.capacity);
  if (weighted)
    if (const int rc = float_bank_check(e->arc_logw, e->final_logw, e->wbank, e->wbank_ld, e->dfa.vocab, what)) return rc;
  if (!e->row_state || !e->row_stamp || !e->claimants || !e->victims || !e->ecounters || !e->epoch)
    return glb::api_fail(GLB_EINVAL, "%s: null eviction table", what);
  return GLB_OK;
}

// rows a bank of `bank_bytes` holds when one takes `row_bytes`: at most a row per state and the bank's own two
int64_t bank_rows(size_t bank_bytes, size_t row_bytes, int64_t vocab, int64_t n_states) {
  if (vocab <= 0 || n_states <= 0) return 0;
  int64_t rows = (int64_t)(bank_bytes / row_bytes);
  if (rows > n_states + 2) rows = n_states + 2;
  return rows > 65535 ? 65535 : rows;
}

// rows 0 and 1 of a block's bank (bit words, or with T = float the floats of `elems` tokens), and no state with a row
template <typename T>
void bank_init(const glb_dfa_args *a, T *bank, int64_t ld, int64_t elems, hipStream_t st) {
  hipLaunchKernelGGL(dfa_bank_init_kernel<T>, dim3(blocks_for(elems > a->n_states ? elems : a->n_states, 256)), dim3(256), 0, st,
                     a->n_states, a->eos_id, a->vocab, bank, ld, elems, a->row_of_state, a->counters);
}

// the fill's grid: 256 tokens a block, at most FILL_MAX_ENTRIES work entries side by side
dim3 fill_grid(const glb_dfa_args *a) {
  return dim3(blocks_for(a->vocab, FILL_THREADS), (unsigned)(a->max_work < FILL_MAX_ENTRIES ? a->max_work : FILL_MAX_ENTRIES));
}

// the claimed rows filled (bit words, or with weights floats), then the filled mark moved up
template <bool WEIGHTED, typename T>
int fill_and_commit(const glb_dfa_args *a, const char *what, const char *launch, const float *arc_logw, const float *final_logw,
                    T *bank, int64_t bank_ld, void *stream) {
  if (a->max_work <= 0) return glb::api_fail(GLB_EINVAL, "%s: max_work %lld <= 0", what, (long long)a->max_work);
  hipLaunchKernelGGL((dfa_fill_kernel<WEIGHTED, false>), fill_grid(a), dim3(FILL_THREADS), 0, (hipStream_t)stream, dfa_of(a), arc_logw,
                     final_logw, bank, bank_ld, (int32_t)a->capacity, a->work, a->counters);
  hipLaunchKernelGGL(dfa_commit_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (int32_t)a->capacity, a->counters);
  return glb::launched(launch);
}

}  // namespace

extern "C" {

int64_t glb_dfa_bank_rows(size_t bank_bytes, int64_t vocab, int64_t n_states) {
  return bank_rows(bank_bytes, (size_t)((vocab + 31) / 32) * sizeof(int32_t), vocab, n_states);
}

int glb_dfa_bank_init(const glb_dfa_args *a, void *stream) {
  if (const int rc = dfa_check(a, "glb_dfa_bank_init", NEED_BANK)) return rc;
  bank_init(a, a->bank, a->bank_ld, (a->vocab + 31) / 32, (hipStream_t)stream);
  return glb::launched("dfa_bank_init launch");
}

int glb_dfa_advance(const glb_dfa_args *a, void *stream) {
  if (const int rc = dfa_check(a, "glb_dfa_advance", NEED_VOCAB | NEED_N)) return rc;
  if (!a->tokens || !a->from || !a->to || !a->state_out || a->ld <= 0) return glb::api_fail(GLB_EINVAL, "glb_dfa_advance: null pointer or ld <= 0");
  hipLaunchKernelGGL(dfa_advance_kernel, dim3(blocks_for(a->n, 128)), dim3(128), 0, (hipStream_t)stream, dfa_of(a), a->n, a->tokens,
                     a->ld, a->from, a->to, a->state_in, a->state_out);
  return glb::launched("dfa_advance launch");
}

int glb_dfa_claim_rows(const glb_dfa_args *a, void *stream) {
  if (const int rc = dfa_check(a, "glb_dfa_claim_rows", NEED_BANK | NEED_N)) return rc;
  if (!a->state_in) return glb::api_fail(GLB_EINVAL, "glb_dfa_claim_rows: state_in is null");
  hipLaunchKernelGGL(dfa_claim_kernel, dim3(blocks_for(a->n, 256)), dim3(256), 0, (hipStream_t)stream, a->n_states, a->n, a->state_in,
                     (int32_t)a->capacity, a->row_of_state, a->work, a->counters);
  return glb::launched("dfa_claim launch");
}

int glb_dfa_fill_masks(const glb_dfa_args *a, void *stream) {
  if (const int rc = dfa_check(a, "glb_dfa_fill_masks", NEED_BANK | NEED_VOCAB)) return rc;
  return fill_and_commit<false>(a, "glb_dfa_fill_masks", "dfa_fill launch", nullptr, nullptr, a->bank, a->bank_ld, stream);
}

int glb_dfa_mask_ids(const glb_dfa_args *a, void *stream) {
  if (const int rc = dfa_check(a, "glb_dfa_mask_ids", NEED_BANK | NEED_N)) return rc;
  if (!a->state_in || !a->out_rows) return glb::api_fail(GLB_EINVAL, "glb_dfa_mask_ids: null pointer");
  hipLaunchKernelGGL(dfa_mask_ids_kernel, dim3(blocks_for(a->n, 256)), dim3(256), 0, (hipStream_t)stream, a->n_states, a->accepting,
                     a->n, a->state_in, a->done, a->row_of_state, (int32_t)a->capacity, a->out_rows, (int32_t *)nullptr,
                     (int32_t *)nullptr);
  return glb::launched("dfa_mask_ids launch");
}

int64_t glb_dfa_weight_bank_rows(size_t bank_bytes, int64_t vocab, int64_t n_states) {
  return bank_rows(bank_bytes, (size_t)((vocab + 63) / 64) * 64 * sizeof(float), vocab, n_states);
}

int glb_dfa_weight_bank_init(const glb_dfa_weight_args *w, void *stream) {
  if (const int rc = dfa_weight_check(w, "glb_dfa_weight_bank_init", 0)) return rc;
  bank_init(&w->dfa, w->wbank, w->wbank_ld, w->dfa.vocab, (hipStream_t)stream);
  return glb::launched("dfa_weight_bank_init launch");
}

int glb_dfa_fill_weights(const glb_dfa_weight_args *w, void *stream) {
  if (const int rc = dfa_weight_check(w, "glb_dfa_fill_weights", NEED_VOCAB)) return rc;
  return fill_and_commit<true>(&w->dfa, "glb_dfa_fill_weights", "dfa_fill_weights launch", w->arc_logw, w->final_logw, w->wbank,
                               w->wbank_ld, stream);
}

int glb_dfa_evict_bank_init(const glb_dfa_evict_args *e, void *stream) {
  if (const int rc = dfa_evict_check(e, "glb_dfa_evict_bank_init", 0)) return rc;
  const glb_dfa_args *a = &e->dfa;
  if (e->wbank) bank_init(a, e->wbank, e->wbank_ld, a->vocab, (hipStream_t)stream);
  else bank_init(a, a->bank, a->bank_ld, (a->vocab + 31) / 32, (hipStream_t)stream);
  hipLaunchKernelGGL(dfa_evict_init_kernel, dim3(blocks_for(a->capacity, 256)), dim3(256), 0, (hipStream_t)stream, (int32_t)a->capacity,
                     e->row_state, e->row_stamp, e->ecounters, e->epoch);
  return glb::launched("dfa_evict_bank_init launch");
}

int glb_dfa_evict_serve(const glb_dfa_evict_args *e, void *stream) {
  if (const int rc = dfa_evict_check(e, "glb_dfa_evict_serve", NEED_VOCAB | NEED_N)) return rc;
  const glb_dfa_args *a = &e->dfa;
  if (!a->state_in || !a->out_rows) return glb::api_fail(GLB_EINVAL, "glb_dfa_evict_serve: null pointer");
  if (a->max_work <= 0) return glb::api_fail(GLB_EINVAL, "glb_dfa_evict_serve: max_work %lld <= 0", (long long)a->max_work);
  const hipStream_t st = (hipStream_t)stream;
  const int32_t capacity = (int32_t)a->capacity;
  hipLaunchKernelGGL(dfa_evict_touch_kernel, dim3(blocks_for(a->n, 256)), dim3(256), 0, st, a->n_states, a->n, a->state_in, capacity,
                     a->row_of_state, e->row_stamp, e->claimants, a->counters, e->ecounters, e->epoch);
  hipLaunchKernelGGL(dfa_evict_select_kernel, dim3(1), dim3(SELECT_THREADS), 0, st, a->n_states, capacity, a->row_of_state,
                     e->row_state, e->row_stamp, e->claimants, e->victims, a->work, a->counters, e->ecounters, e->epoch);
  if (e->wbank)
    hipLaunchKernelGGL((dfa_fill_kernel<true, true>), fill_grid(a), dim3(FILL_THREADS), 0, st, dfa_of(a), e->arc_logw, e->final_logw,
                       e->wbank, e->wbank_ld, capacity, a->work, e->ecounters);
  else
    hipLaunchKernelGGL((dfa_fill_kernel<false, true>), fill_grid(a), dim3(FILL_THREADS), 0, st, dfa_of(a), nullptr, nullptr, a->bank,
                       a->bank_ld, capacity, a->work, e->ecounters);
  hipLaunchKernelGGL(dfa_mask_ids_kernel, dim3(blocks_for(a->n, 256)), dim3(256), 0, st, a->n_states, a->accepting, a->n, a->state_in,
                     a->done, a->row_of_state, capacity, a->out_rows, e->ecounters, e->epoch);
  return glb::launched("dfa_evict_serve launch");
}

}  // extern "C"
