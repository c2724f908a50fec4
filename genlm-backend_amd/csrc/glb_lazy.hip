// glb_lazy.hip — a byte NFA served as a constraint, its subset states made when a particle reaches them (include/glb.h:
// glb_lazy_*).  A state is a set of important NFA states, W 64-bit words: a wave holds one, a lane a word
// (glb_set.hpp, shared with glb_nfa_det.hip).  glb_lazy_advance walks every particle's tokens from its state's set, byte by
// byte, in registers; only the set a particle ends in is looked up and numbered, by glb_number.hpp's kernels: enter (a wave per
// particle), count, scan, number and resolve, over this file's `Lazy`, whose store_row copies the set and derives its
// accepting bit.  The bank of rows is glb_dfa_bank.hpp's, unchanged: only the fill is new - it walks every token from sets[s]
// where glb_dfa.hip follows delta.  Everything read from device memory is range-checked.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/glb.h"
#include "glb_common.hpp"
#include "glb_dfa_bank.hpp"
#include "glb_number.hpp"
#include "glb_set.hpp"

namespace {

constexpr int LAZY_THREADS = NUMBER_THREADS;  // the walk: four waves, a particle each, as number_enter_wave_kernel has them
constexpr int LAZY_WAVES = NUMBER_WAVES;
constexpr int32_t LAZY_MAX_NFA_STATES = 1 << 24;

struct Lazy {
  const uint8_t *bytes;
  int64_t n_bytes;
  const int32_t *ptr;
  const uint8_t *skip;
  int64_t vocab;
  int32_t eos_id;
  int32_t n_nfa, n_imp, W, n_arcs, max_states;
  const int32_t *arc_off, *arc_dst;
  const uint64_t *arc_bytes, *acc_mask, *eclose;
  uint64_t hash_mask;
  unsigned long long *words;  // [slots]; 0: empty
  int32_t *partmin;           // [slots]; the smallest particle index of the chunk that brought the slot's set
  uint64_t mask;              // slots - 1
  uint64_t *cand, *rows;      // rows [max_states][W]: the numbered sets
  uint8_t *accepting_out;
  int32_t *cnt, *status;
  static __device__ void store_row(const Lazy &p, int64_t id, int64_t base, int64_t k);
};

// whether arc a reads `byte`, and then its target where that is a state of the automaton (else -1)
__device__ inline int32_t arc_target(const Lazy &p, int32_t a, int byte) {
  if (!((p.arc_bytes[4 * (int64_t)a + (byte >> 6)] >> (byte & 63)) & 1ull)) return -1;
  const int32_t d = p.arc_dst[a];
  return d >= 0 && d < p.n_nfa ? d : -1;
}

// ---- a set across the lanes of a wave ----------------------------------------------------------------------------------------
// step(set, byte) of include/glb.h: over the words that hold a member, the members by bit scan, each member's arcs; the loops
// are the wave's (every lane sees the same word), the OR a lane's
__device__ inline uint64_t wave_step(const Lazy &p, uint64_t mine, int byte, int lane) {
  uint64_t target = 0;
  uint64_t some = __ballot(mine != 0);
  while (some) {
    const int w = __ffsll((unsigned long long)some) - 1;
    some &= some - 1;
    uint64_t word = bcast64(mine, w);
    while (word) {
      const int32_t m = w * 64 + __ffsll((unsigned long long)word) - 1;
      word &= word - 1;
      if (m >= p.n_imp) break;
      const int32_t a0 = p.arc_off[m], a1 = p.arc_off[m + 1];
      if (a0 < 0 || a1 > p.n_arcs) continue;
      for (int32_t a = a0; a < a1; ++a) {
        const int32_t d = arc_target(p, a, byte);
        if (d >= 0 && lane < p.W) target |= p.eclose[(int64_t)d * p.W + lane];
      }
    }
  }
  return target;
}

// next(set, t): t is the wave's; empty as soon as the set is
__device__ inline uint64_t wave_token(const Lazy &p, uint64_t set, int64_t t, int lane) {
  if (t < 0 || t >= p.vocab || p.skip[t]) return 0;
  const int64_t p0 = p.ptr[t], p1 = p.ptr[t + 1];
  if (p0 < 0 || p1 <= p0 || p1 > p.n_bytes) return 0;  // an empty token, or offsets that are not the vocabulary's
  for (int64_t q = p0; q < p1; ++q) {
    set = wave_step(p, set, p.bytes[q], lane);
    if (!__any(set != 0)) return 0;
  }
  return set;
}

// ---- a set of one word in a lane's register (W == 1) ------------------------------------------------------------------------------
__device__ inline uint64_t lane_token(const Lazy &p, uint64_t set, int64_t t) {
  if (t < 0 || t >= p.vocab || p.skip[t]) return 0;
  const int64_t p0 = p.ptr[t], p1 = p.ptr[t + 1];
  if (p0 < 0 || p1 <= p0 || p1 > p.n_bytes) return 0;
  for (int64_t q = p0; q < p1 && set; ++q) {
    const int byte = p.bytes[q];
    uint64_t word = set, target = 0;
    while (word) {
      const int32_t m = __ffsll((unsigned long long)word) - 1;
      word &= word - 1;
      if (m >= p.n_imp) break;
      const int32_t a0 = p.arc_off[m], a1 = p.arc_off[m + 1];
      if (a0 < 0 || a1 > p.n_arcs) continue;
      for (int32_t a = a0; a < a1; ++a) {
        const int32_t d = arc_target(p, a, byte);
        if (d >= 0) target |= p.eclose[d];
      }
    }
    set = target;
  }
  return set;
}

// ---- init ------------------------------------------------------------------------------------------------------------------------
__global__ void lazy_clear_kernel(Lazy p) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < GLB_LAZY_STATUS) p.status[i] = 0;
  if (i < (uint64_t)p.max_states) p.accepting_out[i] = 0;
  if (i <= p.mask) {
    p.words[i] = 0;
    p.partmin[i] = NO_PART;
  }
}

// state 0: the closure of the start, one wave; an empty set stays out of the table (no particle is ever looked up with one)
__global__ __launch_bounds__(64) void lazy_seed_kernel(Lazy p, int32_t start) {
  const int lane = (int)threadIdx.x;
  const uint64_t word = lane < p.W ? p.eclose[(int64_t)start * p.W + lane] : 0ull;
  if (lane < p.W) p.rows[lane] = word;
  const bool acc = __any(lane < p.W && (word & p.acc_mask[lane < p.W ? lane : 0]) != 0), some = __any(word != 0);
  uint64_t slot;
  uint32_t high;
  set_key(p.hash_mask, p.mask, word, lane, slot, high);
  if (lane == 0) {
    p.accepting_out[0] = acc ? 1 : 0;
    if (some) p.words[slot] = (unsigned long long)high << 32;  // (id 0; the table is empty)
    p.status[N_COUNT] = p.status[N_BASE] = p.status[N_NEXT] = 1;
  }
}

// ---- advance: six launches over the particles [base, base + n) of a call, particle base + k owning row k of `cand`: the walk,
// then the five of glb_number.hpp
// walk, a wave per particle: the tokens of its range from its state's set, in registers; state_out = -1 (dead), the state
// itself (an empty range) or PENDING with the end set in `cand`
__global__ __launch_bounds__(LAZY_THREADS) void lazy_walk_kernel(Lazy p, int64_t base, int64_t n, const int32_t *tokens, int64_t ld,
                                                                const int32_t *from, const int32_t *to, const int32_t *state_in,
                                                                int32_t *state_out) {
  const int lane = (int)threadIdx.x & 63;
  const int32_t known = numbered(p, N_BASE);
  const int64_t waves = (int64_t)gridDim.x * LAZY_WAVES;
  for (int64_t k = (int64_t)blockIdx.x * LAZY_WAVES + (threadIdx.x >> 6); k < n; k += waves) {
    const int64_t i = base + k;
    const int32_t s = state_in ? state_in[i] : 0;
    const int64_t f = from[i], t = to[i];
    int32_t code = -1;
    if (s >= 0 && s < known && f >= 0 && t <= ld && f <= t) {  // (a whole wave)
      if (f == t) {
        code = s;
      } else {
        uint64_t set = lane < p.W ? p.rows[(int64_t)s * p.W + lane] : 0ull;
        bool alive = __any(set != 0);
        for (int64_t j = f; j < t && alive; ++j) {
          set = wave_token(p, set, tokens[i * ld + j], lane);
          alive = __any(set != 0);
        }
        if (alive) {
          if (lane < p.W) p.cand[k * p.W + lane] = set;
          code = PENDING;
        }
      }
    }
    if (lane == 0) state_out[i] = code;
  }
}

// the set of a winner (glb_number.hpp, number_kernel) copied from `cand`, and its accepting bit
__device__ inline void Lazy::store_row(const Lazy &p, int64_t id, int64_t, int64_t k) {
  const uint64_t *row = p.cand + k * p.W;
  bool acc = false;
  for (int j = 0; j < p.W; ++j) {
    const uint64_t word = row[j];
    p.rows[id * p.W + j] = word;
    acc = acc || (word & p.acc_mask[j]) != 0;
  }
  p.accepting_out[id] = acc ? 1 : 0;
}

// ---- the fill: the rows of the work entries, every token walked from sets[s] ----------------------------------------------------
// A work entry whose state is an id that no set has been given (a caller named it; `advance` never does): the claim is taken
// back - the ids launch behind the fill then serves row 0, the empty mask, which is that id's row today - and the row,
// under eviction, is nobody's.  One thread an entry
__device__ inline void unclaim(int32_t *row_of_state, int32_t *row_state, int32_t s, int32_t r) {
  row_of_state[s] = -1;
  if (row_state) row_state[r] = -1;
}

// W == 1, the shape of glb_dfa.hip's fill: a lane a token, the set in its register, 64 tokens one ballot, two words a wave
template <bool EVICT>
__global__ __launch_bounds__(FILL_THREADS) void lazy_fill_lane_kernel(Lazy p, int32_t *bank, int64_t bank_ld, int32_t capacity,
                                                                     const int32_t *work, const int32_t *counters,
                                                                     int32_t *row_of_state, int32_t *row_state) {
  __shared__ int32_t range[2];
  if (threadIdx.x == 0) fill_range<EVICT>(counters, capacity, range);
  __syncthreads();
  const int64_t words = (p.vocab + 31) / 32;
  const int64_t t = (int64_t)blockIdx.x * FILL_THREADS + threadIdx.x;
  const int64_t w0 = (t >> 6) * 2;
  if (w0 >= words) return;  // (a whole wave past the last word: the ballot wants every lane of the others)
  const int32_t known = numbered(p, N_COUNT);
  for (int32_t e = range[0] + (int32_t)blockIdx.y; e < range[1]; e += (int32_t)gridDim.y) {
    const int32_t s = work[2 * (int64_t)e], r = work[2 * (int64_t)e + 1];
    if (s < 0 || s >= p.max_states || r < 2 || r >= capacity) continue;  // (uniform over the block)
    if (s >= known) {  // an id no set has yet: it keeps no row, so that the set that takes the id later gets its own
      if (blockIdx.x == 0 && threadIdx.x == 0) unclaim(row_of_state, row_state, s, r);
      continue;
    }
    const uint64_t set = p.rows[s];
    bool bit = false;
    if (t < p.vocab) bit = t == p.eos_id ? p.accepting_out[s] != 0 : lane_token(p, set, t) != 0;
    const uint64_t b = __ballot(bit);
    if ((threadIdx.x & 63) == 0) {
      int32_t *row = bank + (int64_t)r * bank_ld;
      row[w0] = (int32_t)(uint32_t)b;
      if (w0 + 1 < words) row[w0 + 1] = (int32_t)(uint32_t)(b >> 32);
    }
  }
}

// any W: a wave a token, the set across its lanes.  A workgroup owns one word of the row: its four waves walk eight of the
// word's 32 tokens each, the bits meet in LDS and one thread writes the word - no atomic, no row zeroed first
template <bool EVICT>
__global__ __launch_bounds__(FILL_THREADS) void lazy_fill_wave_kernel(Lazy p, int32_t *bank, int64_t bank_ld, int32_t capacity,
                                                                     const int32_t *work, const int32_t *counters,
                                                                     int32_t *row_of_state, int32_t *row_state) {
  __shared__ int32_t range[2];
  __shared__ uint32_t part[FILL_THREADS / 64];
  if (threadIdx.x == 0) fill_range<EVICT>(counters, capacity, range);
  __syncthreads();
  const int64_t words = (p.vocab + 31) / 32;
  const int64_t wi = blockIdx.x;
  if (wi >= words) return;  // (uniform)
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int32_t known = numbered(p, N_COUNT);
  for (int32_t e = range[0] + (int32_t)blockIdx.y; e < range[1]; e += (int32_t)gridDim.y) {
    const int32_t s = work[2 * (int64_t)e], r = work[2 * (int64_t)e + 1];
    if (s < 0 || s >= p.max_states || r < 2 || r >= capacity) continue;  // (uniform over the block)
    if (s >= known) {
      if (blockIdx.x == 0 && threadIdx.x == 0) unclaim(row_of_state, row_state, s, r);
      continue;
    }
    const uint64_t set = lane < p.W ? p.rows[(int64_t)s * p.W + lane] : 0ull;
    const bool some = __any(set != 0);
    uint32_t bits = 0;
    for (int j = 0; j < 8; ++j) {
      const int64_t t = wi * 32 + wave * 8 + j;
      bool bit = false;
      if (t < p.vocab) bit = t == p.eos_id ? p.accepting_out[s] != 0 : some && __any(wave_token(p, set, t, lane) != 0);
      if (bit) bits |= 1u << (wave * 8 + j);
    }
    if (lane == 0) part[wave] = bits;
    __syncthreads();
    if (threadIdx.x == 0) bank[(int64_t)r * bank_ld + wi] = (int32_t)(part[0] | part[1] | part[2] | part[3]);
    __syncthreads();
  }
}

// ---- the host side -----------------------------------------------------------------------------------------------------------------
int lazy_check(const glb_lazy_args *a, const char *what, int need) {
  if (const int rc = number_check(a, what, "glb_lazy_args", need)) return rc;
  if (a->n_nfa_states < 1 || a->n_nfa_states > LAZY_MAX_NFA_STATES)
    return glb::api_fail(GLB_EINVAL, "%s: n_nfa_states %d outside [1, %d]", what, a->n_nfa_states, LAZY_MAX_NFA_STATES);
  if (a->n_important < 0 || a->n_important > GLB_NFA_MAX_IMPORTANT || a->n_important > a->n_nfa_states)
    return glb::api_fail(GLB_EINVAL, "%s: n_important %d outside [0, min(n_nfa_states, %d)]: a set is one wave, a 64-bit word a lane", what,
                         a->n_important, GLB_NFA_MAX_IMPORTANT);
  const int32_t W = a->n_important > 64 ? (a->n_important + 63) / 64 : 1;
  if (a->n_words != W) return glb::api_fail(GLB_EINVAL, "%s: n_words %d is not max(1, ceil(n_important / 64)) = %d", what, a->n_words, W);
  if (a->nfa_start < 0 || a->nfa_start >= a->n_nfa_states)
    return glb::api_fail(GLB_EINVAL, "%s: nfa_start %d outside [0, n_nfa_states = %d)", what, a->nfa_start, a->n_nfa_states);
  if (a->n_arcs < 0) return glb::api_fail(GLB_EINVAL, "%s: n_arcs %d is negative", what, a->n_arcs);
  if (!a->arc_off || !a->arc_dst || !a->arc_bytes) return glb::api_fail(GLB_EINVAL, "%s: arc_off, arc_dst or arc_bytes is null", what);
  if (!a->accepting_mask) return glb::api_fail(GLB_EINVAL, "%s: accepting_mask is null", what);
  if (!a->eclose) return glb::api_fail(GLB_EINVAL, "%s: eclose is null", what);
  if (!a->sets) return glb::api_fail(GLB_EINVAL, "%s: sets is null", what);
  if (!a->accepting_out) return glb::api_fail(GLB_EINVAL, "%s: accepting_out is null", what);
  return GLB_OK;
}

Lazy lazy_of(const glb_lazy_args *a) {
  const glb_dfa_args *d = &a->dfa;
  unsigned long long *words = (unsigned long long *)a->table;
  return Lazy{d->tok_bytes, d->n_bytes, d->tok_ptr, d->skip, d->vocab, d->eos_id, a->n_nfa_states, a->n_important, a->n_words, a->n_arcs,
              a->max_states, a->arc_off, a->arc_dst, a->arc_bytes, a->accepting_mask, a->eclose, a->hash_mask, words,
              (int32_t *)(words + a->table_slots), (uint64_t)a->table_slots - 1, a->cand, a->sets, a->accepting_out, a->counts, a->status};
}

}  // namespace

extern "C" {

int glb_lazy_init(const glb_lazy_args *a, void *stream) {
  if (const int rc = lazy_check(a, "glb_lazy_init", NEED_BANK)) return rc;
  const glb_dfa_args *d = &a->dfa;
  const hipStream_t st = (hipStream_t)stream;
  const Lazy p = lazy_of(a);
  const int64_t most = a->table_slots > a->max_states ? a->table_slots : a->max_states;
  hipLaunchKernelGGL(lazy_clear_kernel, dim3(blocks_for(most, 256)), dim3(256), 0, st, p);
  hipLaunchKernelGGL(lazy_seed_kernel, dim3(1), dim3(64), 0, st, p, a->nfa_start);
  const int64_t elems = (d->vocab + 31) / 32;
  hipLaunchKernelGGL(dfa_bank_init_kernel<int32_t>, dim3(blocks_for(elems > a->max_states ? elems : a->max_states, 256)), dim3(256), 0, st,
                     a->max_states, d->eos_id, d->vocab, d->bank, d->bank_ld, elems, d->row_of_state, d->counters);
  if (a->epoch)
    hipLaunchKernelGGL(dfa_evict_init_kernel, dim3(blocks_for(d->capacity, 256)), dim3(256), 0, st, (int32_t)d->capacity, a->row_state,
                       a->row_stamp, a->ecounters, a->epoch);
  return glb::launched("lazy_init launch");
}

int glb_lazy_advance(const glb_lazy_args *a, void *stream) {
  if (const int rc = lazy_check(a, "glb_lazy_advance", NEED_WALK | NEED_N)) return rc;
  const glb_dfa_args *d = &a->dfa;
  if (!d->tokens || !d->from || !d->to || !d->state_out || d->ld <= 0) return glb::api_fail(GLB_EINVAL, "glb_lazy_advance: null pointer or ld <= 0");
  if (!a->cand) return glb::api_fail(GLB_EINVAL, "glb_lazy_advance: cand is null");
  if (!a->counts) return glb::api_fail(GLB_EINVAL, "glb_lazy_advance: counts is null");
  if (a->cand_rows < 1 || a->cand_rows > a->table_slots - a->max_states)
    return glb::api_fail(GLB_EINVAL, "glb_lazy_advance: cand_rows %lld outside [1, table_slots - max_states = %lld]: the new sets of a chunk "
                         "must find free slots", (long long)a->cand_rows, (long long)(a->table_slots - a->max_states));
  const hipStream_t st = (hipStream_t)stream;
  const Lazy p = lazy_of(a);
  for (int64_t base = 0; base < d->n; base += a->cand_rows) {
    const int64_t n = d->n - base < a->cand_rows ? d->n - base : a->cand_rows;
    unsigned waves = 0, blocks = 0;
    if (const int rc = stride_grid("lazy: the device's CU count", &waves, n, LAZY_WAVES)) return rc;
    if (const int rc = stride_grid("lazy: the device's CU count", &blocks, n, LAZY_THREADS)) return rc;
    hipLaunchKernelGGL(lazy_walk_kernel, dim3(waves), dim3(LAZY_THREADS), 0, st, p, base, n, d->tokens, d->ld, d->from, d->to, d->state_in,
                       d->state_out);
    hipLaunchKernelGGL(number_enter_wave_kernel<Lazy>, dim3(waves), dim3(LAZY_THREADS), 0, st, p, base, n, d->state_out);
    number_launches(p, blocks, base, n, d->state_out, base + n >= d->n, st);
  }
  return glb::launched("lazy_advance launch");
}

int glb_lazy_serve(const glb_lazy_args *a, void *stream) {
  if (const int rc = lazy_check(a, "glb_lazy_serve", NEED_WALK | NEED_BANK | NEED_N)) return rc;
  const glb_dfa_args *d = &a->dfa;
  if (!d->state_in || !d->out_rows) return glb::api_fail(GLB_EINVAL, "glb_lazy_serve: null pointer");
  if (d->max_work <= 0) return glb::api_fail(GLB_EINVAL, "glb_lazy_serve: max_work %lld <= 0", (long long)d->max_work);
  const hipStream_t st = (hipStream_t)stream;
  const Lazy p = lazy_of(a);
  const int32_t capacity = (int32_t)d->capacity, S = a->max_states;
  const bool evict = a->epoch != nullptr, lanes = a->n_words == 1 && !a->force_wave;
  const unsigned entries = (unsigned)(d->max_work < FILL_MAX_ENTRIES ? d->max_work : FILL_MAX_ENTRIES);
  const dim3 fill(lanes ? blocks_for(d->vocab, FILL_THREADS) : blocks_for(d->vocab, 32), entries), by_n(blocks_for(d->n, 256));
  if (evict) {
    hipLaunchKernelGGL(dfa_evict_touch_kernel, by_n, dim3(256), 0, st, S, d->n, d->state_in, capacity, d->row_of_state, a->row_stamp,
                       a->claimants, d->counters, a->ecounters, a->epoch);
    hipLaunchKernelGGL(dfa_evict_select_kernel, dim3(1), dim3(SELECT_THREADS), 0, st, S, capacity, d->row_of_state, a->row_state,
                       a->row_stamp, a->claimants, a->victims, d->work, d->counters, a->ecounters, a->epoch);
    if (lanes)
      hipLaunchKernelGGL(lazy_fill_lane_kernel<true>, fill, dim3(FILL_THREADS), 0, st, p, d->bank, d->bank_ld, capacity, d->work, a->ecounters,
                         d->row_of_state, a->row_state);
    else
      hipLaunchKernelGGL(lazy_fill_wave_kernel<true>, fill, dim3(FILL_THREADS), 0, st, p, d->bank, d->bank_ld, capacity, d->work, a->ecounters,
                         d->row_of_state, a->row_state);
    hipLaunchKernelGGL(dfa_mask_ids_kernel, by_n, dim3(256), 0, st, S, (const uint8_t *)a->accepting_out, d->n, d->state_in, d->done,
                       d->row_of_state, capacity, d->out_rows, a->ecounters, a->epoch);
  } else {
    hipLaunchKernelGGL(dfa_claim_kernel, by_n, dim3(256), 0, st, S, d->n, d->state_in, capacity, d->row_of_state, d->work, d->counters);
    if (lanes)
      hipLaunchKernelGGL(lazy_fill_lane_kernel<false>, fill, dim3(FILL_THREADS), 0, st, p, d->bank, d->bank_ld, capacity, d->work, d->counters,
                         d->row_of_state, (int32_t *)nullptr);
    else
      hipLaunchKernelGGL(lazy_fill_wave_kernel<false>, fill, dim3(FILL_THREADS), 0, st, p, d->bank, d->bank_ld, capacity, d->work, d->counters,
                         d->row_of_state, (int32_t *)nullptr);
    hipLaunchKernelGGL(dfa_commit_kernel, dim3(1), dim3(1), 0, st, capacity, d->counters);
    hipLaunchKernelGGL(dfa_mask_ids_kernel, by_n, dim3(256), 0, st, S, (const uint8_t *)a->accepting_out, d->n, d->state_in, d->done,
                       d->row_of_state, capacity, d->out_rows, (int32_t *)nullptr, (int32_t *)nullptr);
  }
  return glb::launched("lazy_serve launch");
}

}  // extern "C"
