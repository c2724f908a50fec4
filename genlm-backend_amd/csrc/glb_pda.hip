// glb_pda.hip — a real-time deterministic pushdown automaton over bytes served as a constraint (include/glb.h: glb_pda_*;
// DESIGN.md §25).  A state of the constraint is a configuration - the automaton's state and a bounded stack - of W 64-bit
// words: a wave holds one, a lane a word (glb_set.hpp's hash and key work on the raw words, every byte above the depth being
// zero).  glb_pda_advance walks every particle's tokens from its configuration, byte by byte, in registers; the configuration
// it ends in is looked up and numbered as glb_lazy.hip numbers a set, by glb_number.hpp's kernels: enter (a wave per
// particle), count, scan, number and resolve, over this file's `Pda`, whose store_row copies the configuration and derives
// its accepting byte.  The bank of rows is glb_dfa_bank.hpp's, unchanged: only the fill is new.  Everything read from device
// memory is range-checked.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/glb.h"
#include "glb_common.hpp"
#include "glb_dfa_bank.hpp"
#include "glb_number.hpp"
#include "glb_set.hpp"

namespace {

constexpr int PDA_THREADS = NUMBER_THREADS;  // the walk: four waves, a particle each, as number_enter_wave_kernel has them
constexpr int PDA_WAVES = NUMBER_WAVES;
constexpr int PDA_FILL_THREADS = 64;  // the fill: one wave a workgroup, 64 tokens, at most 64 x 504 bytes of private stacks
constexpr int32_t PDA_MAX_AUTOMATON = 1 << 24;
constexpr int32_t PDA_MAX_SYMBOLS = 126;
constexpr int PDA_POP = 127;

struct Pda {
  const uint8_t *bytes;
  int64_t n_bytes;
  const int32_t *ptr;
  const uint8_t *skip;
  int64_t vocab;
  int32_t eos_id;
  int32_t S, G, max_depth, W, max_states;
  const int32_t *delta;
  const uint8_t *accepting;
  uint64_t hash_mask;
  unsigned long long *words;  // [slots]; 0: empty
  int32_t *partmin;           // [slots]; the smallest particle index of the chunk that brought the slot's configuration
  uint64_t mask;              // slots - 1
  uint64_t *cand, *rows;      // rows [max_states][W]: the numbered configurations
  uint8_t *accepting_out;
  int32_t *cnt, *status;
  static __device__ void store_row(const Pda &p, int64_t id, int64_t base, int64_t k);
};

// word 0 of a configuration: whether its state and depth are the automaton's
__device__ inline bool head_ok(const Pda &p, uint64_t head, int32_t &state, int32_t &depth) {
  state = (int32_t)(uint32_t)head;
  depth = (int32_t)(uint32_t)(head >> 32);
  return state >= 0 && state < p.S && depth >= 0 && depth <= p.max_depth;
}

// delta[state, top, byte] taken apart (state is in [0, S)): false where the walk is dead - no entry, a top that is no
// symbol, a field out of range; op: 0 keep, 1 .. G push, PDA_POP
__device__ inline bool pda_entry(const Pda &p, int32_t state, int top, int byte, int32_t &next, int &op) {
  if (top > p.G) return false;
  const int32_t e = p.delta[((int64_t)state * (p.G + 1) + top) * 256 + byte];
  if (e < 0) return false;
  next = e & 0xffffff;
  op = e >> 24;  // (e >= 0: at most 127)
  return next < p.S && (op == 0 || op == PDA_POP || op <= p.G);
}

// whether token t can be walked at all, and then its bytes [p0, p1): the rules of glb_dfa_advance
__device__ inline bool token_bytes(const Pda &p, int64_t t, int64_t &p0, int64_t &p1) {
  if (t < 0 || t >= p.vocab || p.skip[t]) return false;
  p0 = p.ptr[t], p1 = p.ptr[t + 1];
  return p0 >= 0 && p1 > p0 && p1 <= p.n_bytes;  // (an empty token, or offsets that are not the vocabulary's)
}

// ---- a configuration across the lanes of a wave ----------------------------------------------------------------------------
// step(c, b) of include/glb.h: state and depth are the wave's, `mine` lane l's word (l >= 1: the symbols 8 (l - 1) ..); the
// top is one lane's word in every lane and a shift, a push or a pop a masked update in that one lane
__device__ inline bool wave_step(const Pda &p, int32_t &state, int32_t &depth, uint64_t &mine, int byte, int lane) {
  int top = 0;
  if (depth > 0) top = (int)((bcast64(mine, 1 + ((depth - 1) >> 3)) >> (8 * ((depth - 1) & 7))) & 0xffull);
  int32_t next;
  int op;
  if (!pda_entry(p, state, top, byte, next, op)) return false;
  if (op == PDA_POP) {
    if (depth == 0) return false;
    --depth;
    if (lane == 1 + (depth >> 3)) mine &= ~(0xffull << (8 * (depth & 7)));  // (every byte above the depth stays zero)
  } else if (op) {
    if (depth >= p.max_depth) return false;
    if (lane == 1 + (depth >> 3)) mine |= (uint64_t)op << (8 * (depth & 7));
    ++depth;
  }
  state = next;
  return true;
}

// next(c, t): t is the wave's
__device__ inline bool wave_token(const Pda &p, int32_t &state, int32_t &depth, uint64_t &mine, int64_t t, int lane) {
  int64_t p0, p1;
  if (!token_bytes(p, t, p0, p1)) return false;
  for (int64_t q = p0; q < p1; ++q)
    if (!wave_step(p, state, depth, mine, p.bytes[q], lane)) return false;
  return true;
}

// ---- a token in one lane, over the served configuration's stack in LDS (the fill) ----------------------------------------------
// `below`: how much of the shared stack `base` is still under the lane; `priv` [P][64]: what the lane pushed since, position
// by position, the lanes side by side.  A token may pop below where it began and push again: the pushes then lie on the
// `below` symbols that are left
__device__ inline bool lane_token(const Pda &p, int32_t P, int32_t state, int32_t below, const uint8_t *base, uint8_t *priv, int lane,
                                  int64_t t) {
  int64_t p0, p1;
  if (!token_bytes(p, t, p0, p1)) return false;
  int32_t mine = 0;
  for (int64_t q = p0; q < p1; ++q) {
    const int top = mine > 0 ? priv[(mine - 1) * 64 + lane] : below > 0 ? base[below - 1] : 0;
    int32_t next;
    int op;
    if (!pda_entry(p, state, top, p.bytes[q], next, op)) return false;
    if (op == PDA_POP) {
      if (mine > 0) --mine;
      else if (below > 0) --below;
      else return false;
    } else if (op) {
      if (below + mine >= p.max_depth || mine >= P) return false;  // (mine >= P: a token longer than max_token_bytes says)
      priv[mine * 64 + lane] = (uint8_t)op;
      ++mine;
    }
    state = next;
  }
  return true;
}

// ---- init ------------------------------------------------------------------------------------------------------------------------
__global__ void pda_clear_kernel(Pda p) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < GLB_PDA_STATUS) p.status[i] = 0;
  if (i < (uint64_t)p.max_states) p.accepting_out[i] = 0;
  if (i <= p.mask) {
    p.words[i] = 0;
    p.partmin[i] = NO_PART;
  }
}

// id 0: (start, the empty stack), one wave
__global__ __launch_bounds__(64) void pda_seed_kernel(Pda p, int32_t start) {
  const int lane = (int)threadIdx.x;
  const uint64_t word = lane == 0 ? (uint64_t)(uint32_t)start : 0ull;
  if (lane < p.W) p.rows[lane] = word;
  uint64_t slot;
  uint32_t high;
  set_key(p.hash_mask, p.mask, word, lane, slot, high);
  if (lane == 0) {
    p.accepting_out[0] = p.accepting[start] ? 1 : 0;
    p.words[slot] = (unsigned long long)high << 32;  // (id 0; the table is empty)
    p.status[N_COUNT] = p.status[N_BASE] = p.status[N_NEXT] = 1;
  }
}

// ---- advance: six launches over the particles [base, base + n) of a call, particle base + k owning row k of `cand`: the walk,
// then the five of glb_number.hpp
// walk, a wave per particle: the tokens of its range from its configuration, in registers; state_out = -1 (dead), the id
// itself (an empty range) or PENDING with the end configuration in `cand`
__global__ __launch_bounds__(PDA_THREADS) void pda_walk_kernel(Pda p, int64_t base, int64_t n, const int32_t *tokens, int64_t ld,
                                                              const int32_t *from, const int32_t *to, const int32_t *state_in,
                                                              int32_t *state_out) {
  const int lane = (int)threadIdx.x & 63;
  const int32_t known = numbered(p, N_BASE);
  const int64_t waves = (int64_t)gridDim.x * PDA_WAVES;
  for (int64_t k = (int64_t)blockIdx.x * PDA_WAVES + (threadIdx.x >> 6); k < n; k += waves) {
    const int64_t i = base + k;
    const int32_t s = state_in ? state_in[i] : 0;
    const int64_t f = from[i], t = to[i];
    int32_t code = -1;
    if (s >= 0 && s < known && f >= 0 && t <= ld && f <= t) {  // (a whole wave)
      if (f == t) {
        code = s;
      } else {
        const uint64_t word = lane < p.W ? p.rows[(int64_t)s * p.W + lane] : 0ull;
        int32_t state, depth;
        bool alive = head_ok(p, bcast64(word, 0), state, depth);
        uint64_t mine = lane == 0 ? 0ull : word;
        for (int64_t j = f; j < t && alive; ++j) alive = wave_token(p, state, depth, mine, tokens[i * ld + j], lane);
        if (alive) {
          if (lane == 0) mine = (uint64_t)(uint32_t)state | ((uint64_t)(uint32_t)depth << 32);
          if (lane < p.W) p.cand[k * p.W + lane] = mine;
          code = PENDING;
        }
      }
    }
    if (lane == 0) state_out[i] = code;
  }
}

// the configuration of a winner (glb_number.hpp, number_kernel) copied from `cand`; accepting_out = accepting[state] && depth == 0
__device__ inline void Pda::store_row(const Pda &p, int64_t id, int64_t, int64_t k) {
  const uint64_t *row = p.cand + k * p.W;
  for (int j = 0; j < p.W; ++j) p.rows[id * p.W + j] = row[j];
  int32_t state, depth;
  const bool ok = head_ok(p, row[0], state, depth);
  p.accepting_out[id] = ok && depth == 0 && p.accepting[state] ? 1 : 0;
}

// ---- the fill: the rows of the work entries, every token walked from configs[s] ------------------------------------------------
// A lane a token, a workgroup one wave: 64 tokens one ballot, two words of the row - no atomic, no row zeroed first, a word
// written once.  The served configuration's stack lies in LDS, read-only; a lane keeps its state, how far it has popped into
// that stack and, in dynamic LDS [P][64], what it pushed since (P = min(max_token_bytes, max_depth)).  A work entry whose
// state is an id that no configuration has been given (a caller named it; `advance` never does): the claim is taken back -
// the ids launch behind the fill then serves row 0 - and the row, under eviction, is nobody's
template <bool EVICT>
__global__ __launch_bounds__(PDA_FILL_THREADS) void pda_fill_kernel(Pda p, int32_t P, int32_t *bank, int64_t bank_ld, int32_t capacity,
                                                                   const int32_t *work, const int32_t *counters, int32_t *row_of_state,
                                                                   int32_t *row_state) {
  extern __shared__ uint8_t priv[];  // [P][64]
  __shared__ uint8_t stack[GLB_PDA_MAX_DEPTH + 8];
  __shared__ int32_t range[2];
  if (threadIdx.x == 0) fill_range<EVICT>(counters, capacity, range);
  __syncthreads();
  const int lane = (int)threadIdx.x;
  const int64_t words = (p.vocab + 31) / 32;
  const int64_t t = (int64_t)blockIdx.x * PDA_FILL_THREADS + lane;
  const int64_t w0 = (int64_t)blockIdx.x * 2;
  if (w0 >= words) return;  // (the whole workgroup)
  const int32_t known = numbered(p, N_COUNT);
  for (int32_t e = range[0] + (int32_t)blockIdx.y; e < range[1]; e += (int32_t)gridDim.y) {
    const int32_t s = work[2 * (int64_t)e], r = work[2 * (int64_t)e + 1];
    if (s < 0 || s >= p.max_states || r < 2 || r >= capacity) continue;  // (uniform over the block)
    if (s >= known) {  // an id no configuration has yet: it keeps no row, so that the one that takes the id later gets its own
      if (blockIdx.x == 0 && threadIdx.x == 0) {
        row_of_state[s] = -1;
        if (row_state) row_state[r] = -1;
      }
      continue;
    }
    const uint64_t *config = p.rows + (int64_t)s * p.W;
    int32_t state, depth;
    const bool ok = head_ok(p, config[0], state, depth);  // (uniform)
    __syncthreads();  // (the entry before is read to its end)
    if (ok) {
      const uint8_t *symbols = (const uint8_t *)(config + 1);  // one byte a symbol, bottom first
      for (int32_t i = lane; i < depth; i += PDA_FILL_THREADS) stack[i] = symbols[i];
    }
    __syncthreads();
    bool bit = false;
    if (t < p.vocab) bit = t == p.eos_id ? p.accepting_out[s] != 0 : ok && lane_token(p, P, state, depth, stack, priv, lane, t);
    const uint64_t b = __ballot(bit);
    if (lane == 0) {
      int32_t *row = bank + (int64_t)r * bank_ld;
      row[w0] = (int32_t)(uint32_t)b;
      if (w0 + 1 < words) row[w0 + 1] = (int32_t)(uint32_t)(b >> 32);
    }
  }
}

// ---- the host side -----------------------------------------------------------------------------------------------------------------
int pda_check(const glb_pda_args *a, const char *what, int need) {
  if (const int rc = number_check(a, what, "glb_pda_args", need)) return rc;
  if (a->n_pda_states < 1 || a->n_pda_states > PDA_MAX_AUTOMATON)
    return glb::api_fail(GLB_EINVAL, "%s: n_pda_states %d outside [1, %d]", what, a->n_pda_states, PDA_MAX_AUTOMATON);
  if (a->n_symbols < 1 || a->n_symbols > PDA_MAX_SYMBOLS)
    return glb::api_fail(GLB_EINVAL, "%s: n_symbols %d outside [1, %d]", what, a->n_symbols, PDA_MAX_SYMBOLS);
  if (a->start < 0 || a->start >= a->n_pda_states)
    return glb::api_fail(GLB_EINVAL, "%s: start %d outside [0, n_pda_states = %d)", what, a->start, a->n_pda_states);
  if (a->max_depth < 1 || a->max_depth > GLB_PDA_MAX_DEPTH)
    return glb::api_fail(GLB_EINVAL, "%s: max_depth %d outside [1, %d]: a configuration is one wave, a 64-bit word a lane", what, a->max_depth,
                         GLB_PDA_MAX_DEPTH);
  const int32_t W = 1 + (a->max_depth + 7) / 8;
  if (a->n_words != W) return glb::api_fail(GLB_EINVAL, "%s: n_words %d is not 1 + ceil(max_depth / 8) = %d", what, a->n_words, W);
  if (!a->delta) return glb::api_fail(GLB_EINVAL, "%s: delta is null", what);
  if (!a->accepting) return glb::api_fail(GLB_EINVAL, "%s: accepting is null", what);
  if (!a->configs) return glb::api_fail(GLB_EINVAL, "%s: configs is null", what);
  if ((uintptr_t)a->configs & 7) return glb::api_fail(GLB_EINVAL, "%s: configs is not aligned to 8 bytes", what);
  if (!a->accepting_out) return glb::api_fail(GLB_EINVAL, "%s: accepting_out is null", what);
  return GLB_OK;
}

Pda pda_of(const glb_pda_args *a) {
  const glb_dfa_args *d = &a->dfa;
  unsigned long long *words = (unsigned long long *)a->table;
  return Pda{d->tok_bytes, d->n_bytes, d->tok_ptr, d->skip, d->vocab, d->eos_id, a->n_pda_states, a->n_symbols, a->max_depth, a->n_words,
             a->max_states, a->delta, a->accepting, a->hash_mask, words, (int32_t *)(words + a->table_slots), (uint64_t)a->table_slots - 1,
             a->cand, a->configs, a->accepting_out, a->counts, a->status};
}

}  // namespace

extern "C" {

int glb_pda_init(const glb_pda_args *a, void *stream) {
  if (const int rc = pda_check(a, "glb_pda_init", NEED_BANK)) return rc;
  const glb_dfa_args *d = &a->dfa;
  const hipStream_t st = (hipStream_t)stream;
  const Pda p = pda_of(a);
  const int64_t most = a->table_slots > a->max_states ? a->table_slots : a->max_states;
  hipLaunchKernelGGL(pda_clear_kernel, dim3(blocks_for(most, 256)), dim3(256), 0, st, p);
  hipLaunchKernelGGL(pda_seed_kernel, dim3(1), dim3(64), 0, st, p, a->start);
  const int64_t elems = (d->vocab + 31) / 32;
  hipLaunchKernelGGL(dfa_bank_init_kernel<int32_t>, dim3(blocks_for(elems > a->max_states ? elems : a->max_states, 256)), dim3(256), 0, st,
                     a->max_states, d->eos_id, d->vocab, d->bank, d->bank_ld, elems, d->row_of_state, d->counters);
  if (a->epoch)
    hipLaunchKernelGGL(dfa_evict_init_kernel, dim3(blocks_for(d->capacity, 256)), dim3(256), 0, st, (int32_t)d->capacity, a->row_state,
                       a->row_stamp, a->ecounters, a->epoch);
  return glb::launched("pda_init launch");
}

int glb_pda_advance(const glb_pda_args *a, void *stream) {
  if (const int rc = pda_check(a, "glb_pda_advance", NEED_WALK | NEED_N)) return rc;
  const glb_dfa_args *d = &a->dfa;
  if (!d->tokens || !d->from || !d->to || !d->state_out || d->ld <= 0) return glb::api_fail(GLB_EINVAL, "glb_pda_advance: null pointer or ld <= 0");
  if (!a->cand) return glb::api_fail(GLB_EINVAL, "glb_pda_advance: cand is null");
  if ((uintptr_t)a->cand & 7) return glb::api_fail(GLB_EINVAL, "glb_pda_advance: cand is not aligned to 8 bytes");
  if (!a->counts) return glb::api_fail(GLB_EINVAL, "glb_pda_advance: counts is null");
  if (a->cand_rows < 1 || a->cand_rows > a->table_slots - a->max_states)
    return glb::api_fail(GLB_EINVAL, "glb_pda_advance: cand_rows %lld outside [1, table_slots - max_states = %lld]: the new configurations "
                         "of a chunk must find free slots", (long long)a->cand_rows, (long long)(a->table_slots - a->max_states));
  const hipStream_t st = (hipStream_t)stream;
  const Pda p = pda_of(a);
  for (int64_t base = 0; base < d->n; base += a->cand_rows) {
    const int64_t n = d->n - base < a->cand_rows ? d->n - base : a->cand_rows;
    unsigned waves = 0, blocks = 0;
    if (const int rc = stride_grid("pda: the device's CU count", &waves, n, PDA_WAVES)) return rc;
    if (const int rc = stride_grid("pda: the device's CU count", &blocks, n, PDA_THREADS)) return rc;
    hipLaunchKernelGGL(pda_walk_kernel, dim3(waves), dim3(PDA_THREADS), 0, st, p, base, n, d->tokens, d->ld, d->from, d->to, d->state_in,
                       d->state_out);
    hipLaunchKernelGGL(number_enter_wave_kernel<Pda>, dim3(waves), dim3(PDA_THREADS), 0, st, p, base, n, d->state_out);
    number_launches(p, blocks, base, n, d->state_out, base + n >= d->n, st);
  }
  return glb::launched("pda_advance launch");
}

int glb_pda_serve(const glb_pda_args *a, void *stream) {
  if (const int rc = pda_check(a, "glb_pda_serve", NEED_WALK | NEED_BANK | NEED_N)) return rc;
  const glb_dfa_args *d = &a->dfa;
  if (!d->state_in || !d->out_rows) return glb::api_fail(GLB_EINVAL, "glb_pda_serve: null pointer");
  if (d->max_work <= 0) return glb::api_fail(GLB_EINVAL, "glb_pda_serve: max_work %lld <= 0", (long long)d->max_work);
  if (a->max_token_bytes < 1) return glb::api_fail(GLB_EINVAL, "glb_pda_serve: max_token_bytes %d < 1", a->max_token_bytes);
  const hipStream_t st = (hipStream_t)stream;
  const Pda p = pda_of(a);
  const int32_t capacity = (int32_t)d->capacity, S = a->max_states;
  const int32_t P = a->max_token_bytes < a->max_depth ? a->max_token_bytes : a->max_depth;  // a lane's private stack
  const size_t lds = (size_t)P * PDA_FILL_THREADS;                                           // at most 504 x 64 bytes
  const bool evict = a->epoch != nullptr;
  const unsigned entries = (unsigned)(d->max_work < FILL_MAX_ENTRIES ? d->max_work : FILL_MAX_ENTRIES);
  const dim3 fill(blocks_for(d->vocab, PDA_FILL_THREADS), entries), by_n(blocks_for(d->n, 256));
  if (evict) {
    hipLaunchKernelGGL(dfa_evict_touch_kernel, by_n, dim3(256), 0, st, S, d->n, d->state_in, capacity, d->row_of_state, a->row_stamp,
                       a->claimants, d->counters, a->ecounters, a->epoch);
    hipLaunchKernelGGL(dfa_evict_select_kernel, dim3(1), dim3(SELECT_THREADS), 0, st, S, capacity, d->row_of_state, a->row_state,
                       a->row_stamp, a->claimants, a->victims, d->work, d->counters, a->ecounters, a->epoch);
    hipLaunchKernelGGL(pda_fill_kernel<true>, fill, dim3(PDA_FILL_THREADS), lds, st, p, P, d->bank, d->bank_ld, capacity, d->work, a->ecounters,
                       d->row_of_state, a->row_state);
    hipLaunchKernelGGL(dfa_mask_ids_kernel, by_n, dim3(256), 0, st, S, (const uint8_t *)a->accepting_out, d->n, d->state_in, d->done,
                       d->row_of_state, capacity, d->out_rows, a->ecounters, a->epoch);
  } else {
    hipLaunchKernelGGL(dfa_claim_kernel, by_n, dim3(256), 0, st, S, d->n, d->state_in, capacity, d->row_of_state, d->work, d->counters);
    hipLaunchKernelGGL(pda_fill_kernel<false>, fill, dim3(PDA_FILL_THREADS), lds, st, p, P, d->bank, d->bank_ld, capacity, d->work, d->counters,
                       d->row_of_state, (int32_t *)nullptr);
    hipLaunchKernelGGL(dfa_commit_kernel, dim3(1), dim3(1), 0, st, capacity, d->counters);
    hipLaunchKernelGGL(dfa_mask_ids_kernel, by_n, dim3(256), 0, st, S, (const uint8_t *)a->accepting_out, d->n, d->state_in, d->done,
                       d->row_of_state, capacity, d->out_rows, (int32_t *)nullptr, (int32_t *)nullptr);
  }
  return glb::launched("pda_serve launch");
}

}  // extern "C"
