// glb_pda.hip — a real-time deterministic pushdown automaton over bytes served as a constraint (include/glb.h: glb_pda_*;
// DESIGN.md §25).  A state of the constraint is a configuration - the automaton's state and a bounded stack - of W 64-bit
// words: a wave holds one, a lane a word (glb_set.hpp's hash and key work on the raw words, every byte above the depth being
// zero).  glb_pda_advance walks every particle's tokens from its configuration, byte by byte, in registers; the configuration
// it ends in is looked up and numbered as glb_lazy.hip numbers a set: enter, count, scan, number and resolve are that file's
// kernels over `configs` in place of `sets`, stated a second time here (glb_lazy.hip is left as it is).  The bank of rows is
// glb_dfa_bank.hpp's, unchanged: only the fill is new.  Everything read from device memory is range-checked.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/glb.h"
#include "glb_common.hpp"
#include "glb_dfa_bank.hpp"
#include "glb_set.hpp"

namespace {

enum { P_COUNT = 0, P_FLAGS = 1, P_BASE = 2, P_NEXT = 3 };
constexpr int PDA_THREADS = 256;  // four waves, a particle each; count / number: 256 particles a block
constexpr int PDA_WAVES = PDA_THREADS / 64;
constexpr int PDA_FILL_THREADS = 64;  // the fill: one wave a workgroup, 64 tokens, at most 64 x 504 bytes of private stacks
constexpr int32_t PDA_MAX_CONFIGS = 1 << 22;
constexpr int32_t PDA_MAX_AUTOMATON = 1 << 24;
constexpr int32_t PDA_MAX_SYMBOLS = 126;
constexpr int PDA_POP = 127;
constexpr int32_t NO_PART = 0x7fffffff;
constexpr int32_t PENDING = INT32_MIN;    // state_out between walk and enter: the particle's end configuration lies in its row of `cand`
constexpr uint32_t REF_PART = 0x80000000u;  // the low half of a slot: this bit and a particle index of the chunk, else a numbered id
constexpr uint32_t REF_TOMB = 0xffffffffu;  // a configuration that found no id below max_states: never equal to anything, probed past

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
  uint64_t *cand, *configs;
  uint8_t *accepting_out;
  int32_t *cnt, *status;
};

__device__ inline int32_t flags_now(const int32_t *status) {
  return __hip_atomic_load(&status[P_FLAGS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the configurations numbered, never more than the rows of `configs`
__device__ inline int32_t numbered(const Pda &p, int word) {
  const int32_t c = p.status[word];
  return c < 0 ? 0 : c > p.max_states ? p.max_states : c;
}

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
  if (lane < p.W) p.configs[lane] = word;
  uint64_t slot;
  uint32_t high;
  set_key(p.hash_mask, p.mask, word, lane, slot, high);
  if (lane == 0) {
    p.accepting_out[0] = p.accepting[start] ? 1 : 0;
    p.words[slot] = (unsigned long long)high << 32;  // (id 0; the table is empty)
    p.status[P_COUNT] = p.status[P_BASE] = p.status[P_NEXT] = 1;
  }
}

// ---- advance: six launches over the particles [base, base + n) of a call, particle base + k owning row k of `cand` ---------------
// walk, a wave per particle: the tokens of its range from its configuration, in registers; state_out = -1 (dead), the id
// itself (an empty range) or PENDING with the end configuration in `cand`
__global__ __launch_bounds__(PDA_THREADS) void pda_walk_kernel(Pda p, int64_t base, int64_t n, const int32_t *tokens, int64_t ld,
                                                              const int32_t *from, const int32_t *to, const int32_t *state_in,
                                                              int32_t *state_out) {
  const int lane = (int)threadIdx.x & 63;
  const int32_t known = numbered(p, P_BASE);
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
        const uint64_t word = lane < p.W ? p.configs[(int64_t)s * p.W + lane] : 0ull;
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

// enter, a wave per particle that is PENDING: its end configuration looked up; state_out = the id where an earlier call or
// chunk numbered it, else -2 - slot until pda_resolve_kernel.  A new configuration's slot is claimed by one compare-and-swap
// of the whole word.  A chunk that begins with every id taken claims nothing: a configuration not found is -1 and the overflow
__global__ __launch_bounds__(PDA_THREADS) void pda_enter_kernel(Pda p, int64_t base, int64_t n, int32_t *state_out) {
  const int lane = (int)threadIdx.x & 63;
  const bool full = p.status[P_COUNT] >= p.max_states;  // (written by the chunk before, not by this one)
  const int64_t waves = (int64_t)gridDim.x * PDA_WAVES;
  for (int64_t k = (int64_t)blockIdx.x * PDA_WAVES + (threadIdx.x >> 6); k < n; k += waves) {
    if (state_out[base + k] != PENDING) continue;  // (a whole wave)
    if (flags_now(p.status) & GLB_PDA_BUG) break;
    const uint64_t target = lane < p.W ? p.cand[k * p.W + lane] : 0ull;
    uint64_t slot;
    uint32_t high;
    set_key(p.hash_mask, p.mask, target, lane, slot, high);
    const unsigned long long claim = ((unsigned long long)high << 32) | REF_PART | (uint32_t)k;
    int32_t out = -1;
    bool settled = false;
    for (uint64_t probe = 0; probe <= p.mask && !settled; ++probe, slot = (slot + 1) & p.mask) {
      unsigned long long cur = word_now(&p.words[slot]);  // (one address: the same in every lane)
      if (cur == 0ull) {
        if (full) break;
        unsigned long long old = 0ull;
        if (lane == 0) old = atomicCAS(&p.words[slot], 0ull, claim);
        old = bcast64(old, 0);
        if (old == 0ull) {  // this wave's: a new configuration
          if (lane == 0) atomicMin(&p.partmin[slot], (int32_t)k);
          out = -2 - (int32_t)slot;
          settled = true;
          break;
        }
        cur = old;
      }
      const uint32_t ref = (uint32_t)cur;
      if ((uint32_t)(cur >> 32) == high && ref != REF_TOMB) {
        const uint64_t *row = nullptr;  // the configuration behind the reference
        if (ref & REF_PART) {
          if ((int64_t)(ref & 0x7fffffffu) < n) row = p.cand + (int64_t)(ref & 0x7fffffffu) * p.W;
        } else if ((int32_t)ref < p.max_states) {
          row = p.configs + (int64_t)ref * p.W;
        }
        if (!row) {
          if (lane == 0) atomicOr(&p.status[P_FLAGS], GLB_PDA_BUG);
          settled = true;
          break;
        }
        const uint64_t other = lane < p.W ? row[lane] : 0ull;
        if (!__any(other != target)) {
          if (ref & REF_PART) {
            if (lane == 0) atomicMin(&p.partmin[slot], (int32_t)k);
            out = -2 - (int32_t)slot;
          } else {
            out = (int32_t)ref;
          }
          settled = true;
          break;
        }
      }
      if ((probe & 31) == 31 && (flags_now(p.status) & GLB_PDA_BUG)) settled = true;
    }
    // not found and nothing claimed: every id is taken (or, a table walked all round, every slot)
    if (!settled && lane == 0) atomicOr(&p.status[P_FLAGS], GLB_PDA_OVERFLOW);
    if (lane == 0) state_out[base + k] = out;
  }
}

// whether particle k of the chunk is the one that numbers its end configuration: the smallest to have ended in it
__device__ inline bool wins(const Pda &p, int32_t code, int64_t k, int64_t &slot) {
  slot = -2 - (int64_t)code;
  return code <= -2 && (uint64_t)slot <= p.mask && p.partmin[slot] == (int32_t)k;
}

// cnt[b]: the new configurations that the particles [256 b, 256 b + 256) of the chunk number
__global__ __launch_bounds__(PDA_THREADS) void pda_count_kernel(Pda p, int64_t base, int64_t n, const int32_t *state_out) {
  const int64_t nb = (n + PDA_THREADS - 1) / PDA_THREADS;
  for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const int64_t k = b * PDA_THREADS + threadIdx.x;
    int64_t slot;
    const bool w = k < n && wins(p, state_out[base + k], k, slot);
    const int c = __syncthreads_count(w);
    if (threadIdx.x == 0) p.cnt[b] = c;
  }
}

// one block: cnt becomes its exclusive prefix sums; P_NEXT = the configurations after this chunk, at most max_states - past
// it the overflow flag
__global__ __launch_bounds__(SCAN_THREADS) void pda_scan_kernel(Pda p, int64_t n) {
  __shared__ int32_t wave_sum[SCAN_THREADS / 64];
  __shared__ int32_t carry;
  const int32_t total = scan_exclusive(p.cnt, (int32_t)((n + PDA_THREADS - 1) / PDA_THREADS), wave_sum, &carry);
  if (threadIdx.x == 0) {
    const int64_t next = (int64_t)numbered(p, P_COUNT) + total;  // (total <= n <= 2^30)
    if (next > p.max_states) atomicOr(&p.status[P_FLAGS], GLB_PDA_OVERFLOW);
    p.status[P_NEXT] = (int32_t)(next > p.max_states ? p.max_states : next);
  }
}

// the winners number their configurations: id = P_COUNT + cnt[b] + the winners of the block at smaller particles; the
// configuration copied from `cand`, accepting_out = accepting[state] && depth == 0, and the slot's reference turned into the
// id - or, with no id left, into the tombstone
__global__ __launch_bounds__(PDA_THREADS) void pda_number_kernel(Pda p, int64_t base, int64_t n, const int32_t *state_out) {
  __shared__ int32_t wave_n[PDA_WAVES];
  const int32_t count = numbered(p, P_COUNT);
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int64_t nb = (n + PDA_THREADS - 1) / PDA_THREADS;
  for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const int64_t k = b * PDA_THREADS + threadIdx.x;
    int64_t slot;
    const bool w = k < n && wins(p, state_out[base + k], k, slot);
    const unsigned long long ballot = __ballot(w);
    if (lane == 0) wave_n[wave] = __popcll(ballot);
    __syncthreads();
    int32_t rank = __popcll(ballot & ((1ull << lane) - 1ull));
    for (int v = 0; v < wave; ++v) rank += wave_n[v];
    if (w) {
      const int64_t id = (int64_t)count + p.cnt[b] + rank;
      const unsigned long long high = p.words[slot] & 0xffffffff00000000ull;
      if (id >= 0 && id < p.max_states) {
        const uint64_t *row = p.cand + k * p.W;
        for (int j = 0; j < p.W; ++j) p.configs[id * p.W + j] = row[j];
        int32_t state, depth;
        const bool ok = head_ok(p, row[0], state, depth);
        p.accepting_out[id] = ok && depth == 0 && p.accepting[state] ? 1 : 0;
        p.words[slot] = high | (unsigned long long)id;
      } else {
        p.words[slot] = high | REF_TOMB;
      }
    }
    __syncthreads();
  }
}

// state_out of the chunk: -2 - slot becomes the id its slot was given, -1 behind a tombstone.  The chunk's last launch: the
// count moves on (no launch of the chunk reads it from here), and with the call's last chunk the ids a caller may name
__global__ void pda_resolve_kernel(Pda p, int64_t base, int64_t n, int32_t *state_out, int last) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k == 0) {
    p.status[P_COUNT] = p.status[P_NEXT];
    if (last) p.status[P_BASE] = p.status[P_NEXT];
  }
  if (k >= n) return;
  const int32_t code = state_out[base + k];
  if (code > -2) return;
  const int64_t slot = -2 - (int64_t)code;
  int32_t id = -1;
  bool bug = true;
  if ((uint64_t)slot <= p.mask) {
    const uint32_t ref = (uint32_t)p.words[slot];
    if (ref == REF_TOMB) bug = false;
    else if (!(ref & REF_PART) && (int32_t)ref < p.max_states) id = (int32_t)ref, bug = false;
  }
  if (bug) atomicOr(&p.status[P_FLAGS], GLB_PDA_BUG);
  state_out[base + k] = id;
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
  const int32_t known = numbered(p, P_COUNT);
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
    const uint64_t *config = p.configs + (int64_t)s * p.W;
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
constexpr int NEED_N = 1, NEED_BANK = 2, NEED_WALK = 4;

int pda_check(const glb_pda_args *a, const char *what, int need) {
  if (const int rc = glb::block_ok(a, what, "glb_pda_args")) return rc;
  const glb_dfa_args *d = &a->dfa;
  if (const int rc = glb::block_ok(d, what, "glb_dfa_args")) return rc;
  if (a->max_states < 1 || a->max_states > PDA_MAX_CONFIGS)
    return glb::api_fail(GLB_EINVAL, "%s: max_states %d outside [1, %d]", what, a->max_states, PDA_MAX_CONFIGS);
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
  if (a->table_slots < 2 * (int64_t)a->max_states || a->table_slots > ((int64_t)1 << 30) || (a->table_slots & (a->table_slots - 1)))
    return glb::api_fail(GLB_EINVAL, "%s: table_slots %lld is not a power of two in [2 max_states = %lld, 2^30]", what,
                         (long long)a->table_slots, 2 * (long long)a->max_states);
  if (!a->table) return glb::api_fail(GLB_EINVAL, "%s: table is null", what);
  if ((uintptr_t)a->table & 7) return glb::api_fail(GLB_EINVAL, "%s: table is not aligned to 8 bytes", what);
  if (!a->configs) return glb::api_fail(GLB_EINVAL, "%s: configs is null", what);
  if ((uintptr_t)a->configs & 7) return glb::api_fail(GLB_EINVAL, "%s: configs is not aligned to 8 bytes", what);
  if (!a->accepting_out) return glb::api_fail(GLB_EINVAL, "%s: accepting_out is null", what);
  if (!a->status) return glb::api_fail(GLB_EINVAL, "%s: status is null", what);
  const int tables = !!a->row_state + !!a->row_stamp + !!a->claimants + !!a->victims + !!a->ecounters + !!a->epoch;
  if (tables != 0 && tables != 6) return glb::api_fail(GLB_EINVAL, "%s: the eviction tables are given in part (%d of 6)", what, tables);
  if (d->vocab <= 0 || d->vocab > 0x7fffff00ll) return glb::api_fail(GLB_EINVAL, "%s: vocab %lld", what, (long long)d->vocab);
  if (need & NEED_WALK) {
    if (!d->tok_bytes || !d->tok_ptr || !d->skip || d->n_bytes < 0 || d->n_bytes > 0x7fffffffll)
      return glb::api_fail(GLB_EINVAL, "%s: vocabulary bytes missing", what);
  }
  if (need & NEED_BANK) {
    if (d->bank_ld < (d->vocab + 31) / 32)
      return glb::api_fail(GLB_EINVAL, "%s: bank_ld %lld < %lld words", what, (long long)d->bank_ld, (long long)((d->vocab + 31) / 32));
    if (d->capacity < (tables ? 3 : 2) || d->capacity > (tables ? 65535 : 0x7fffffffll))
      return glb::api_fail(GLB_EINVAL, "%s: capacity %lld (rows 0 and 1 are the bank's own; an evicting bank: [3, 65535])", what, (long long)d->capacity);
    if (!d->bank || !d->row_of_state || !d->work || !d->counters) return glb::api_fail(GLB_EINVAL, "%s: null bank pointer", what);
  }
  if (need & NEED_N) {
    if (d->n <= 0) return glb::api_fail(GLB_EINVAL, "%s: n %lld <= 0", what, (long long)d->n);
  }
  return GLB_OK;
}

Pda pda_of(const glb_pda_args *a) {
  const glb_dfa_args *d = &a->dfa;
  unsigned long long *words = (unsigned long long *)a->table;
  return Pda{d->tok_bytes, d->n_bytes, d->tok_ptr, d->skip, d->vocab, d->eos_id, a->n_pda_states, a->n_symbols, a->max_depth, a->n_words,
             a->max_states, a->delta, a->accepting, a->hash_mask, words, (int32_t *)(words + a->table_slots), (uint64_t)a->table_slots - 1,
             a->cand, a->configs, a->accepting_out, a->counts, a->status};
}

// blocks for a grid that strides over its work: four to a CU, and no more than the work has
int pda_grid(int64_t items, int per_block, unsigned *blocks) {
  static std::atomic<int> cus_of_device{0};  // (one kind of device a process)
  int cus = cus_of_device.load(std::memory_order_relaxed);
  if (cus <= 0) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return glb::api_hip_fail(e, "pda: the device's CU count");
    if (cus <= 0) cus = 256;
    cus_of_device.store(cus, std::memory_order_relaxed);
  }
  const int64_t need = (items + per_block - 1) / per_block, most = (int64_t)cus * 4;
  *blocks = (unsigned)(need < most ? (need > 0 ? need : 1) : most);
  return GLB_OK;
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
    if (const int rc = pda_grid(n, PDA_WAVES, &waves)) return rc;
    if (const int rc = pda_grid(n, PDA_THREADS, &blocks)) return rc;
    hipLaunchKernelGGL(pda_walk_kernel, dim3(waves), dim3(PDA_THREADS), 0, st, p, base, n, d->tokens, d->ld, d->from, d->to, d->state_in,
                       d->state_out);
    hipLaunchKernelGGL(pda_enter_kernel, dim3(waves), dim3(PDA_THREADS), 0, st, p, base, n, d->state_out);
    hipLaunchKernelGGL(pda_count_kernel, dim3(blocks), dim3(PDA_THREADS), 0, st, p, base, n, (const int32_t *)d->state_out);
    hipLaunchKernelGGL(pda_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, p, n);
    hipLaunchKernelGGL(pda_number_kernel, dim3(blocks), dim3(PDA_THREADS), 0, st, p, base, n, (const int32_t *)d->state_out);
    hipLaunchKernelGGL(pda_resolve_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, st, p, base, n, d->state_out, base + n >= d->n ? 1 : 0);
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
