// glb_conj.hip — the conjunction of K constraints served as one (include/glb.h: glb_conj_*).  A state is the
// tuple of the K part states, W = ceil(K / 2) <= 4 64-bit words, numbered on the device as glb_lazy.hip numbers a set and
// glb_pda.hip a configuration: enter, count, scan, number and resolve are those files' kernels, stated a third time here (both
// are left as they are) - but a LANE per particle, not a wave: a lane packs its tuple from the parts' state arrays, hashes
// it and compares it by itself, where a wave would keep four lanes of 64 busy.  The bank of rows is glb_dfa_bank.hpp's,
// unchanged; the fill is the combine: a new row is the AND (with weights: the ordered float32 sum, -inf under a cleared bit)
// of the parts' rows of one particle that holds the state.  Everything read from device memory is range-checked.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/glb.h"
#include "glb_common.hpp"
#include "glb_dfa_bank.hpp"
#include "glb_set.hpp"

namespace {

enum { P_COUNT = 0, P_FLAGS = 1, P_BASE = 2, P_NEXT = 3 };
constexpr int CONJ_THREADS = 256;  // a particle a lane; count / number: 256 particles a block; the combine: 1024 words or floats
constexpr int CONJ_WAVES = CONJ_THREADS / 64;
constexpr int MAX_K = GLB_CONJ_MAX_PARTS, MAX_W = (GLB_CONJ_MAX_PARTS + 1) / 2;
constexpr int32_t CONJ_MAX_TUPLES = 1 << 22;
constexpr int64_t CONJ_MAX_N = (int64_t)1 << 30;
constexpr int32_t NO_PART = 0x7fffffff;
constexpr uint32_t REF_PART = 0x80000000u;  // the low half of a slot: this bit and a particle index of the chunk, else a numbered id
constexpr uint32_t REF_TOMB = 0xffffffffu;  // a tuple that found no id below max_states: never equal to anything, probed past

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
// four words or floats of a row as one 16-byte access: a row begins wherever its bank's leading dimension puts it, so only
// the alignment of an element is promised
struct __attribute__((packed, aligned(4))) Words4 {
  i32x4 v;
};
struct __attribute__((packed, aligned(4))) Floats4 {
  f32x4 v;
};

struct Conj {
  int32_t K, W, max_states;
  uint64_t hash_mask;
  unsigned long long *words;  // [slots]; 0: empty
  int32_t *partmin;           // [slots]; the smallest particle index of the chunk that brought the slot's tuple
  uint64_t mask;              // slots - 1
  uint64_t *tuples;
  int32_t *cnt, *status;
  int32_t *part_states;
  int64_t part_ld;
};

// the parts' rows and banks, by value: indexed under full unrolling only, so that they stay in scalar registers
struct Parts {
  const int32_t *rows[MAX_K];
  const void *bank[MAX_K];
  int64_t ld[MAX_K], capacity[MAX_K];
  int32_t weighted[MAX_K];
};

__device__ inline int32_t flags_now(const int32_t *status) {
  return __hip_atomic_load(&status[P_FLAGS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the tuples numbered, never more than the rows of `tuples`
__device__ inline int32_t numbered(const Conj &c, int word) {
  const int32_t v = c.status[word];
  return v < 0 ? 0 : v > c.max_states ? c.max_states : v;
}

// the tuple of particle i, packed; false where a part is dead
__device__ inline bool pack(const Conj &c, int64_t i, uint64_t t[MAX_W]) {
  bool alive = true;
#pragma unroll
  for (int j = 0; j < MAX_W; ++j) t[j] = 0ull;
#pragma unroll
  for (int k = 0; k < MAX_K; ++k)
    if (k < c.K) {
      const int32_t s = c.part_states[(int64_t)k * c.part_ld + i];
      alive = alive && s >= 0;
      t[k >> 1] |= (uint64_t)(uint32_t)s << (32 * (k & 1));
    }
  return alive;
}

// where the probing of a tuple starts and the high half of its slot: glb_set.hpp's set_key, one lane over all the words
__device__ inline void tuple_key(const Conj &c, const uint64_t t[MAX_W], uint64_t &slot, uint32_t &high) {
  uint64_t h = 0ull;
#pragma unroll
  for (int j = 0; j < MAX_W; ++j)
    if (j < c.W) h ^= mix64(t[j] ^ ((uint64_t)(j + 1) * 0x9e3779b97f4a7c15ull));
  h = mix64(h);
  if (c.hash_mask) h &= c.hash_mask;
  high = TAG_USED | (uint32_t)((h ^ (h >> 31)) & 0x7fffffffu);
  slot = mix64(h) & c.mask;
}

__device__ inline bool same(const Conj &c, const uint64_t a[MAX_W], const uint64_t b[MAX_W]) {
  bool eq = true;
#pragma unroll
  for (int j = 0; j < MAX_W; ++j)
    if (j < c.W) eq = eq && a[j] == b[j];
  return eq;
}

// ---- init ------------------------------------------------------------------------------------------------------------------------
__global__ void conj_clear_kernel(Conj c, int32_t *rep) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < GLB_CONJ_STATUS) c.status[i] = 0;
  if (i < (uint64_t)c.max_states) rep[i] = -1;
  if (i <= c.mask) {
    c.words[i] = 0;
    c.partmin[i] = NO_PART;
  }
}

struct Start {
  int32_t part[MAX_K];
};

// id 0: the parts' start states, one thread
__global__ void conj_seed_kernel(Conj c, Start start) {
  uint64_t t[MAX_W];
#pragma unroll
  for (int j = 0; j < MAX_W; ++j) t[j] = 0ull;
#pragma unroll
  for (int k = 0; k < MAX_K; ++k)
    if (k < c.K) t[k >> 1] |= (uint64_t)(uint32_t)start.part[k] << (32 * (k & 1));
#pragma unroll
  for (int j = 0; j < MAX_W; ++j)
    if (j < c.W) c.tuples[j] = t[j];
  uint64_t slot;
  uint32_t high;
  tuple_key(c, t, slot, high);
  c.words[slot] = (unsigned long long)high << 32;  // (id 0; the table is empty)
  c.status[P_COUNT] = c.status[P_BASE] = c.status[P_NEXT] = 1;
}

// ---- unpack: a lane a particle, one gather of W words, K stores ------------------------------------------------------------------------
__global__ __launch_bounds__(CONJ_THREADS) void conj_unpack_kernel(Conj c, int64_t n, const int32_t *state_in, const int32_t *done,
                                                                  int32_t *claim_states, int32_t *rep) {
  const int64_t i = (int64_t)blockIdx.x * CONJ_THREADS + threadIdx.x;
  if (i >= n) return;
  const int32_t s = state_in ? state_in[i] : 0;
  const bool known = s >= 0 && s < numbered(c, P_COUNT);
  uint64_t t[MAX_W];
#pragma unroll
  for (int j = 0; j < MAX_W; ++j) t[j] = known && j < c.W ? c.tuples[(int64_t)s * c.W + j] : 0ull;
#pragma unroll
  for (int k = 0; k < MAX_K; ++k)
    if (k < c.K) c.part_states[(int64_t)k * c.part_ld + i] = known ? (int32_t)(uint32_t)(t[k >> 1] >> (32 * (k & 1))) : -1;
  if (claim_states) {
    const bool asks = known && !(done && done[i]);  // (a particle that is done is served row 0 or 1: its state needs no row)
    claim_states[i] = asks ? s : -1;
    if (asks) rep[s] = (int32_t)i;  // (any of the particles that hold s: their part rows are equal within a call)
  }
}

// ---- number: five launches over the particles [base, base + n) of a call, particle base + k the chunk's k -----------------------------
// enter, a lane per particle: its tuple looked up; state_out = -1 where a part is dead, the id where an earlier call or chunk
// numbered the tuple, else -2 - slot until conj_resolve_kernel.  A new tuple's slot is claimed by one compare-and-swap of the
// whole word; no lane waits on another's stores.  A chunk that begins with every id taken claims nothing: a tuple not found
// is -1 and the overflow
__global__ __launch_bounds__(CONJ_THREADS) void conj_enter_kernel(Conj c, int64_t base, int64_t n, int32_t *state_out) {
  const bool full = c.status[P_COUNT] >= c.max_states;  // (written by the chunk before, not by this one)
  const int64_t stride = (int64_t)gridDim.x * CONJ_THREADS;
  for (int64_t k = (int64_t)blockIdx.x * CONJ_THREADS + threadIdx.x; k < n; k += stride) {
    uint64_t target[MAX_W];
    int32_t out = -1;
    if (pack(c, base + k, target) && !(flags_now(c.status) & GLB_CONJ_BUG)) {
      uint64_t slot;
      uint32_t high;
      tuple_key(c, target, slot, high);
      const unsigned long long claim = ((unsigned long long)high << 32) | REF_PART | (uint32_t)k;
      bool settled = false;
      for (uint64_t probe = 0; probe <= c.mask && !settled; ++probe, slot = (slot + 1) & c.mask) {
        unsigned long long cur = word_now(&c.words[slot]);
        if (cur == 0ull) {
          if (full) break;
          const unsigned long long old = atomicCAS(&c.words[slot], 0ull, claim);
          if (old == 0ull) {  // this lane's: a new tuple
            atomicMin(&c.partmin[slot], (int32_t)k);
            out = -2 - (int32_t)slot;
            settled = true;
            break;
          }
          cur = old;
        }
        const uint32_t ref = (uint32_t)cur;
        if ((uint32_t)(cur >> 32) == high && ref != REF_TOMB) {
          uint64_t other[MAX_W];
          bool there = false;  // the tuple behind the reference
          if (ref & REF_PART) {
            if ((int64_t)(ref & 0x7fffffffu) < n) there = pack(c, base + (int64_t)(ref & 0x7fffffffu), other);
          } else if ((int32_t)ref < c.max_states) {
#pragma unroll
            for (int j = 0; j < MAX_W; ++j) other[j] = j < c.W ? c.tuples[(int64_t)ref * c.W + j] : 0ull;
            there = true;
          }
          if (!there) {
            atomicOr(&c.status[P_FLAGS], GLB_CONJ_BUG);
            settled = true;
            break;
          }
          if (same(c, other, target)) {
            if (ref & REF_PART) {
              atomicMin(&c.partmin[slot], (int32_t)k);
              out = -2 - (int32_t)slot;
            } else {
              out = (int32_t)ref;
            }
            settled = true;
            break;
          }
        }
        if ((probe & 31) == 31 && (flags_now(c.status) & GLB_CONJ_BUG)) settled = true;
      }
      // not found and nothing claimed: every id is taken (or, a table walked all round, every slot)
      if (!settled) atomicOr(&c.status[P_FLAGS], GLB_CONJ_OVERFLOW);
    }
    state_out[base + k] = out;
  }
}

// whether particle k of the chunk is the one that numbers its tuple: the smallest to have ended in it
__device__ inline bool wins(const Conj &c, int32_t code, int64_t k, int64_t &slot) {
  slot = -2 - (int64_t)code;
  return code <= -2 && (uint64_t)slot <= c.mask && c.partmin[slot] == (int32_t)k;
}

// cnt[b]: the new tuples that the particles [256 b, 256 b + 256) of the chunk number
__global__ __launch_bounds__(CONJ_THREADS) void conj_count_kernel(Conj c, int64_t base, int64_t n, const int32_t *state_out) {
  const int64_t nb = (n + CONJ_THREADS - 1) / CONJ_THREADS;
  for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const int64_t k = b * CONJ_THREADS + threadIdx.x;
    int64_t slot;
    const bool w = k < n && wins(c, state_out[base + k], k, slot);
    const int total = __syncthreads_count(w);
    if (threadIdx.x == 0) c.cnt[b] = total;
  }
}

// one block: cnt becomes its exclusive prefix sums; P_NEXT = the tuples after this chunk, at most max_states - past it the
// overflow flag
__global__ __launch_bounds__(SCAN_THREADS) void conj_scan_kernel(Conj c, int64_t n) {
  __shared__ int32_t wave_sum[SCAN_THREADS / 64];
  __shared__ int32_t carry;
  const int32_t total = scan_exclusive(c.cnt, (int32_t)((n + CONJ_THREADS - 1) / CONJ_THREADS), wave_sum, &carry);
  if (threadIdx.x == 0) {
    const int64_t next = (int64_t)numbered(c, P_COUNT) + total;  // (total <= n <= 2^30)
    if (next > c.max_states) atomicOr(&c.status[P_FLAGS], GLB_CONJ_OVERFLOW);
    c.status[P_NEXT] = (int32_t)(next > c.max_states ? c.max_states : next);
  }
}

// the winners number their tuples: id = P_COUNT + cnt[b] + the winners of the block at smaller particles; the tuple packed
// once more into `tuples`, and the slot's reference turned into the id - or, with no id left, into the tombstone
__global__ __launch_bounds__(CONJ_THREADS) void conj_number_kernel(Conj c, int64_t base, int64_t n, const int32_t *state_out) {
  __shared__ int32_t wave_n[CONJ_WAVES];
  const int32_t count = numbered(c, P_COUNT);
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int64_t nb = (n + CONJ_THREADS - 1) / CONJ_THREADS;
  for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const int64_t k = b * CONJ_THREADS + threadIdx.x;
    int64_t slot;
    const bool w = k < n && wins(c, state_out[base + k], k, slot);
    const unsigned long long ballot = __ballot(w);
    if (lane == 0) wave_n[wave] = __popcll(ballot);
    __syncthreads();
    int32_t rank = __popcll(ballot & ((1ull << lane) - 1ull));
    for (int v = 0; v < wave; ++v) rank += wave_n[v];
    if (w) {
      const int64_t id = (int64_t)count + c.cnt[b] + rank;
      const unsigned long long high = c.words[slot] & 0xffffffff00000000ull;
      if (id >= 0 && id < c.max_states) {
        uint64_t t[MAX_W];
        pack(c, base + k, t);
#pragma unroll
        for (int j = 0; j < MAX_W; ++j)
          if (j < c.W) c.tuples[id * c.W + j] = t[j];
        c.words[slot] = high | (unsigned long long)id;
      } else {
        c.words[slot] = high | REF_TOMB;
      }
    }
    __syncthreads();
  }
}

// state_out of the chunk: -2 - slot becomes the id its slot was given, -1 behind a tombstone.  The chunk's last launch: the
// count moves on (no launch of the chunk reads it from here), and with the call's last chunk the ids a caller may name
__global__ void conj_resolve_kernel(Conj c, int64_t base, int64_t n, int32_t *state_out, int last) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k == 0) {
    c.status[P_COUNT] = c.status[P_NEXT];
    if (last) c.status[P_BASE] = c.status[P_NEXT];
  }
  if (k >= n) return;
  const int32_t code = state_out[base + k];
  if (code > -2) return;
  const int64_t slot = -2 - (int64_t)code;
  int32_t id = -1;
  bool bug = true;
  if ((uint64_t)slot <= c.mask) {
    const uint32_t ref = (uint32_t)c.words[slot];
    if (ref == REF_TOMB) bug = false;
    else if (!(ref & REF_PART) && (int32_t)ref < c.max_states) id = (int32_t)ref, bug = false;
  }
  if (bug) atomicOr(&c.status[P_FLAGS], GLB_CONJ_BUG);
  state_out[base + k] = id;
}

// ---- the combine: the rows of the work entries, from the parts' rows of one particle that holds the state -----------------------------
// Grid (row chunks, work entries side by side), a lane four elements of the row: words of a bit bank, floats - tokens - of a
// float bank.  Thread 0 of a block finds the entry's particle and its K part rows, every one range-checked, into LDS; an
// entry that has none (its state was named by no particle of this call, or a part row lies outside that part's bank) is
// skipped and its claim taken back, so that the ids launch serves row 0 and a later call claims again
template <bool EVICT, bool FLOAT>
__global__ __launch_bounds__(CONJ_THREADS) void conj_combine_kernel(Parts p, int32_t K, int64_t vocab, int32_t max_states, int64_t n,
                                                                   const int32_t *claim_states, const int32_t *rep,
                                                                   std::conditional_t<FLOAT, float, int32_t> *bank, int64_t bank_ld,
                                                                   int32_t capacity, const int32_t *work, const int32_t *counters,
                                                                   int32_t *row_of_state, int32_t *row_state) {
  __shared__ int32_t range[2];
  __shared__ int32_t part_row[MAX_K];
  __shared__ int32_t found;
  if (threadIdx.x == 0) fill_range<EVICT>(counters, capacity, range);
  __syncthreads();
  const int64_t words = (vocab + 31) / 32, elems = FLOAT ? vocab : words;
  const int64_t e0 = 4 * ((int64_t)blockIdx.x * CONJ_THREADS + threadIdx.x);
  for (int32_t e = range[0] + (int32_t)blockIdx.y; e < range[1]; e += (int32_t)gridDim.y) {
    const int32_t s = work[2 * (int64_t)e], r = work[2 * (int64_t)e + 1];
    if (s < 0 || s >= max_states || r < 2 || r >= capacity) continue;  // (uniform over the block)
    __syncthreads();  // (the entry before is read to its end)
    if (threadIdx.x == 0) {
      const int32_t i = rep[s];
      bool ok = i >= 0 && i < n && claim_states[i] == s;
#pragma unroll
      for (int k = 0; k < MAX_K; ++k)
        if (k < K && ok) {
          const int32_t rk = p.rows[k][i];
          ok = rk >= 0 && rk < p.capacity[k];
          part_row[k] = rk;
        }
      found = ok;
      if (!ok && blockIdx.x == 0) {
        row_of_state[s] = -1;
        if (row_state) row_state[r] = -1;
      }
    }
    __syncthreads();
    if (!found || e0 >= elems) continue;
    if constexpr (FLOAT) {
      float *row = bank + (int64_t)r * bank_ld;
      if (e0 + 3 < elems) {
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < MAX_K; ++k)
          if (k < K && p.weighted[k]) acc += ((const Floats4 *)((const float *)p.bank[k] + (int64_t)part_row[k] * p.ld[k] + e0))->v;
        uint32_t bits = 0xfu;
#pragma unroll
        for (int k = 0; k < MAX_K; ++k)
          if (k < K && !p.weighted[k])  // (e0 is a multiple of four: its four tokens lie in one word)
            bits &= (uint32_t)((const int32_t *)p.bank[k])[(int64_t)part_row[k] * p.ld[k] + (e0 >> 5)] >> (e0 & 31);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (!((bits >> j) & 1u)) acc[j] = -__builtin_inff();
        Floats4 q;
        q.v = acc;
        *(Floats4 *)(row + e0) = q;
      } else {
        for (int64_t t = e0; t < elems; ++t) {
          float acc = 0.0f;
          bool bit = true;
#pragma unroll
          for (int k = 0; k < MAX_K; ++k)
            if (k < K) {
              if (p.weighted[k]) acc += ((const float *)p.bank[k])[(int64_t)part_row[k] * p.ld[k] + t];
              else bit = bit && (((uint32_t)((const int32_t *)p.bank[k])[(int64_t)part_row[k] * p.ld[k] + (t >> 5)] >> (t & 31)) & 1u);
            }
          row[t] = bit ? acc : -__builtin_inff();
        }
      }
    } else {
      int32_t *row = bank + (int64_t)r * bank_ld;
      if (e0 + 3 < elems) {
        i32x4 acc = {-1, -1, -1, -1};
#pragma unroll
        for (int k = 0; k < MAX_K; ++k)
          if (k < K) acc &= ((const Words4 *)((const int32_t *)p.bank[k] + (int64_t)part_row[k] * p.ld[k] + e0))->v;
        Words4 q;
        q.v = acc;
        *(Words4 *)(row + e0) = q;
      } else {
        for (int64_t w = e0; w < elems; ++w) {
          int32_t acc = -1;
#pragma unroll
          for (int k = 0; k < MAX_K; ++k)
            if (k < K) acc &= ((const int32_t *)p.bank[k])[(int64_t)part_row[k] * p.ld[k] + w];
          row[w] = acc;
        }
      }
    }
  }
}

// every particle's row: `done` - row 1 where every part served its row 1, else row 0; else the state's row, 0 for a dead state
// or one without a row.  With `ecounters` and `epoch` (an evicting bank) the call ends here, as in dfa_mask_ids_kernel
__global__ void conj_ids_kernel(Parts p, int32_t K, int32_t max_states, int64_t n, const int32_t *states, const int32_t *done,
                                const int32_t *row_of_state, int32_t capacity, int32_t *out, int32_t *ecounters, int32_t *epoch) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 && ecounters && epoch) {  // (no launch of this call reads either after the selection)
    if (*epoch < 0x7fffffff) *epoch += 1;
    ecounters[E_CLAIMANTS] = 0;
    ecounters[E_TAKEN] = 0;
  }
  if (i >= n) return;
  if (done && done[i]) {
    bool all = true;
#pragma unroll
    for (int k = 0; k < MAX_K; ++k)
      if (k < K) all = all && p.rows[k][i] == 1;
    out[i] = all ? 1 : 0;
    return;
  }
  const int32_t s = states[i];
  int32_t r = 0;
  if (s >= 0 && s < max_states) {
    r = row_of_state[s];
    if (r < 2 || r >= capacity) r = 0;
  }
  out[i] = r;
}

// ---- the host side -----------------------------------------------------------------------------------------------------------------
constexpr int NEED_N = 1, NEED_BANK = 2, NEED_STATES = 4;

int conj_check(const glb_conj_args *a, const char *what, int need) {
  if (const int rc = glb::block_ok(a, what, "glb_conj_args")) return rc;
  const glb_dfa_args *d = &a->dfa;
  if (const int rc = glb::block_ok(d, what, "glb_dfa_args")) return rc;
  if (a->n_parts < 2 || a->n_parts > GLB_CONJ_MAX_PARTS)
    return glb::api_fail(GLB_EINVAL, "%s: n_parts %d outside [2, %d]", what, a->n_parts, GLB_CONJ_MAX_PARTS);
  if (a->n_words != (a->n_parts + 1) / 2)
    return glb::api_fail(GLB_EINVAL, "%s: n_words %d is not ceil(n_parts / 2) = %d", what, a->n_words, (a->n_parts + 1) / 2);
  if (a->max_states < 1 || a->max_states > CONJ_MAX_TUPLES)
    return glb::api_fail(GLB_EINVAL, "%s: max_states %d outside [1, %d]", what, a->max_states, CONJ_MAX_TUPLES);
  if (a->table_slots < 2 * (int64_t)a->max_states || a->table_slots > ((int64_t)1 << 30) || (a->table_slots & (a->table_slots - 1)))
    return glb::api_fail(GLB_EINVAL, "%s: table_slots %lld is not a power of two in [2 max_states = %lld, 2^30]", what,
                         (long long)a->table_slots, 2 * (long long)a->max_states);
  if (!a->table) return glb::api_fail(GLB_EINVAL, "%s: table is null", what);
  if ((uintptr_t)a->table & 7) return glb::api_fail(GLB_EINVAL, "%s: table is not aligned to 8 bytes", what);
  if (!a->tuples) return glb::api_fail(GLB_EINVAL, "%s: tuples is null", what);
  if ((uintptr_t)a->tuples & 7) return glb::api_fail(GLB_EINVAL, "%s: tuples is not aligned to 8 bytes", what);
  if (!a->status) return glb::api_fail(GLB_EINVAL, "%s: status is null", what);
  if (!a->rep) return glb::api_fail(GLB_EINVAL, "%s: rep is null", what);
  const int tables = !!a->row_state + !!a->row_stamp + !!a->claimants + !!a->victims + !!a->ecounters + !!a->epoch;
  if (tables != 0 && tables != 6) return glb::api_fail(GLB_EINVAL, "%s: the eviction tables are given in part (%d of 6)", what, tables);
  if (d->vocab <= 0 || d->vocab > 0x7fffff00ll) return glb::api_fail(GLB_EINVAL, "%s: vocab %lld", what, (long long)d->vocab);
  if (need & NEED_BANK) {
    const int64_t ld = a->wbank ? a->wbank_ld : d->bank_ld, elems = a->wbank ? d->vocab : (d->vocab + 31) / 32;
    if (ld < elems)
      return glb::api_fail(GLB_EINVAL, "%s: %s %lld < %lld %s", what, a->wbank ? "wbank_ld" : "bank_ld", (long long)ld, (long long)elems,
                           a->wbank ? "floats" : "words");
    if (d->capacity < (tables ? 3 : 2) || d->capacity > (tables ? 65535 : 0x7fffffffll))
      return glb::api_fail(GLB_EINVAL, "%s: capacity %lld (rows 0 and 1 are the bank's own; an evicting bank: [3, 65535])", what, (long long)d->capacity);
    if ((!d->bank && !a->wbank) || !d->row_of_state || !d->work || !d->counters) return glb::api_fail(GLB_EINVAL, "%s: null bank pointer", what);
  }
  if (need & NEED_N) {
    if (d->n <= 0 || d->n > CONJ_MAX_N) return glb::api_fail(GLB_EINVAL, "%s: n %lld outside [1, 2^30]", what, (long long)d->n);
  }
  if (need & NEED_STATES) {
    if (!a->part_states) return glb::api_fail(GLB_EINVAL, "%s: part_states is null", what);
    if (a->part_ld < d->n) return glb::api_fail(GLB_EINVAL, "%s: part_ld %lld < n = %lld", what, (long long)a->part_ld, (long long)d->n);
  }
  return GLB_OK;
}

Conj conj_of(const glb_conj_args *a) {
  unsigned long long *words = (unsigned long long *)a->table;
  return Conj{a->n_parts, a->n_words, a->max_states, a->hash_mask, words, (int32_t *)(words + a->table_slots), (uint64_t)a->table_slots - 1,
              a->tuples, a->counts, a->status, a->part_states, a->part_ld};
}

Parts parts_of(const glb_conj_args *a) {
  Parts p{};
  for (int k = 0; k < a->n_parts; ++k) {
    p.rows[k] = a->part_rows[k], p.bank[k] = a->part_bank[k];
    p.ld[k] = a->part_bank_ld[k], p.capacity[k] = a->part_capacity[k], p.weighted[k] = a->part_weighted[k];
  }
  return p;
}

// blocks for a grid that strides over its work: four to a CU, and no more than the work has
int conj_grid(int64_t items, int per_block, unsigned *blocks) {
  static std::atomic<int> cus_of_device{0};  // (one kind of device a process)
  int cus = cus_of_device.load(std::memory_order_relaxed);
  if (cus <= 0) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return glb::api_hip_fail(e, "conj: the device's CU count");
    if (cus <= 0) cus = 256;
    cus_of_device.store(cus, std::memory_order_relaxed);
  }
  const int64_t need = (items + per_block - 1) / per_block, most = (int64_t)cus * 4;
  *blocks = (unsigned)(need < most ? (need > 0 ? need : 1) : most);
  return GLB_OK;
}

template <bool FLOAT>
void conj_serve_launches(const glb_conj_args *a, hipStream_t st) {
  const glb_dfa_args *d = &a->dfa;
  const Parts p = parts_of(a);
  const int32_t capacity = (int32_t)d->capacity, S = a->max_states, K = a->n_parts;
  std::conditional_t<FLOAT, float, int32_t> *bank;
  int64_t ld;
  if constexpr (FLOAT) bank = a->wbank, ld = a->wbank_ld;
  else bank = d->bank, ld = d->bank_ld;
  const int64_t elems = FLOAT ? d->vocab : (d->vocab + 31) / 32;
  const unsigned entries = (unsigned)(d->max_work < FILL_MAX_ENTRIES ? d->max_work : FILL_MAX_ENTRIES);
  const dim3 fill(blocks_for(elems, 4 * CONJ_THREADS), entries), by_n(blocks_for(d->n, 256));
  if (a->epoch) {
    hipLaunchKernelGGL(dfa_evict_touch_kernel, by_n, dim3(256), 0, st, S, d->n, (const int32_t *)a->claim_states, capacity, d->row_of_state,
                       a->row_stamp, a->claimants, d->counters, a->ecounters, a->epoch);
    hipLaunchKernelGGL(dfa_evict_select_kernel, dim3(1), dim3(SELECT_THREADS), 0, st, S, capacity, d->row_of_state, a->row_state,
                       a->row_stamp, a->claimants, a->victims, d->work, d->counters, a->ecounters, a->epoch);
    hipLaunchKernelGGL((conj_combine_kernel<true, FLOAT>), fill, dim3(CONJ_THREADS), 0, st, p, K, d->vocab, S, d->n,
                       (const int32_t *)a->claim_states, (const int32_t *)a->rep, bank, ld, capacity, d->work, a->ecounters, d->row_of_state,
                       a->row_state);
    hipLaunchKernelGGL(conj_ids_kernel, by_n, dim3(256), 0, st, p, K, S, d->n, d->state_in, d->done, d->row_of_state, capacity, d->out_rows,
                       a->ecounters, a->epoch);
  } else {
    hipLaunchKernelGGL(dfa_claim_kernel, by_n, dim3(256), 0, st, S, d->n, (const int32_t *)a->claim_states, capacity, d->row_of_state, d->work,
                       d->counters);
    hipLaunchKernelGGL((conj_combine_kernel<false, FLOAT>), fill, dim3(CONJ_THREADS), 0, st, p, K, d->vocab, S, d->n,
                       (const int32_t *)a->claim_states, (const int32_t *)a->rep, bank, ld, capacity, d->work, d->counters, d->row_of_state,
                       (int32_t *)nullptr);
    hipLaunchKernelGGL(dfa_commit_kernel, dim3(1), dim3(1), 0, st, capacity, d->counters);
    hipLaunchKernelGGL(conj_ids_kernel, by_n, dim3(256), 0, st, p, K, S, d->n, d->state_in, d->done, d->row_of_state, capacity, d->out_rows,
                       (int32_t *)nullptr, (int32_t *)nullptr);
  }
}

}  // namespace

extern "C" {

int glb_conj_init(const glb_conj_args *a, void *stream) {
  if (const int rc = conj_check(a, "glb_conj_init", NEED_BANK)) return rc;
  Start start{};
  for (int k = 0; k < a->n_parts; ++k) {
    if (a->part_start[k] < 0) return glb::api_fail(GLB_EINVAL, "glb_conj_init: part_start[%d] = %d < 0", k, a->part_start[k]);
    start.part[k] = a->part_start[k];
  }
  const glb_dfa_args *d = &a->dfa;
  const hipStream_t st = (hipStream_t)stream;
  const Conj c = conj_of(a);
  const int64_t most = a->table_slots > a->max_states ? a->table_slots : a->max_states;
  hipLaunchKernelGGL(conj_clear_kernel, dim3(blocks_for(most, 256)), dim3(256), 0, st, c, a->rep);
  hipLaunchKernelGGL(conj_seed_kernel, dim3(1), dim3(1), 0, st, c, start);
  if (a->wbank) {
    const int64_t elems = d->vocab;
    hipLaunchKernelGGL(dfa_bank_init_kernel<float>, dim3(blocks_for(elems > a->max_states ? elems : a->max_states, 256)), dim3(256), 0, st,
                       a->max_states, d->eos_id, d->vocab, a->wbank, a->wbank_ld, elems, d->row_of_state, d->counters);
  } else {
    const int64_t elems = (d->vocab + 31) / 32;
    hipLaunchKernelGGL(dfa_bank_init_kernel<int32_t>, dim3(blocks_for(elems > a->max_states ? elems : a->max_states, 256)), dim3(256), 0, st,
                       a->max_states, d->eos_id, d->vocab, d->bank, d->bank_ld, elems, d->row_of_state, d->counters);
  }
  if (a->epoch)
    hipLaunchKernelGGL(dfa_evict_init_kernel, dim3(blocks_for(d->capacity, 256)), dim3(256), 0, st, (int32_t)d->capacity, a->row_state,
                       a->row_stamp, a->ecounters, a->epoch);
  return glb::launched("conj_init launch");
}

int glb_conj_unpack(const glb_conj_args *a, void *stream) {
  if (const int rc = conj_check(a, "glb_conj_unpack", NEED_N | NEED_STATES)) return rc;
  const glb_dfa_args *d = &a->dfa;
  hipLaunchKernelGGL(conj_unpack_kernel, dim3(blocks_for(d->n, CONJ_THREADS)), dim3(CONJ_THREADS), 0, (hipStream_t)stream, conj_of(a), d->n,
                     d->state_in, d->done, a->claim_states, a->rep);
  return glb::launched("conj_unpack launch");
}

int glb_conj_number(const glb_conj_args *a, void *stream) {
  if (const int rc = conj_check(a, "glb_conj_number", NEED_N | NEED_STATES)) return rc;
  const glb_dfa_args *d = &a->dfa;
  if (!d->state_out) return glb::api_fail(GLB_EINVAL, "glb_conj_number: state_out is null");
  if (!a->counts) return glb::api_fail(GLB_EINVAL, "glb_conj_number: counts is null");
  if (a->cand_rows < 1 || a->cand_rows > a->table_slots - a->max_states)
    return glb::api_fail(GLB_EINVAL, "glb_conj_number: cand_rows %lld outside [1, table_slots - max_states = %lld]: the new tuples of a "
                         "chunk must find free slots", (long long)a->cand_rows, (long long)(a->table_slots - a->max_states));
  const hipStream_t st = (hipStream_t)stream;
  const Conj c = conj_of(a);
  for (int64_t base = 0; base < d->n; base += a->cand_rows) {
    const int64_t n = d->n - base < a->cand_rows ? d->n - base : a->cand_rows;
    unsigned blocks = 0;
    if (const int rc = conj_grid(n, CONJ_THREADS, &blocks)) return rc;
    hipLaunchKernelGGL(conj_enter_kernel, dim3(blocks), dim3(CONJ_THREADS), 0, st, c, base, n, d->state_out);
    hipLaunchKernelGGL(conj_count_kernel, dim3(blocks), dim3(CONJ_THREADS), 0, st, c, base, n, (const int32_t *)d->state_out);
    hipLaunchKernelGGL(conj_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, st, c, n);
    hipLaunchKernelGGL(conj_number_kernel, dim3(blocks), dim3(CONJ_THREADS), 0, st, c, base, n, (const int32_t *)d->state_out);
    hipLaunchKernelGGL(conj_resolve_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, st, c, base, n, d->state_out, base + n >= d->n ? 1 : 0);
  }
  return glb::launched("conj_number launch");
}

int glb_conj_serve(const glb_conj_args *a, void *stream) {
  if (const int rc = conj_check(a, "glb_conj_serve", NEED_N | NEED_BANK)) return rc;
  const glb_dfa_args *d = &a->dfa;
  if (!d->state_in) return glb::api_fail(GLB_EINVAL, "glb_conj_serve: state_in is null");
  if (!d->out_rows) return glb::api_fail(GLB_EINVAL, "glb_conj_serve: out_rows is null");
  if (!a->claim_states) return glb::api_fail(GLB_EINVAL, "glb_conj_serve: claim_states is null");
  if (d->max_work <= 0) return glb::api_fail(GLB_EINVAL, "glb_conj_serve: max_work %lld <= 0", (long long)d->max_work);
  for (int k = 0; k < a->n_parts; ++k) {
    if (!a->part_rows[k]) return glb::api_fail(GLB_EINVAL, "glb_conj_serve: part_rows[%d] is null", k);
    if (!a->part_bank[k]) return glb::api_fail(GLB_EINVAL, "glb_conj_serve: part_bank[%d] is null", k);
    if (a->part_weighted[k] && !a->wbank)
      return glb::api_fail(GLB_EINVAL, "glb_conj_serve: part_weighted[%d] is set and wbank is null: a weighted part needs a float bank", k);
    const int64_t elems = a->part_weighted[k] ? d->vocab : (d->vocab + 31) / 32;
    if (a->part_bank_ld[k] < elems)
      return glb::api_fail(GLB_EINVAL, "glb_conj_serve: part_bank_ld[%d] %lld < %lld", k, (long long)a->part_bank_ld[k], (long long)elems);
    if (a->part_capacity[k] < 2 || a->part_capacity[k] > 0x7fffffffll)
      return glb::api_fail(GLB_EINVAL, "glb_conj_serve: part_capacity[%d] %lld outside [2, 2^31)", k, (long long)a->part_capacity[k]);
  }
  if (a->wbank) conj_serve_launches<true>(a, (hipStream_t)stream);
  else conj_serve_launches<false>(a, (hipStream_t)stream);
  return glb::launched("conj_serve launch");
}

}  // extern "C"
