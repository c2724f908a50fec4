// glb_conj.hip — the conjunction of K constraints served as one (include/glb.h: glb_conj_*).  A state is the
// tuple of the K part states, W = ceil(K / 2) <= 4 64-bit words, numbered on the device as glb_lazy.hip numbers a set and
// glb_pda.hip a configuration: count, scan, number and resolve are glb_number.hpp's kernels over this file's `Conj`, whose
// store_row packs the tuple once more.  Enter is this file's own: a LANE per particle, not a wave - a lane packs its tuple
// from the parts' state arrays, hashes it and compares it by itself, where a wave would keep four lanes of 64 busy.  The bank
// of rows is glb_dfa_bank.hpp's, unchanged; the fill is the combine: a new row is the AND (with weights: the ordered float32
// sum, -inf under a cleared bit) of the parts' rows of one particle that holds the state.  Everything read from device memory
// is range-checked.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/glb.h"
#include "glb_common.hpp"
#include "glb_dfa_bank.hpp"
#include "glb_number.hpp"
#include "glb_set.hpp"

namespace {

constexpr int CONJ_THREADS = NUMBER_THREADS;  // enter: a particle a lane; the combine: 1024 words or floats a block
constexpr int MAX_K = GLB_CONJ_MAX_PARTS, MAX_W = (GLB_CONJ_MAX_PARTS + 1) / 2;
constexpr int64_t CONJ_MAX_N = (int64_t)1 << 30;

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
  uint64_t *rows;             // [max_states][W]: the numbered tuples
  int32_t *cnt, *status;
  int32_t *part_states;
  int64_t part_ld;
  static __device__ void store_row(const Conj &c, int64_t id, int64_t base, int64_t k);
};

// the parts' rows and banks, by value: indexed under full unrolling only, so that they stay in scalar registers
struct Parts {
  const int32_t *rows[MAX_K];
  const void *bank[MAX_K];
  int64_t ld[MAX_K], capacity[MAX_K];
  int32_t weighted[MAX_K];
};

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

// the tuple of a winner (glb_number.hpp, number_kernel) packed once more into `rows`
__device__ inline void Conj::store_row(const Conj &c, int64_t id, int64_t base, int64_t k) {
  uint64_t t[MAX_W];
  pack(c, base + k, t);
#pragma unroll
  for (int j = 0; j < MAX_W; ++j)
    if (j < c.W) c.rows[id * c.W + j] = t[j];
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
    if (j < c.W) c.rows[j] = t[j];
  uint64_t slot;
  uint32_t high;
  tuple_key(c, t, slot, high);
  c.words[slot] = (unsigned long long)high << 32;  // (id 0; the table is empty)
  c.status[N_COUNT] = c.status[N_BASE] = c.status[N_NEXT] = 1;
}

// ---- unpack: a lane a particle, one gather of W words, K stores ------------------------------------------------------------------------
__global__ __launch_bounds__(CONJ_THREADS) void conj_unpack_kernel(Conj c, int64_t n, const int32_t *state_in, const int32_t *done,
                                                                  int32_t *claim_states, int32_t *rep) {
  const int64_t i = (int64_t)blockIdx.x * CONJ_THREADS + threadIdx.x;
  if (i >= n) return;
  const int32_t s = state_in ? state_in[i] : 0;
  const bool known = s >= 0 && s < numbered(c, N_COUNT);
  uint64_t t[MAX_W];
#pragma unroll
  for (int j = 0; j < MAX_W; ++j) t[j] = known && j < c.W ? c.rows[(int64_t)s * c.W + j] : 0ull;
#pragma unroll
  for (int k = 0; k < MAX_K; ++k)
    if (k < c.K) c.part_states[(int64_t)k * c.part_ld + i] = known ? (int32_t)(uint32_t)(t[k >> 1] >> (32 * (k & 1))) : -1;
  if (claim_states) {
    const bool asks = known && !(done && done[i]);  // (a particle that is done is served row 0 or 1: its state needs no row)
    claim_states[i] = asks ? s : -1;
    if (asks) rep[s] = (int32_t)i;  // (any of the particles that hold s: their part rows are equal within a call)
  }
}

// ---- number: five launches over the particles [base, base + n) of a call, particle base + k the chunk's k: enter, then the
// four of glb_number.hpp
// enter, a lane per particle: its tuple looked up; state_out = -1 where a part is dead, the id where an earlier call or chunk
// numbered the tuple, else -2 - slot until number_resolve_kernel.  A new tuple's slot is claimed by one compare-and-swap of the
// whole word; no lane waits on another's stores.  A chunk that begins with every id taken claims nothing: a tuple not found
// is -1 and the overflow
__global__ __launch_bounds__(CONJ_THREADS) void conj_enter_kernel(Conj c, int64_t base, int64_t n, int32_t *state_out) {
  const bool full = c.status[N_COUNT] >= c.max_states;  // (written by the chunk before, not by this one)
  const int64_t stride = (int64_t)gridDim.x * CONJ_THREADS;
  for (int64_t k = (int64_t)blockIdx.x * CONJ_THREADS + threadIdx.x; k < n; k += stride) {
    uint64_t target[MAX_W];
    int32_t out = -1;
    if (pack(c, base + k, target) && !(flags_now(c.status) & NUMBER_BUG)) {
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
            for (int j = 0; j < MAX_W; ++j) other[j] = j < c.W ? c.rows[(int64_t)ref * c.W + j] : 0ull;
            there = true;
          }
          if (!there) {
            atomicOr(&c.status[N_FLAGS], NUMBER_BUG);
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
        if ((probe & 31) == 31 && (flags_now(c.status) & NUMBER_BUG)) settled = true;
      }
      // not found and nothing claimed: every id is taken (or, a table walked all round, every slot)
      if (!settled) atomicOr(&c.status[N_FLAGS], NUMBER_OVERFLOW);
    }
    state_out[base + k] = out;
  }
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
constexpr int NEED_STATES = 8;  // (beside glb_number.hpp's NEED_N and NEED_BANK, both checked here: a float bank, a bound on n)

int conj_check(const glb_conj_args *a, const char *what, int need) {
  if (const int rc = number_check(a, what, "glb_conj_args", 0)) return rc;
  const glb_dfa_args *d = &a->dfa;
  if (a->n_parts < 2 || a->n_parts > GLB_CONJ_MAX_PARTS)
    return glb::api_fail(GLB_EINVAL, "%s: n_parts %d outside [2, %d]", what, a->n_parts, GLB_CONJ_MAX_PARTS);
  if (a->n_words != (a->n_parts + 1) / 2)
    return glb::api_fail(GLB_EINVAL, "%s: n_words %d is not ceil(n_parts / 2) = %d", what, a->n_words, (a->n_parts + 1) / 2);
  if (!a->tuples) return glb::api_fail(GLB_EINVAL, "%s: tuples is null", what);
  if ((uintptr_t)a->tuples & 7) return glb::api_fail(GLB_EINVAL, "%s: tuples is not aligned to 8 bytes", what);
  if (!a->rep) return glb::api_fail(GLB_EINVAL, "%s: rep is null", what);
  const bool tables = a->epoch != nullptr;  // (all six or none)
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
    if (const int rc = stride_grid("conj: the device's CU count", &blocks, n, CONJ_THREADS)) return rc;
    hipLaunchKernelGGL(conj_enter_kernel, dim3(blocks), dim3(CONJ_THREADS), 0, st, c, base, n, d->state_out);
    number_launches(c, blocks, base, n, d->state_out, base + n >= d->n, st);
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
