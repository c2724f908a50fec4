// glb_number.hpp — states numbered on the device when a particle reaches them: what glb_lazy.hip (a state is
// a set of NFA states), glb_pda.hip (a configuration) and glb_conj.hip (a tuple of part states) share.  A state is W 64-bit
// words; it is looked up in the table of §23 - a slot one word, 31 bits of hash and a reference: the particle of this chunk
// that claimed it (written by the launch before the one that probes: no wave waits for another's stores) or the id of a
// numbered state (its row of `rows`).  The smallest particle index to end in a new state numbers it, so ids and rows do not
// depend on the order the atomics take.  A chunk of particles [base, base + n) is numbered by five launches: enter, count,
// scan, number, resolve.  The scan, the rank of a winner among its block's and the launch grid (stride_grid) are
// glb_block.hpp's.
//
// The kernels are templates over the translation unit's parameter struct P, passed by value.  P has: W, max_states,
// hash_mask, words, partmin, mask, rows, cnt, status - and cand where number_enter_wave_kernel is used - and a
//   static __device__ void store_row(const P &p, int64_t id, int64_t base, int64_t k)
// that writes row `id` of `rows`, and whatever the unit keeps beside a row, for particle k of the chunk.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/glb.h"
#include "glb_block.hpp"
#include "glb_common.hpp"
#include "glb_set.hpp"

namespace {

enum { N_COUNT = 0, N_FLAGS = 1, N_BASE = 2, N_NEXT = 3 };  // the status words: numbered, flags, numbered when the call began, after this chunk
enum { NUMBER_OVERFLOW = 1, NUMBER_BUG = 2 };               // the flags, the same in the three blocks of include/glb.h
static_assert(GLB_LAZY_OVERFLOW == NUMBER_OVERFLOW && GLB_PDA_OVERFLOW == NUMBER_OVERFLOW && GLB_CONJ_OVERFLOW == NUMBER_OVERFLOW, "");
static_assert(GLB_LAZY_BUG == NUMBER_BUG && GLB_PDA_BUG == NUMBER_BUG && GLB_CONJ_BUG == NUMBER_BUG, "");
constexpr int NUMBER_THREADS = 256;  // enter: four waves, a particle each (or a lane each); count / number: 256 particles a block
constexpr int NUMBER_WAVES = NUMBER_THREADS / 64;
constexpr int32_t NUMBER_MAX_STATES = 1 << 22;
constexpr int32_t NO_PART = 0x7fffffff;
constexpr int32_t PENDING = INT32_MIN;      // state_out between walk and enter: the particle's end state lies in its row of `cand`
constexpr uint32_t REF_PART = 0x80000000u;  // the low half of a slot: this bit and a particle index of the chunk, else a numbered id
constexpr uint32_t REF_TOMB = 0xffffffffu;  // a state that found no id below max_states: never equal to anything, probed past

__device__ inline int32_t flags_now(const int32_t *status) {
  return __hip_atomic_load(&status[N_FLAGS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the states numbered, never more than the rows of `rows`
template <typename P>
__device__ inline int32_t numbered(const P &p, int word) {
  const int32_t c = p.status[word];
  return c < 0 ? 0 : c > p.max_states ? p.max_states : c;
}

// enter, a wave per particle that is PENDING: its end state looked up; state_out = the id where an earlier call or chunk
// numbered it, else -2 - slot until number_resolve_kernel.  A new state's slot is claimed by one compare-and-swap of the whole
// word.  A chunk that begins with every id taken claims nothing: a state not found is -1 and the overflow
template <typename P>
__global__ __launch_bounds__(NUMBER_THREADS) void number_enter_wave_kernel(P p, int64_t base, int64_t n, int32_t *state_out) {
  const int lane = (int)threadIdx.x & 63;
  const bool full = p.status[N_COUNT] >= p.max_states;  // (written by the chunk before, not by this one)
  const int64_t waves = (int64_t)gridDim.x * NUMBER_WAVES;
  for (int64_t k = (int64_t)blockIdx.x * NUMBER_WAVES + (threadIdx.x >> 6); k < n; k += waves) {
    if (state_out[base + k] != PENDING) continue;  // (a whole wave)
    if (flags_now(p.status) & NUMBER_BUG) break;
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
        if (old == 0ull) {  // this wave's: a new state
          if (lane == 0) atomicMin(&p.partmin[slot], (int32_t)k);
          out = -2 - (int32_t)slot;
          settled = true;
          break;
        }
        cur = old;
      }
      const uint32_t ref = (uint32_t)cur;
      if ((uint32_t)(cur >> 32) == high && ref != REF_TOMB) {
        const uint64_t *row = nullptr;  // the state behind the reference
        if (ref & REF_PART) {
          if ((int64_t)(ref & 0x7fffffffu) < n) row = p.cand + (int64_t)(ref & 0x7fffffffu) * p.W;
        } else if ((int32_t)ref < p.max_states) {
          row = p.rows + (int64_t)ref * p.W;
        }
        if (!row) {
          if (lane == 0) atomicOr(&p.status[N_FLAGS], NUMBER_BUG);
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
      if ((probe & 31) == 31 && (flags_now(p.status) & NUMBER_BUG)) settled = true;
    }
    // not found and nothing claimed: every id is taken (or, a table walked all round, every slot)
    if (!settled && lane == 0) atomicOr(&p.status[N_FLAGS], NUMBER_OVERFLOW);
    if (lane == 0) state_out[base + k] = out;
  }
}

// whether particle k of the chunk is the one that numbers its end state: the smallest to have ended in it
template <typename P>
__device__ inline bool wins(const P &p, int32_t code, int64_t k, int64_t &slot) {
  slot = -2 - (int64_t)code;
  return code <= -2 && (uint64_t)slot <= p.mask && p.partmin[slot] == (int32_t)k;
}

// cnt[b]: the new states that the particles [256 b, 256 b + 256) of the chunk number
template <typename P>
__global__ __launch_bounds__(NUMBER_THREADS) void number_count_kernel(P p, int64_t base, int64_t n, const int32_t *state_out) {
  const int64_t nb = (n + NUMBER_THREADS - 1) / NUMBER_THREADS;
  for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const int64_t k = b * NUMBER_THREADS + threadIdx.x;
    int64_t slot;
    const bool w = k < n && wins(p, state_out[base + k], k, slot);
    const int c = __syncthreads_count(w);
    if (threadIdx.x == 0) p.cnt[b] = c;
  }
}

// one block: cnt becomes its exclusive prefix sums; N_NEXT = the states after this chunk, at most max_states - past it the
// overflow flag
template <typename P>
__global__ __launch_bounds__(SCAN_THREADS) void number_scan_kernel(P p, int64_t n) {
  __shared__ int32_t wave_sum[SCAN_THREADS / 64];
  __shared__ int32_t carry;
  const int32_t total = scan_exclusive(p.cnt, (int32_t)((n + NUMBER_THREADS - 1) / NUMBER_THREADS), wave_sum, &carry);
  if (threadIdx.x == 0) {
    const int64_t next = (int64_t)numbered(p, N_COUNT) + total;  // (total <= n <= 2^30)
    if (next > p.max_states) atomicOr(&p.status[N_FLAGS], NUMBER_OVERFLOW);
    p.status[N_NEXT] = (int32_t)(next > p.max_states ? p.max_states : next);
  }
}

// the winners number their states: id = N_COUNT + cnt[b] + the winners of the block at smaller particles; the row written
// by P::store_row, and the slot's reference turned into the id - or, with no id left, into the tombstone
template <typename P>
__global__ __launch_bounds__(NUMBER_THREADS) void number_kernel(P p, int64_t base, int64_t n, const int32_t *state_out) {
  __shared__ int32_t wave_n[NUMBER_WAVES];
  const int32_t count = numbered(p, N_COUNT);
  const int64_t nb = (n + NUMBER_THREADS - 1) / NUMBER_THREADS;
  for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    const int64_t k = b * NUMBER_THREADS + threadIdx.x;
    int64_t slot;
    const bool w = k < n && wins(p, state_out[base + k], k, slot);
    const int32_t rank = block_rank(w, wave_n);
    if (w) {
      const int64_t id = (int64_t)count + p.cnt[b] + rank;
      const unsigned long long high = p.words[slot] & 0xffffffff00000000ull;
      if (id >= 0 && id < p.max_states) {
        P::store_row(p, id, base, k);
        p.words[slot] = high | (unsigned long long)id;
      } else {
        p.words[slot] = high | REF_TOMB;
      }
    }
    __syncthreads();
  }
}

// state_out of the chunk: -2 - slot becomes the id its slot was given, -1 behind a tombstone.  The chunk's last launch: the
// count moves on (no launch of the chunk reads it from here), and with the call's last chunk the states a caller may name
template <typename P>
__global__ void number_resolve_kernel(P p, int64_t base, int64_t n, int32_t *state_out, int last) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k == 0) {
    p.status[N_COUNT] = p.status[N_NEXT];
    if (last) p.status[N_BASE] = p.status[N_NEXT];
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
  if (bug) atomicOr(&p.status[N_FLAGS], NUMBER_BUG);
  state_out[base + k] = id;
}

// ---- the host side -----------------------------------------------------------------------------------------------------------------
// the launches of a chunk behind its enter: count, scan, number, resolve (`last`: the call's last chunk)
template <typename P>
void number_launches(const P &p, unsigned blocks, int64_t base, int64_t n, int32_t *state_out, bool last, hipStream_t st) {
  hipLaunchKernelGGL(number_count_kernel<P>, dim3(blocks), dim3(NUMBER_THREADS), 0, st, p, base, n, (const int32_t *)state_out);
  hipLaunchKernelGGL(number_scan_kernel<P>, dim3(1), dim3(SCAN_THREADS), 0, st, p, n);
  hipLaunchKernelGGL(number_kernel<P>, dim3(blocks), dim3(NUMBER_THREADS), 0, st, p, base, n, (const int32_t *)state_out);
  hipLaunchKernelGGL(number_resolve_kernel<P>, dim3(blocks_for(n, 256)), dim3(256), 0, st, p, base, n, state_out, last ? 1 : 0);
}

// What the three blocks (A: glb_lazy_args, glb_pda_args, glb_conj_args) are refused for alike: the block and its glb_dfa_args,
// max_states, the table, the status words, eviction tables given in part, the vocabulary's size; then, of the embedded
// glb_dfa_args, the groups `need` names.  `what` is the entry's name, `block` the block's.  Each unit's own checks follow
constexpr int NEED_N = 1, NEED_BANK = 2, NEED_WALK = 4;

template <typename A>
int number_check(const A *a, const char *what, const char *block, int need) {
  if (const int rc = glb::block_ok(a, what, block)) return rc;
  const glb_dfa_args *d = &a->dfa;
  if (const int rc = glb::block_ok(d, what, "glb_dfa_args")) return rc;
  if (a->max_states < 1 || a->max_states > NUMBER_MAX_STATES)
    return glb::api_fail(GLB_EINVAL, "%s: max_states %d outside [1, %d]", what, a->max_states, NUMBER_MAX_STATES);
  if (a->table_slots < 2 * (int64_t)a->max_states || a->table_slots > ((int64_t)1 << 30) || (a->table_slots & (a->table_slots - 1)))
    return glb::api_fail(GLB_EINVAL, "%s: table_slots %lld is not a power of two in [2 max_states = %lld, 2^30]", what,
                         (long long)a->table_slots, 2 * (long long)a->max_states);
  if (!a->table) return glb::api_fail(GLB_EINVAL, "%s: table is null", what);
  if ((uintptr_t)a->table & 7) return glb::api_fail(GLB_EINVAL, "%s: table is not aligned to 8 bytes", what);
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

}  // namespace
