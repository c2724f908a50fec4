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
#include "glb_dfa_bank.hpp"

namespace {

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

template <bool WEIGHTED, bool EVICT>
__global__ __launch_bounds__(FILL_THREADS) void dfa_fill_kernel(Dfa d, const float *arc_logw, const float *final_logw,
                                                               std::conditional_t<WEIGHTED, float, int32_t> *bank,
                                                               int64_t bank_ld, int32_t capacity, const int32_t *work,
                                                               const int32_t *counters) {
  __shared__ int32_t range[2];
  if (threadIdx.x == 0) fill_range<EVICT>(counters, capacity, range);
  __syncthreads();
  dfa_fill_entries<WEIGHTED>(d, arc_logw, final_logw, bank, bank_ld, capacity, work, range[0], range[1]);
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
