// glb_topk.hpp - the selection core of glb_topk.hip: a wave keeps the largest entries it has seen as a sorted
// list, one entry a lane (lane 0 the largest), each a packed 64-bit value
//     (monotone bits of the key << 32) | ~index        0: no entry
// so that an unsigned maximum yields the largest key and, among equal keys, the lowest index.  -0 is folded into +0 before the
// bits are taken; a key that is not above -inf (NaN too) packs to 0 and is never selected.
// select_chunk offers the wave 64 keys a lane (a 4096-index chunk as glb_rowlse.hpp reads it, or EPV = 1: index
// j * 64 + lane): the chunk is skipped when no lane's largest key reaches the list's k-th entry; otherwise every lane finds its
// largest packed value below its ceiling (a statically unrolled pass: no register number depends on data), the wave takes
// the maxima above the threshold one by one into the list (a lane-neighbour shift), the lanes that gave one lower their ceiling
// to it and look again.  The list is a function of the keys and indices offered, not of the order of the offers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "glb_rowlse.hpp"

namespace glb {

constexpr int kTopkMax = 64;  // entries a wave's list holds: one a lane

__device__ __forceinline__ uint32_t key_mono(float key) {  // float order as unsigned order (after folding -0)
  uint32_t u = __float_as_uint(key);
  u = u == 0x80000000u ? 0u : u;
  return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
}

__device__ __forceinline__ float mono_key(uint32_t m) {
  return __uint_as_float((m & 0x80000000u) ? (m ^ 0x80000000u) : ~m);
}

// nidx: ~index
__device__ __forceinline__ uint64_t pack_entry(float key, uint32_t nidx) {
  return key > kNegInf ? (((uint64_t)key_mono(key) << 32) | nidx) : 0ull;
}
__device__ __forceinline__ int32_t entry_index(uint64_t e) { return (int32_t)~(uint32_t)e; }
__device__ __forceinline__ float entry_key(uint64_t e) { return mono_key((uint32_t)(e >> 32)); }

// wave maximum of an unsigned 64-bit value, wave-uniform (wave_scan_u64's moves: a lane without a source is offered 0)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ uint64_t max_step_u64(uint64_t v) {
  const uint64_t o = dpp_u64_or0<CTRL, ROW_MASK>(v);
  return o > v ? o : v;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
  v = max_step_u64<0x111, 0xf>(v);
  v = max_step_u64<0x112, 0xf>(v);
  v = max_step_u64<0x114, 0xf>(v);
  v = max_step_u64<0x118, 0xf>(v);
  v = max_step_u64<0x142, 0xa>(v);
  v = max_step_u64<0x143, 0xc>(v);
  return readlane_u64(v, 63);
}

// the lane's largest packed value below `ceil` among its 64 keys; nidx0 = ~(index of the lane's element (vector 0, component 0))
template <int EPV>
__device__ __forceinline__ uint64_t lane_best_below(const float (&z)[64], uint32_t nidx0, uint64_t ceil) {
  uint64_t best = 0;
#pragma unroll
  for (int j = 0; j < 64; ++j) {
    const uint64_t p = pack_entry(z[j], nidx0 - (uint32_t)((j / EPV) * 64 * EPV + j % EPV));  // (~(a + b) = ~a - b)
    best = (p < ceil && p > best) ? p : best;
  }
  return best;
}

// `wm` (wave-uniform, above the list's last entry, equal to none) into the sorted list
__device__ __forceinline__ void list_insert(uint64_t &L, uint64_t wm, int lane) {
  const int pos = __popcll(__ballot(L > wm));  // (sorted: the lanes above wm are lanes 0 .. pos - 1)
  const uint64_t up = (uint64_t)__shfl_up((unsigned long long)L, 1);
  L = lane < pos ? L : (lane == pos ? wm : up);
}

// 64 keys a lane with indices base + ((j / EPV) * 64 + lane) * EPV + j % EPV against the wave's list of k entries
template <int EPV>
__device__ __forceinline__ void select_chunk(const float (&z)[64], int base, int lane, int k, uint64_t &L) {
  uint64_t thr = readlane_u64(L, k - 1);
  {
    const float fm = lane_max64(z);
    const bool may = fm > kNegInf && key_mono(fm) >= (uint32_t)(thr >> 32);
    if (__ballot(may) == 0ull) return;  // (wave-uniform)
  }
  const uint32_t nidx0 = ~(uint32_t)(base + lane * EPV);
  uint64_t ceil = ~0ull;
  for (;;) {
    uint64_t pb = lane_best_below<EPV>(z, nidx0, ceil);
    bool gave = false;
    for (;;) {
      const uint64_t wm = wave_max_u64(pb);
      if (wm <= thr) break;  // (wave-uniform; 0: nothing left)
      list_insert(L, wm, lane);
      thr = readlane_u64(L, k - 1);
      if (pb == wm) {  // (one lane: an index occurs once)
        ceil = wm;
        pb = 0;
        gave = true;
      }
    }
    if (__ballot(gave) == 0ull) break;
  }
}

}  // namespace glb
