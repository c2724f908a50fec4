// glb_set.hpp — a set of important NFA states held by one wave, a 64-bit word a lane: what
// glb_nfa_det.hip (determinisation) and glb_lazy.hip (subsets made while decoding) share - the hash of a set, a lane's word
// in every lane, a slot's two halves, and the one-block scan that turns counts into offsets.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr int SCAN_THREADS = 1024;
constexpr uint32_t TAG_USED = 0x80000000u;  // the high half of a slot that is not empty: this bit and 31 bits of hash

__device__ inline uint64_t mix64(uint64_t x) {  // (the finaliser of splitmix64)
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

// lane `src`'s value in every lane
__device__ inline uint64_t bcast64(uint64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
  return ((uint64_t)hi << 32) | lo;
}

// the hash of the set a wave holds (lanes >= W hold zero and add nothing), the same in every lane
__device__ inline uint64_t set_hash(uint64_t word, int lane) {
  uint64_t h = word ? mix64(word ^ ((uint64_t)(lane + 1) * 0x9e3779b97f4a7c15ull)) : 0ull;
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)h, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(h >> 32), d);
    h ^= ((uint64_t)hi << 32) | lo;
  }
  return mix64(h);
}

// where the probing of a set starts in a table of mask + 1 slots, and the high half of its slot; hash_mask != 0 is ANDed
// onto the hash first
__device__ inline void set_key(uint64_t hash_mask, uint64_t mask, uint64_t word, int lane, uint64_t &slot, uint32_t &high) {
  uint64_t h = set_hash(word, lane);
  if (hash_mask) h &= hash_mask;
  high = TAG_USED | (uint32_t)((h ^ (h >> 31)) & 0x7fffffffu);
  slot = mix64(h) & mask;
}

__device__ inline unsigned long long word_now(const unsigned long long *w) {
  return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One block of SCAN_THREADS, every thread of it: cnt[0 .. n) becomes its exclusive prefix sums; the total, in every thread.
// wave_sum [SCAN_THREADS / 64] and carry [1] are the block's LDS
__device__ inline int32_t scan_exclusive(int32_t *cnt, int32_t n, int32_t *wave_sum, int32_t *carry) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  if (threadIdx.x == 0) *carry = 0;
  __syncthreads();
  for (int32_t base = 0; base < n; base += SCAN_THREADS) {
    const int32_t k = base + (int32_t)threadIdx.x;
    const int32_t v = k < n ? cnt[k] : 0;
    int32_t incl = v;
    for (int d = 1; d < 64; d <<= 1) {
      const int32_t up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int32_t before = *carry;
    for (int w = 0; w < wave; ++w) before += wave_sum[w];
    if (k < n) cnt[k] = before + incl - v;
    __syncthreads();
    if (threadIdx.x == SCAN_THREADS - 1) *carry = before + incl;
    __syncthreads();
  }
  return *carry;
}

}  // namespace
