// glb_set.hpp — a set of important NFA states held by one wave, a 64-bit word a lane: what
// glb_nfa_det.hip (determinisation) and glb_lazy.hip (subsets made while decoding) share - the hash of a set, a lane's word
// in every lane, a slot's two halves.  The mixer, a word read as it is now and the one-block scan are glb_block.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "glb_block.hpp"

namespace {

constexpr uint32_t TAG_USED = 0x80000000u;  // the high half of a slot that is not empty: this bit and 31 bits of hash

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

}  // namespace
