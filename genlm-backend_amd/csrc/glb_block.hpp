// glb_block.hpp — what the units that number states on the device share below their own pipelines (glb_search.hpp: the
// queue search of DESIGN.md §22 / §23; glb_number.hpp: the particles of §24; glb_set.hpp; glb_dfa_min.hip): the 64-bit
// mixer, a word read as it is now, the one-block scan that turns counts into offsets, the rank of a thread among its
// block's, and the grid of four blocks a CU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/glb.h"
#include "glb_common.hpp"

namespace {

constexpr int SCAN_THREADS = 1024;

__device__ inline uint64_t mix64(uint64_t x) {  // (the finaliser of splitmix64)
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  return x ^ (x >> 31);
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

// Every thread of the block: the threads before this one whose `w` holds.  wave_n [waves of the block] is the block's LDS;
// a barrier lies between two calls
__device__ inline int32_t block_rank(bool w, int32_t *wave_n) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const unsigned long long ballot = __ballot(w);
  if (lane == 0) wave_n[wave] = __popcll(ballot);
  __syncthreads();
  int32_t rank = __popcll(ballot & ((1ull << lane) - 1ull));
  for (int v = 0; v < wave; ++v) rank += wave_n[v];
  return rank;
}

// blocks for a grid that strides over its work: four to a CU - the size of a launch whose work only the device knows - and,
// for `items` in blocks of `per_block`, no more than the work has; `what` names the failure
inline int stride_grid(const char *what, unsigned *blocks, int64_t items = INT64_MAX, int per_block = 1) {
  static std::atomic<int> cus_of_device{0};  // (one kind of device a process)
  int cus = cus_of_device.load(std::memory_order_relaxed);
  if (cus <= 0) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return glb::api_hip_fail(e, what);
    if (cus <= 0) cus = 256;
    cus_of_device.store(cus, std::memory_order_relaxed);
  }
  const int64_t need = items / per_block + (items % per_block != 0), most = (int64_t)cus * 4;
  *blocks = (unsigned)(need < most ? (need > 0 ? need : 1) : most);
  return GLB_OK;
}

}  // namespace
