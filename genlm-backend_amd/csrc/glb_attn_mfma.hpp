// glb_attn_mfma.hpp - what the MFMA tile attention kernels share (glb_attn_tile.hip: a chunk over a KV slab row, DESIGN.md §34;
// glb_attn_batch.hip: a padded batch by strides under a mask, §35): the tile's shape, its way into LDS and the two products
// on it.  How a kernel finds its keys, what it masks and how it folds a tile into the softmax state stay with the kernel.
//   TileShape<DT, DH>   sizes of a tile of KT keys in LDS and in the 256 threads' registers
//   stage_tile          the registers of a loaded tile to LDS: K rows padded, 16-bit V transposed into operand order
//   tile_scores         S^T = K . Q^T: s[half][v] = score of key 16 half + 4 quad + v of the tile for the lane's own query
//   tile_pv             O^T += V^T . P^T: o[dt][v] = dim 16 dt + 4 quad + v of the lane's own query
//   store4              four consecutive output dims of one query
// Lane (col = lane & 15, quad = lane >> 4) of a wave belongs to query row col of the wave's 16-row fragment throughout.
// Templates and inlined device functions only: each kernel's arithmetic is the text below, in both files the same.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/glb.h"
#include "glb_attn.hpp"

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int KT = 32;          // key positions of a tile
constexpr int THREADS = 256;    // 4 waves
constexpr int QROWS = 64;       // query rows of a block: one 16-row fragment per wave

template <int DT, int DH>
struct TileShape {
  static constexpr bool F32 = DT == GLB_F32;
  static constexpr int ES = F32 ? 4 : 2, EPV = 16 / ES;  // element size; elements of a 16-byte vector
  static constexpr int VPR = DH / EPV;                   // vectors of a key's row
  static constexpr int KPITCH = DH * ES + 16;            // bytes of a K row in LDS (float32: of a V row too)
  static constexpr int VTPITCH = KT * 2 + 16;            // bytes of a row of V^T [dim][key] (16-bit types)
  static constexpr int K_BYTES = KT * KPITCH, V_BYTES = F32 ? KT * KPITCH : DH * VTPITCH;
  static constexpr int NQ = F32 ? DH / 16 : DH / 32;     // Q operand vectors of a lane
  static constexpr int NK = KT * VPR / THREADS;          // K vectors a thread moves per tile (float32: V vectors too)
  static constexpr int NV = F32 ? NK : 2;                // 16-bit V: two keys of one 8-dim chunk
  static constexpr int ND = DH / 16;                     // output tiles of 16 dims
  static_assert(NK >= 1 && NK * THREADS == KT * VPR && (F32 || (KT / 2) * VPR <= THREADS), "a tile must deal out evenly");
  // 16-bit V: thread x < 16 VPR moves chunk x % VPR of the keys in operand slots 2 j, 2 j + 1 (j = x / VPR); the key of the
  // tile in slot 2 j - slot 2 j + 1 holds the next
  static __device__ __forceinline__ int v_key(int tid) {
    const int vj = tid / VPR;
    return 16 * ((2 * vj & 7) >> 2) + 4 * (vj >> 2) + (2 * vj & 3);
  }
};

template <int DT>
__device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c) {
  if constexpr (DT == GLB_BF16)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// four consecutive output dims of one query
template <int DT>
__device__ __forceinline__ void store4(char *p, const float (&x)[4]) {
  if constexpr (DT == GLB_F32) {
    *reinterpret_cast<f32x4 *>(p) = f32x4{x[0], x[1], x[2], x[3]};
  } else {
    const float y[8] = {x[0], x[1], x[2], x[3], 0.0f, 0.0f, 0.0f, 0.0f};
    const u32x4 w = pack16v<DT>(y);
    *reinterpret_cast<u32x2 *>(p) = u32x2{w.x, w.y};
  }
}

// kreg[i]: vector x % VPR of key x / VPR of the tile, x = tid + i THREADS; vreg: the same of V (float32), or chunk tid % VPR of
// the keys v_key(tid), v_key(tid) + 1 (16-bit, threads below 16 VPR)
template <int DT, int DH>
__device__ __forceinline__ void stage_tile(char *k_lds, char *v_lds, const u32x4 (&kreg)[TileShape<DT, DH>::NK],
                                           const u32x4 (&vreg)[TileShape<DT, DH>::NV], int tid) {
  using S = TileShape<DT, DH>;
  constexpr int VPR = S::VPR, KPITCH = S::KPITCH, VTPITCH = S::VTPITCH;
#pragma unroll
  for (int i = 0; i < S::NK; ++i) {
    const int x = tid + i * THREADS, key = x / VPR, ch = x - key * VPR;
    *reinterpret_cast<u32x4 *>(k_lds + key * KPITCH + ch * 16) = kreg[i];
    if constexpr (S::F32) *reinterpret_cast<u32x4 *>(v_lds + key * KPITCH + ch * 16) = vreg[i];
  }
  if constexpr (!S::F32) {
    if (tid < (KT / 2) * VPR) {
      const int vj = tid / VPR, vch = tid - vj * VPR;
      const uint32_t lo[4] = {vreg[0].x, vreg[0].y, vreg[0].z, vreg[0].w}, hi[4] = {vreg[1].x, vreg[1].y, vreg[1].z, vreg[1].w};
#pragma unroll
      for (int e = 0; e < 8; ++e) {  // dim 8 ch + e of both keys as one word
        const uint32_t x0 = (lo[e >> 1] >> (16 * (e & 1))) & 0xffffu, x1 = (hi[e >> 1] >> (16 * (e & 1))) & 0xffffu;
        *reinterpret_cast<uint32_t *>(v_lds + (vch * 8 + e) * VTPITCH + vj * 4) = x0 | (x1 << 16);
      }
    }
  }
}

// qv: the fragment's Q operand - lane (col, quad) holds dims 32 c + 8 quad .. (16-bit) / 16 c + 4 quad .. (float32) of its query
template <int DT, int DH>
__device__ __forceinline__ void tile_scores(const char *k_lds, const u32x4 (&qv)[TileShape<DT, DH>::NQ], f32x4 (&s)[2], int col, int quad) {
  using S = TileShape<DT, DH>;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    s[half] = f32x4{0.f, 0.f, 0.f, 0.f};
    const char *kp = k_lds + (16 * half + col) * S::KPITCH + quad * 16;
#pragma unroll
    for (int c = 0; c < S::NQ; ++c) {
      const u32x4 kv = *reinterpret_cast<const u32x4 *>(kp + c * 64);
      if constexpr (S::F32) {
        const uint32_t kw[4] = {kv.x, kv.y, kv.z, kv.w}, qw[4] = {qv[c].x, qv[c].y, qv[c].z, qv[c].w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          s[half] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(kw[e]), __uint_as_float(qw[e]), s[half], 0, 0, 0);
      } else {
        s[half] = mfma16<DT>(kv, qv[c], s[half]);
      }
    }
  }
}

// p[i]: the probability of key 16 (i >> 2) + 4 quad + (i & 3) of the tile for the lane's query - the accumulator layout of
// tile_scores, which IS the lane's share of the B operand as long as V^T is read in the same key order
template <int DT, int DH>
__device__ __forceinline__ void tile_pv(const char *v_lds, const float (&p)[8], f32x4 (&o)[TileShape<DT, DH>::ND], int col, int quad) {
  using S = TileShape<DT, DH>;
  if constexpr (S::F32) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const char *vp = v_lds + (16 * (i >> 2) + 4 * quad + (i & 3)) * S::KPITCH + col * 4;
#pragma unroll
      for (int dt = 0; dt < S::ND; ++dt)
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(*reinterpret_cast<const float *>(vp + dt * 64), p[i], o[dt], 0, 0, 0);
    }
  } else {
    const u32x4 pb = pack16v<DT>(p);  // slots 8 quad + 4 half + v: the order V^T is stored in
#pragma unroll
    for (int dt = 0; dt < S::ND; ++dt)
      o[dt] = mfma16<DT>(*reinterpret_cast<const u32x4 *>(v_lds + (16 * dt + col) * S::VTPITCH + quad * 16), pb, o[dt]);
  }
}

}  // namespace
