// glb_attn_tile.hip - glb_slab_attention_tile (include/glb.h): the attention of a forward that feeds up to
// GLB_KV_TILE_MAX = 128 new tokens per row over KV slab rows where they lie - glb_slab_attention_chunk's contract for chunks
// that kernel's one-wave-per-query design does not reach.  There a row's T x G query waves each walk the whole cached
// prefix; here the K / V of a (row, KV head) come on chip once per 64 queries and both products run on MFMA.
//
// Work split.  A workgroup of 4 waves serves (row, KV head, block of 64 query rows); query row qr = t * G + g is new token t
// under query head hk * G + g (t-major: a 16-row fragment's tokens are neighbours, so whole key tiles are wholly visible to
// it or wholly behind it).  A wave owns one 16-row fragment; lane (col = lane & 15, quad = lane >> 4) belongs to query row
// col of the fragment in EVERYTHING below - operand, scores, softmax state, output - so no value ever changes lanes except
// the two butterfly steps (xor 16, xor 32) of a row maximum and, once, of the row sum.
//
// Data movement.  Keys come in tiles of KT = 32 positions: slab positions below pos, then k_new / v_new from pos on (never what
// the slab held there).  All 256 threads load a tile with 16-byte loads into registers while the previous tile is worked on,
// then write it to LDS, where the four waves share it.  K rows are padded by 16 bytes (row pitch = 4 banks off a multiple of
// 64: the sixteen keys of an operand read start in different banks).  Positions past the block's last visible key are read
// from that last key - every address formed is a valid one - and masked.
//
// Matrix instructions.  The wave computes S^T = K . Q^T (A operand: K rows from LDS; B operand: the fragment's Q, in
// registers for the whole launch): the accumulator then holds, for the lane's OWN query, scores of keys 4 quad + v and
// 16 + 4 quad + v (v = 0 .. 3).  Those eight probabilities ARE the lane's share of the B operand of O^T = V^T . P^T as long as
// V^T's A operand is read in the same key order, so P never passes through LDS.  16-bit types: v_mfma_f32_16x16x32_{bf16,
// f16}; V is transposed on its way into LDS ([dim][key], keys in operand order: slot 8 quad + 4 half + v holds key
// 16 half + 4 quad + v), pairs of keys written as one 32-bit word, and one 16-byte read gives a lane its operand.  float32:
// v_mfma_f32_16x16x4f32 on unrounded inputs, V stays [key][dim] and one 4-byte read per instruction gives the operand.  The
// online softmax runs in float32 on the accumulators; P is rounded to the element type only as the MFMA operand.  O^T's
// accumulator gives the lane four consecutive output dims of its own query: 8- / 16-byte stores.
//
// Masking per tile and fragment: a tile wholly visible takes no per-element test, a tile wholly behind the fragment is not
// computed.  Key 0 is visible to every query, so after the first tile every row maximum is finite: exp(-inf - -inf) cannot
// occur.  Padded query rows (t >= n_new, or past T G) compute on the row's last valid query and store zeros / nothing.
//
// The append: the LAST query block that holds a valid query reads every new position on its way to LDS, and writes those
// vectors to the slab as it holds them; no thread of the launch reads slab positions >= pos.
//
// Safety: pos, n_new and row_of are checked before any address is formed from them; a bad row (block-uniform) stores NaN and
// returns before the first barrier.  No atomics, no workspace: fit for a captured graph.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/glb.h"
#include "glb_attn.hpp"
#include "glb_attn_host.hpp"
#include "glb_attn_mfma.hpp"
#include "glb_common.hpp"

namespace {

struct TileArgs {
  const char *q, *k_new, *v_new;
  char *k_slab, *v_slab, *out;
  const int32_t *pos, *n_new, *row_of;
  int64_t q_sr, q_sh, q_sp, k_sr, k_sh, k_sp, v_sr, v_sh, v_sp;  // element strides: row, head, position
  int32_t n, H, Hkv, cap, T, n_slab_rows, QB;                   // QB: query blocks of a (row, KV head)
  float scale;
};

template <int DT, int DH>
__global__ __launch_bounds__(THREADS) void slab_attention_tile_kernel(const TileArgs a) {
  using S = TileShape<DT, DH>;
  constexpr bool F32 = S::F32;
  constexpr int ES = S::ES, VPR = S::VPR, NQ = S::NQ, NK = S::NK, NV = S::NV, ND = S::ND;
  __shared__ __attribute__((aligned(16))) char k_lds[S::K_BYTES];
  __shared__ __attribute__((aligned(16))) char v_lds[S::V_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
  const int qb = blockIdx.x % a.QB, rk = blockIdx.x / a.QB, hk = rk % a.Hkv, r = rk / a.Hkv;
  const int G = a.H / a.Hkv, TG = a.T * G;
  const int pos = a.pos[r], nn = a.n_new[r];
  const int64_t sr = a.row_of ? (int64_t)a.row_of[r] : (int64_t)r;
  // a chunk that does not lie inside the row (or a row outside the slab): the caller's bug - no fault, no plausible answer:
  // NaN for the whole row, nothing appended.  Nothing below forms an address from pos / nn / sr of such a row.
  const bool bad = pos < 0 || nn < 1 || nn > a.T || (int64_t)pos + nn > a.cap || sr < 0 || sr >= a.n_slab_rows;
  const int n_valid = bad ? 0 : nn * G;  // query rows 0 .. n_valid - 1 are real
  const int qr = qb * QROWS + wave * 16 + col;  // this lane's query row
  const auto out_at = [&](int row) {  // the four dims 4 quad .. of output tile 0 of query row `row` < TG
    const int t = row / G, h = hk * G + (row - t * G);
    return a.out + ((((int64_t)r * a.T + t) * a.H + h) * DH + 4 * quad) * ES;
  };
  if (qb * QROWS >= n_valid) {  // (block-uniform) a bad row, or a block of padding queries only: NaN / zeros, no barrier met
    if (qr < TG) {
      const float f = bad ? __builtin_nanf("") : 0.0f;
      const float z[4] = {f, f, f, f};
      char *o = out_at(qr);
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) store4<DT>(o + dt * 16 * ES, z);
    }
    return;
  }
  // ---- from here on: 0 <= pos, 1 <= nn <= T, pos + nn <= cap, 0 <= sr < n_slab_rows
  const int last_q = n_valid - 1;
  const int qrc = qr < last_q ? qr : last_q;  // padded rows work on the last valid query
  const int t_q = qrc / G, h_q = hk * G + (qrc - t_q * G);
  const int fr0 = qb * QROWS + wave * 16;
  const int t_lo = (fr0 < last_q ? fr0 : last_q) / G, t_hi = (fr0 + 15 < last_q ? fr0 + 15 : last_q) / G;  // the fragment's tokens
  const int t_blk = (qb * QROWS + QROWS - 1 < last_q ? qb * QROWS + QROWS - 1 : last_q) / G;                // the block's last token
  const int kend = pos + t_blk + 1;  // the block reads keys 0 .. kend - 1 (kend <= pos + nn <= cap)
  const int n_tiles = (kend + KT - 1) / KT;
  const bool append = qb == last_q / QROWS;  // this block meets every new position (t_blk = nn - 1): it writes them to the slab
  const int lim = pos + t_q;                 // the last key this lane's query sees

  // the fragment's Q operand: lane (col, quad) holds dims 32 c + 8 quad .. (16-bit) / 16 c + 4 quad .. (float32) of its query
  u32x4 qv[NQ];
  {
    const char *qp = a.q + ((int64_t)r * a.q_sr + (int64_t)h_q * a.q_sh + (int64_t)t_q * a.q_sp) * ES;
#pragma unroll
    for (int c = 0; c < NQ; ++c) qv[c] = *reinterpret_cast<const u32x4 *>(qp + (c * 4 + quad) * 16);
  }
  const int64_t slab_row = (sr * a.Hkv + hk) * a.cap;
  const char *kn = a.k_new + ((int64_t)r * a.k_sr + (int64_t)hk * a.k_sh) * ES;
  const char *vn = a.v_new + ((int64_t)r * a.v_sr + (int64_t)hk * a.v_sh) * ES;
  // the 16-byte vector `ch` of key position p (< kend after the clamp) of K or V; a new position is appended on the way
  const auto fetch = [&](char *slab, const char *fresh, int64_t sp, int p, int ch) {
    const int pc = p < kend ? p : kend - 1;
    if (pc < pos) return *reinterpret_cast<const u32x4 *>(slab + ((slab_row + pc) * DH) * ES + ch * 16);
    const u32x4 v = *reinterpret_cast<const u32x4 *>(fresh + (int64_t)(pc - pos) * sp * ES + ch * 16);
    if (append && p < kend) *reinterpret_cast<u32x4 *>(slab + ((slab_row + p) * DH) * ES + ch * 16) = v;
    return v;
  };
  const int vkey = S::v_key(tid), vch = tid % VPR;  // 16-bit V: this thread's two keys of a tile and its chunk of them
  u32x4 kreg[NK], vreg[NV];
  const auto load_tile = [&](int tile0) {
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      const int x = tid + i * THREADS, key = x / VPR, ch = x - key * VPR;
      kreg[i] = fetch(a.k_slab, kn, a.k_sp, tile0 + key, ch);
      if constexpr (F32) vreg[i] = fetch(a.v_slab, vn, a.v_sp, tile0 + key, ch);
    }
    if constexpr (!F32) {
      if (tid < (KT / 2) * VPR) {
        vreg[0] = fetch(a.v_slab, vn, a.v_sp, tile0 + vkey, vch);
        vreg[1] = fetch(a.v_slab, vn, a.v_sp, tile0 + vkey + 1, vch);
      }
    }
  };
  float m = -__builtin_huge_valf(), l = 0.0f;  // the lane's query: running maximum (the same in its four lanes); the lane's share of the sum
  f32x4 o[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  load_tile(0);
  for (int tile = 0; tile < n_tiles; ++tile) {
    const int tile0 = tile * KT;
    __syncthreads();  // every wave is done with the tile before
    stage_tile<DT, DH>(k_lds, v_lds, kreg, vreg, tid);
    __syncthreads();
    if (tile + 1 < n_tiles) load_tile(tile0 + KT);  // travels while this tile is worked on
    if (tile0 > pos + t_hi) continue;               // (wave-uniform) wholly behind the fragment; tile 0 never is
    // ---- S^T = K . Q^T: s[half][v] = score of key tile0 + 16 half + 4 quad + v for this lane's query
    f32x4 s[2];
    tile_scores<DT, DH>(k_lds, qv, s, col, quad);
    // ---- online softmax on the accumulator layout
    const bool full = tile0 + KT - 1 <= pos + t_lo;  // (wave-uniform) every key of the tile is seen by every query of the fragment
    float p[8], tm = -__builtin_huge_valf();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float x = s[i >> 2][i & 3] * a.scale;
      if (!full && tile0 + 16 * (i >> 2) + 4 * quad + (i & 3) > lim) x = -__builtin_huge_valf();
      p[i] = x;
      tm = fmaxf(tm, x);
    }
    tm = fmaxf(tm, __shfl_xor(tm, 16, 64));
    tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
    const float m2 = fmaxf(m, tm);      // finite: tile 0 holds key 0, which every query sees
    const float c = __expf(m - m2);     // (tile 0: exp(-inf) = 0)
    float ps = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      p[i] = __expf(p[i] - m2);
      ps += p[i];
    }
    l = l * c + ps;
    m = m2;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) o[dt] *= c;
    // ---- O^T += V^T . P^T: o[dt][v] = dim 16 dt + 4 quad + v of this lane's query
    tile_pv<DT, DH>(v_lds, p, o, col, quad);
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (qr < TG) {
    const float inv = qr < n_valid ? 1.0f / l : 0.0f;  // a padded query: zeros
    char *op = out_at(qr);
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) {
      const float y[4] = {o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv};
      store4<DT>(op + dt * 16 * ES, y);
    }
  }
}

}  // namespace

extern "C" int glb_slab_attention_tile(const void *q, const int64_t q_strides[3], const void *k_new, const int64_t k_strides[3],
                                       const void *v_new, const int64_t v_strides[3], void *k_slab, void *v_slab,
                                       const int32_t *pos, const int32_t *n_new, const int32_t *row_of, int64_t n_rows,
                                       int64_t n_slab_rows, int64_t heads, int64_t kv_heads, int64_t cap, int64_t head_dim,
                                       int64_t max_new, float scale, int32_t dtype, void *out, void *stream) {
  TileArgs a{};
  if (const int rc = fill_chunk_args("glb_slab_attention_tile", GLB_KV_TILE_MAX, kTileHeadDims, q, q_strides, k_new, k_strides, v_new,
                                     v_strides, k_slab, v_slab, pos, n_new, row_of, n_rows, n_slab_rows, heads, kv_heads, cap, head_dim,
                                     max_new, scale, dtype, out, a))
    return rc;
  // one workgroup per (row, KV head, block of QROWS query rows): bounded factors first, then their product
  if (n_rows > 0x7fffffffll || heads > 0xffffffll) return glb::api_fail(GLB_EINVAL, "glb_slab_attention_tile: bad sizes");
  const int64_t q_blocks = (max_new * (heads / kv_heads) + QROWS - 1) / QROWS;
  if (n_rows * kv_heads * q_blocks > 0x7fffffffll) return glb::api_fail(GLB_EINVAL, "glb_slab_attention_tile: bad sizes");
  a.QB = (int32_t)q_blocks;
  const dim3 grid((unsigned)(n_rows * kv_heads * q_blocks));
  const hipError_t e = launch_attention_form(kTileHeadDims, dtype, head_dim, [&](auto dt, auto dh) {
    hipLaunchKernelGGL((slab_attention_tile_kernel<decltype(dt)::value, decltype(dh)::value>), grid, dim3(THREADS), 0, (hipStream_t)stream, a);
  });
  if (e != hipSuccess) return glb::api_hip_fail(e, "slab_attention_tile launch");
  return GLB_OK;
}
