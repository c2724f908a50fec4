// glb_attn_packed_tile.hip - glb_packed_row_map and glb_packed_attention_tile (include/glb.h): attention over a
// ROW-PACKED batch whose contexts share the rows of their prompt - glb_short_attention_packed's plan without its bound of 32
// keys.  That kernel is one wave per (segment, KV head) and every wave brings its prompt's K / V on chip again; here the tile,
// its way into LDS and the two MFMA products are glb_attn_mfma.hpp's (shared with glb_attn_tile.hip and glb_attn_batch.hip),
// and the work is split over PACKED ROWS, not over segments.
//
// Work split.  A workgroup of 4 waves serves (block of 64 query rows, KV head); query row qr = row * G + g is packed row `row`
// under query head hk * G + g (row-major), so a block holds the tails of several contexts at once (GPT-2 heads, 3-token
// tails: 21 contexts), or part of one long tail or prompt.  A wave owns one 16-row fragment and lane (col = lane & 15,
// quad = lane >> 4) belongs to query row col of it in everything: operand, visibility bits, scores, softmax state, output.
//
// Row map.  glb_packed_row_map turns the plan into one int32x4 per packed row, once per forward: (seg_start, pre_start,
// pre_len, named).  The attention kernel reads its rows' entries and checks every one against n_rows itself (the map is device
// data): 0 <= seg_start <= row, pre_start >= 0, pre_len >= 0, pre_start + pre_len <= n_rows, or the row counts as unnamed -
// it sees nothing and stores nothing.  Every address below is formed from integers that passed these checks.
//
// The keys of query row r come in two kinds, and the block walks them in passes of the same tile loop (`walk`): keys are the
// packed rows start .. last, 32 a tile, and a lane sees key s where lo <= s <= hi for its own two integers.
//   shared keys (phase A)  the prompt rows pre_start .. pre_start + pre_len - 1: all visible.  The block picks the smallest
//     (pre_start, pre_len) above the one it served last by a reduction over its 256 lanes and walks that range once for every
//     query that names it - no mask, full MFMA rows, the prompt's K / V on chip once per 64 queries; lanes of another range
//     see nothing in that pass (lo > hi), a fragment without a matching lane skips the MFMAs.  One prompt: one pass.
//   own keys (phase B)     the segment's own rows seg_start .. r: a block-diagonal causal band in packed-row space.  One walk
//     from the smallest seg_start among the block's rows to its last named row, lo = seg_start, hi = r.  A prompt segment
//     (pre_len = 0) is served by this phase alone.
// Per tile a wave-wide vote takes one of §35's three ways: all visible - no select; none - skip; mixed - -inf per element.
// Online softmax makes the order of the passes irrelevant; §35's -inf rule holds: while a query's maximum is still -inf the
// exponentials are taken against 0.  A named query always sees its own row, so its sum is positive.
//
// K / V tiles travel a tile ahead in the 256 threads' registers; a key position past `last` is read from row `last` (a row
// below n_rows) and masked.  No atomics, no workspace, writes `out` only: fit for a captured graph.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/glb.h"
#include "glb_attn.hpp"
#include "glb_attn_host.hpp"
#include "glb_attn_mfma.hpp"
#include "glb_common.hpp"

namespace {

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr int MAP_THREADS = 256;

// ---- the row map ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MAP_THREADS) void packed_row_map_clear_kernel(i32x4 *row_map, int32_t M) {
  const int64_t r = (int64_t)blockIdx.x * MAP_THREADS + threadIdx.x;
  if (r < M) row_map[r] = i32x4{0, 0, 0, 0};  // every row starts unnamed
}

// one workgroup per segment: glb_short_attention_packed's rule - a segment that is not followed names no row and counts
__global__ __launch_bounds__(MAP_THREADS) void packed_row_map_kernel(const int32_t *plan, int32_t M, int32_t max_keys, i32x4 *row_map,
                                                                     uint32_t *err) {
  const int32_t *seg = plan + (int64_t)blockIdx.x * 4;
  const int64_t pre_start = seg[0], pre_len = seg[1], tail_start = seg[2], tail_len = seg[3];
  // (block-uniform)
  if (pre_len < 0 || tail_len < 1 || pre_len + tail_len > max_keys || pre_start < 0 || pre_start + pre_len > M || tail_start < 0 ||
      tail_start + tail_len > M) {
    if (threadIdx.x == 0) atomicAdd(err, 1u);
    return;
  }
  const i32x4 e{(int32_t)tail_start, (int32_t)pre_start, (int32_t)pre_len, 1};
  for (int64_t t = threadIdx.x; t < tail_len; t += MAP_THREADS) row_map[tail_start + t] = e;  // tail_start + t < M
}

// ---- the attention ----------------------------------------------------------------------------------------------------------
struct PackedTileArgs {
  const char *q, *k, *v;
  char *out;
  const i32x4 *row_map;                        // [M]
  int64_t q_sr, q_sh, k_sr, k_sh, v_sr, v_sh;  // element strides: packed row, head
  int32_t M, H, Hkv;
  float scale;
};

// the smallest x of the block's 256 lanes; `red`: four words of LDS, free again on return
__device__ __forceinline__ u64 block_min(u64 x, u64 *red, int wave, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u64 y = __shfl_xor(x, d, 64);
    x = y < x ? y : x;
  }
  if (lane == 0) red[wave] = x;
  __syncthreads();
  u64 r = red[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) r = red[w] < r ? red[w] : r;
  __syncthreads();
  return r;
}

template <int DT, int DH>
__global__ __launch_bounds__(THREADS) void packed_attention_tile_kernel(const PackedTileArgs a) {
  using S = TileShape<DT, DH>;
  constexpr bool F32 = S::F32;
  constexpr int ES = S::ES, VPR = S::VPR, NQ = S::NQ, NK = S::NK, NV = S::NV, ND = S::ND;
  constexpr int NONE = 0x7fffffff;
  __shared__ __attribute__((aligned(16))) char k_lds[S::K_BYTES];
  __shared__ __attribute__((aligned(16))) char v_lds[S::V_BYTES];
  __shared__ u64 red_lds[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
  const int hk = blockIdx.x % a.Hkv, qb = blockIdx.x / a.Hkv;
  const int G = a.H / a.Hkv;
  const int qr = qb * QROWS + wave * 16 + col;  // this lane's query row (the host bounds M G + 64 below 2^31)
  const int row_q = qr / G, h_q = hk * G + (qr - row_q * G);
  const int rowc = row_q < a.M ? row_q : a.M - 1;  // a row past the batch reads the last row's query and stores nothing

  // ---- this lane's row of the map, checked: lo_own .. hi_own are its own keys, pre0 .. pre0 + pre_n - 1 the shared ones
  int lo_own = NONE, hi_own = -1, pre0 = 0, pre_n = 0;
  if (row_q < a.M) {
    const i32x4 e = a.row_map[row_q];
    if (e.w != 0 && e.x >= 0 && e.x <= row_q && e.y >= 0 && e.z >= 0 && (int64_t)e.y + e.z <= a.M)
      lo_own = e.x, hi_own = row_q, pre0 = e.y, pre_n = e.z;
  }
  const bool named = hi_own >= 0;
  const u64 my_range = pre_n > 0 ? ((u64)(uint32_t)pre0 << 32) | (uint32_t)pre_n : ~0ull;  // (pre_n >= 1: never 0)

  u32x4 qv[NQ];  // the fragment's Q operand (tile_scores)
  {
    const char *qp = a.q + ((int64_t)rowc * a.q_sr + (int64_t)h_q * a.q_sh) * ES;
#pragma unroll
    for (int c = 0; c < NQ; ++c) qv[c] = *reinterpret_cast<const u32x4 *>(qp + (c * 4 + quad) * 16);
  }
  const char *kb = a.k + (int64_t)hk * a.k_sh * ES;
  const char *vb = a.v + (int64_t)hk * a.v_sh * ES;
  const int vkey = S::v_key(tid), vch = tid % VPR;  // 16-bit V: this thread's two keys of a tile and its chunk of them
  u32x4 kreg[NK], vreg[NV];
  // the tile of packed rows tile0 .. tile0 + 31; rows past `last` (< M) are read from row `last` and masked
  const auto load_tile = [&](int tile0, int last) {
    const auto fetch = [&](const char *base, int64_t sr, int p, int ch) {
      const int pc = p < last ? p : last;
      return *reinterpret_cast<const u32x4 *>(base + (int64_t)pc * sr * ES + ch * 16);
    };
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      const int x = tid + i * THREADS, key = x / VPR, ch = x - key * VPR;
      kreg[i] = fetch(kb, a.k_sr, tile0 + key, ch);
      if constexpr (F32) vreg[i] = fetch(vb, a.v_sr, tile0 + key, ch);
    }
    if constexpr (!F32) {
      if (tid < (KT / 2) * VPR) {
        vreg[0] = fetch(vb, a.v_sr, tile0 + vkey, vch);
        vreg[1] = fetch(vb, a.v_sr, tile0 + vkey + 1, vch);
      }
    }
  };

  float m = -__builtin_huge_valf(), l = 0.0f;  // the lane's query: running maximum (the same in its four lanes); the lane's share of the sum
  f32x4 o[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- phase B's range: the smallest seg_start and the last row among the block's named rows
  const int own_start = (int)block_min((u64)(uint32_t)lo_own, red_lds, wave, lane);
  const u64 last_from_top = block_min(named ? (u64)(uint32_t)(NONE - hi_own) : ~0ull, red_lds, wave, lane);
  if (last_from_top == ~0ull) return;  // (block-uniform) no named row: nothing is written
  const int own_last = NONE - (int)last_from_top;  // own_start <= own_last: a named row's seg_start is at most the row

  u64 served = 0;  // the last shared range walked; ranges are walked in ascending order of (pre_start, pre_len)
  for (bool own = false; !own;) {
    // ---- the pass: keys start .. last (0 <= start <= last < M), this lane sees lo <= s <= hi
    int start, last, lo, hi;
    const u64 next = block_min(my_range > served ? my_range : ~0ull, red_lds, wave, lane);
    if (next != ~0ull) {  // (block-uniform) phase A: one more shared range
      served = next;
      start = (int)(next >> 32), last = start + (int)(uint32_t)next - 1;
      const bool mine = my_range == next;
      lo = mine ? start : NONE, hi = mine ? last : -1;
    } else {  // phase B, the last pass
      own = true;
      start = own_start, last = own_last, lo = lo_own, hi = hi_own;
    }
    load_tile(start, last);
    for (int tile0 = start; tile0 <= last; tile0 += KT) {
      __syncthreads();  // every wave is done with the tile before
      stage_tile<DT, DH>(k_lds, v_lds, kreg, vreg, tid);
      __syncthreads();
      if (tile0 + KT <= last) load_tile(tile0 + KT, last);  // travel while this tile is worked on
      // bit i: this lane's query sees key tile0 + 16 (i >> 2) + 4 quad + (i & 3) - the accumulator layout of tile_scores
      uint32_t vis = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int s = tile0 + 16 * (i >> 2) + 4 * quad + (i & 3);
        vis |= (s >= lo && s <= hi ? 1u : 0u) << i;
      }
      if (!__any(vis != 0)) continue;  // (wave-uniform) no query of the fragment sees a key of the tile
      f32x4 s[2];
      tile_scores<DT, DH>(k_lds, qv, s, col, quad);
      // ---- online softmax on the accumulator layout
      const bool full = __all(vis == 0xffu);  // (wave-uniform) every query of the fragment sees every key of the tile
      float p[8], tm = -__builtin_huge_valf();
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float x = s[i >> 2][i & 3] * a.scale;
        if (!full && !((vis >> i) & 1u)) x = -__builtin_huge_valf();
        p[i] = x;
        tm = fmaxf(tm, x);
      }
      tm = fmaxf(tm, __shfl_xor(tm, 16, 64));
      tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
      const float m2 = fmaxf(m, tm);
      const float mref = m2 == -__builtin_huge_valf() ? 0.0f : m2;  // a query that has seen nothing yet: exponentials against 0, all 0
      const float c = __expf(m - mref);
      float ps = 0.0f;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        p[i] = __expf(p[i] - mref);
        ps += p[i];
      }
      l = l * c + ps;
      m = m2;
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) o[dt] *= c;
      tile_pv<DT, DH>(v_lds, p, o, col, quad);
    }
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (named) {
    const float inv = l > 0.0f ? 1.0f / l : 0.0f;
    char *op = a.out + (((int64_t)row_q * a.H + h_q) * DH + 4 * quad) * ES;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) {
      const float y[4] = {o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv};
      store4<DT>(op + dt * 16 * ES, y);
    }
  }
}

}  // namespace

extern "C" int glb_packed_row_map(const int32_t *plan, int64_t n_segments, int64_t n_rows, int64_t max_keys, int32_t *row_map,
                                  uint32_t *err_word, void *stream) {
  const char *entry = "glb_packed_row_map";
  if (!plan || !row_map || !err_word) return glb::api_fail(GLB_EINVAL, "%s: null pointer", entry);
  if (n_segments <= 0 || n_rows <= 0 || n_segments > 0x7fffffffll || n_rows > 0x7fffffffll) return glb::api_fail(GLB_EINVAL, "%s: bad sizes", entry);
  if (max_keys < 1 || max_keys > GLB_PACKED_ATTENTION_MAX_KEYS)
    return glb::api_fail(GLB_EINVAL, "%s: %lld keys per context (1 .. %d are served)", entry, (long long)max_keys, GLB_PACKED_ATTENTION_MAX_KEYS);
  if ((uintptr_t)plan % 16 || (uintptr_t)row_map % 16 || (uintptr_t)err_word % 4)
    return glb::api_fail(GLB_EINVAL, "%s: plan and row_map must be 16-byte aligned, the error word 4-byte", entry);
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(packed_row_map_clear_kernel, dim3(blocks_for(n_rows, MAP_THREADS)), dim3(MAP_THREADS), 0, s, (i32x4 *)row_map, (int32_t)n_rows);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return glb::api_hip_fail(e, "packed_row_map clear launch");
  hipLaunchKernelGGL(packed_row_map_kernel, dim3((unsigned)n_segments), dim3(MAP_THREADS), 0, s, plan, (int32_t)n_rows, (int32_t)max_keys,
                     (i32x4 *)row_map, err_word);
  e = hipGetLastError();
  if (e != hipSuccess) return glb::api_hip_fail(e, "packed_row_map launch");
  return GLB_OK;
}

extern "C" int glb_packed_attention_tile(const void *q, int64_t q_stride_row, int64_t q_stride_head, const void *k, int64_t k_stride_row,
                                         int64_t k_stride_head, const void *v, int64_t v_stride_row, int64_t v_stride_head,
                                         const int32_t *row_map, int64_t n_rows, int64_t heads, int64_t kv_heads, int64_t head_dim,
                                         float scale, int32_t dtype, void *out, void *stream) {
  const char *entry = "glb_packed_attention_tile";
  if (!q || !k || !v || !out || !row_map) return glb::api_fail(GLB_EINVAL, "%s: null pointer", entry);
  if (const int rc = check_dtype(dtype)) return rc;
  if (n_rows <= 0 || heads <= 0 || kv_heads <= 0 || heads % kv_heads || heads > 0xffffffll || n_rows > 0x7fffffffll)
    return glb::api_fail(GLB_EINVAL, "%s: bad sizes", entry);
  const auto strides = {q_stride_row, q_stride_head, k_stride_row, k_stride_head, v_stride_row, v_stride_head};
  bool signs = true;  // no negative stride
  for (const int64_t st : strides) signs = signs && st >= 0;
  if (const int rc = check_head_dim_and_alignment(entry, kTileHeadDims, dtype, head_dim, {q, k, v, out, row_map}, strides, signs)) return rc;
  // one workgroup per (block of QROWS query rows, KV head); a query row and a key position past the batch's end stay ints
  const int64_t q_rows = n_rows * (heads / kv_heads), q_blocks = (q_rows + QROWS - 1) / QROWS;
  if (q_rows > 0x7fffffffll - QROWS || q_blocks * kv_heads > 0x7fffffffll) return glb::api_fail(GLB_EINVAL, "%s: bad sizes", entry);
  PackedTileArgs a{};
  a.q = (const char *)q;
  a.k = (const char *)k;
  a.v = (const char *)v;
  a.out = (char *)out;
  a.row_map = (const i32x4 *)row_map;
  a.q_sr = q_stride_row, a.q_sh = q_stride_head;
  a.k_sr = k_stride_row, a.k_sh = k_stride_head;
  a.v_sr = v_stride_row, a.v_sh = v_stride_head;
  a.M = (int32_t)n_rows;
  a.H = (int32_t)heads;
  a.Hkv = (int32_t)kv_heads;
  a.scale = scale;
  const dim3 grid((unsigned)(q_blocks * kv_heads));
  const hipError_t e = launch_attention_form(kTileHeadDims, dtype, head_dim, [&](auto dt, auto dh) {
    hipLaunchKernelGGL((packed_attention_tile_kernel<decltype(dt)::value, decltype(dh)::value>), grid, dim3(THREADS), 0, (hipStream_t)stream, a);
  });
  if (e != hipSuccess) return glb::api_hip_fail(e, "packed_attention_tile launch");
  return GLB_OK;
}
