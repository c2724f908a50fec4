// glb_attn_batch.hip - glb_batch_attention_tile (include/glb.h): masked attention of a padded batch of contexts
// of any length - glb_short_attention's contract without its bound on q_len * k_len.  That kernel is one wave per (row, head,
// query) and every wave walks its keys alone; here the K / V of a (row, KV head) come on chip once per 64 queries and both
// products run on MFMA: the tile, its way into LDS and the products are glb_attn_mfma.hpp's, shared with glb_attn_tile.hip.
//
// Work split.  A workgroup of 4 waves serves (row, KV head, block of 64 query rows); query row qr = t * G + g is query
// position t under query head hk * G + g (t-major), a wave owns one 16-row fragment and lane (col = lane & 15,
// quad = lane >> 4) belongs to query row col of it in everything: operand, mask bits, scores, softmax state, output.
//
// Keys are positions 0 .. k_len - 1 of the row's own K / V, read by the caller's strides where the projection (or a gathered
// prefix cache) left them: no slab, nothing appended.  Every address is formed from host integers and loop counters below
// k_len; a mask byte is only ever compared with zero.
//
// Visibility.  Before its key loop the block scans the mask rows of its queries (at most 64 positions t) - single bytes up
// to the first 16-byte boundary of a row, aligned 16-byte loads from there, single bytes behind the last whole vector: the
// mask pointer and strides need no alignment and no byte outside a row is read - for the first and the last key any of them
// sees, and loops over the tiles of 32 keys in that range only: left padding and the causal upper triangle cost nothing.
// A null mask means causal, key s <= t + k_len - q_len: the range follows from the block's last t.  Per tile a lane reads
// the eight mask bytes of its own query's keys (with the tile's K / V, a tile ahead) into eight bits; a wave-wide vote then
// takes one of three ways: all visible - no per-element select; none - the fragment skips the tile's MFMAs; mixed - -inf per
// hidden element.  The causal form computes the same eight bits from t.
//
// The -inf rule.  A general mask can hide the first tiles from a query, so its running maximum m can still be -inf when a
// tile is folded: the exponentials are then taken against 0 instead - exp(-inf - 0) = 0 for the rescale and for every
// probability, never exp(-inf - -inf).  A query whose sum ends at 0 saw nothing: it stores zeros (glb_short_attention's rule
// for padding queries).  Padded query rows (qr >= q_len G) compute on the block's last valid query and store nothing.
//
// No atomics, no workspace, writes `out` only: fit for a captured graph.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/glb.h"
#include "glb_attn.hpp"
#include "glb_attn_host.hpp"
#include "glb_attn_mfma.hpp"
#include "glb_common.hpp"

namespace {

struct BatchArgs {
  const char *q, *k, *v;
  const uint8_t *mask;  // null: causal
  char *out;
  int64_t q_sr, q_sh, q_sp, k_sr, k_sh, k_sp, v_sr, v_sh, v_sp;  // element strides: row, head, position
  int64_t m_sr, m_sq;                                            // byte strides of the mask: row, query
  int32_t H, Hkv, Lq, Lk, QB;                                    // QB: query blocks of a (row, KV head)
  float scale;
};

// the first and last nonzero byte of mask row `row` [0, n), found by one wave: lo > hi when there is none
__device__ __forceinline__ void scan_mask_row(const uint8_t *row, int n, int lane, int &lo, int &hi) {
  const int head_all = (int)((16 - ((uintptr_t)row & 15)) & 15);
  const int head = head_all < n ? head_all : n;  // single bytes up to the first 16-byte boundary
  const int n_vec = (n - head) >> 4, tail0 = head + (n_vec << 4);
  const auto see = [&](int s) {
    lo = s < lo ? s : lo;
    hi = s > hi ? s : hi;
  };
  if (lane < head && row[lane]) see(lane);
  for (int i = lane; i < n_vec; i += 64) {
    const u32x4 w = *reinterpret_cast<const u32x4 *>(row + head + (i << 4));
    const uint32_t x[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x[j]) {
        const int base = head + (i << 4) + 4 * j;
        see(base + (__builtin_ctz(x[j]) >> 3));
        see(base + 3 - (__builtin_clz(x[j]) >> 3));
      }
  }
  if (tail0 + lane < n && row[tail0 + lane]) see(tail0 + lane);  // fewer than 16 bytes are left
}

template <int DT, int DH>
__global__ __launch_bounds__(THREADS) void batch_attention_tile_kernel(const BatchArgs a) {
  using S = TileShape<DT, DH>;
  constexpr bool F32 = S::F32;
  constexpr int ES = S::ES, VPR = S::VPR, NQ = S::NQ, NK = S::NK, NV = S::NV, ND = S::ND;
  __shared__ __attribute__((aligned(16))) char k_lds[S::K_BYTES];
  __shared__ __attribute__((aligned(16))) char v_lds[S::V_BYTES];
  __shared__ int range_lds[8];  // the four waves' first / last visible key
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
  const int qb = blockIdx.x % a.QB, rk = blockIdx.x / a.QB, hk = rk % a.Hkv, r = rk / a.Hkv;
  const int G = a.H / a.Hkv, TG = a.Lq * G, off = a.Lk - a.Lq;
  const int last_q = TG - 1;
  const int qr = qb * QROWS + wave * 16 + col;  // this lane's query row
  const int qrc = qr < last_q ? qr : last_q;    // padded rows work on the last valid query
  const int t_q = qrc / G, h_q = hk * G + (qrc - t_q * G);
  const int t_first = qb * QROWS / G, t_last = (qb * QROWS + QROWS - 1 < last_q ? qb * QROWS + QROWS - 1 : last_q) / G;  // the block's positions
  const uint8_t *mrow = a.mask ? a.mask + (int64_t)r * a.m_sr + (int64_t)t_q * a.m_sq : nullptr;  // this lane's query's mask row
  const int lim = t_q + off;  // causal: the last key this lane's query sees

  // ---- the keys the block's queries see: [kmin, kmax]
  int kmin = 0, kmax = t_last + off;
  if (a.mask) {
    int lo = a.Lk, hi = -1;
    for (int t = t_first + wave; t <= t_last; t += 4)
      scan_mask_row(a.mask + (int64_t)r * a.m_sr + (int64_t)t * a.m_sq, a.Lk, lane, lo, hi);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int lo2 = __shfl_xor(lo, d, 64), hi2 = __shfl_xor(hi, d, 64);
      lo = lo2 < lo ? lo2 : lo;
      hi = hi2 > hi ? hi2 : hi;
    }
    if (lane == 0) range_lds[wave] = lo, range_lds[4 + wave] = hi;
    __syncthreads();
    kmin = range_lds[0], kmax = range_lds[4];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      kmin = range_lds[w] < kmin ? range_lds[w] : kmin;
      kmax = range_lds[4 + w] > kmax ? range_lds[4 + w] : kmax;
    }
  }
  const auto out_at = [&](int row) {  // the four dims 4 quad .. of output tile 0 of query row `row` < TG
    const int t = row / G, h = hk * G + (row - t * G);
    return a.out + ((((int64_t)r * a.Lq + t) * a.H + h) * DH + 4 * quad) * ES;
  };
  if (kmin > kmax) {  // (block-uniform) padding queries only: zeros
    if (qr < TG) {
      const float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      char *o = out_at(qr);
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) store4<DT>(o + dt * 16 * ES, z);
    }
    return;
  }
  // ---- from here on 0 <= kmin <= kmax < Lk
  const int tile_lo = kmin / KT, tile_hi = kmax / KT;

  u32x4 qv[NQ];  // the fragment's Q operand (tile_scores)
  {
    const char *qp = a.q + ((int64_t)r * a.q_sr + (int64_t)h_q * a.q_sh + (int64_t)t_q * a.q_sp) * ES;
#pragma unroll
    for (int c = 0; c < NQ; ++c) qv[c] = *reinterpret_cast<const u32x4 *>(qp + (c * 4 + quad) * 16);
  }
  const char *kb = a.k + ((int64_t)r * a.k_sr + (int64_t)hk * a.k_sh) * ES;
  const char *vb = a.v + ((int64_t)r * a.v_sr + (int64_t)hk * a.v_sh) * ES;
  // the 16-byte vector `ch` of key position p; positions past the last visible key are read from that key and masked
  const auto fetch = [&](const char *base, int64_t sp, int p, int ch) {
    const int pc = p < kmax ? p : kmax;
    return *reinterpret_cast<const u32x4 *>(base + (int64_t)pc * sp * ES + ch * 16);
  };
  const int vkey = S::v_key(tid), vch = tid % VPR;  // 16-bit V: this thread's two keys of a tile and its chunk of them
  u32x4 kreg[NK], vreg[NV];
  const auto load_tile = [&](int tile0) {
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      const int x = tid + i * THREADS, key = x / VPR, ch = x - key * VPR;
      kreg[i] = fetch(kb, a.k_sp, tile0 + key, ch);
      if constexpr (F32) vreg[i] = fetch(vb, a.v_sp, tile0 + key, ch);
    }
    if constexpr (!F32) {
      if (tid < (KT / 2) * VPR) {
        vreg[0] = fetch(vb, a.v_sp, tile0 + vkey, vch);
        vreg[1] = fetch(vb, a.v_sp, tile0 + vkey + 1, vch);
      }
    }
  };
  // bit i: this lane's query sees key tile0 + 16 (i >> 2) + 4 quad + (i & 3) - the accumulator layout of tile_scores
  const auto load_visible = [&](int tile0) {
    uint32_t bits = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int s = tile0 + 16 * (i >> 2) + 4 * quad + (i & 3);
      bool vis;
      if (mrow) vis = s <= kmax && mrow[s] != 0;
      else vis = s <= lim;
      bits |= (vis ? 1u : 0u) << i;
    }
    return bits;
  };

  float m = -__builtin_huge_valf(), l = 0.0f;  // the lane's query: running maximum (the same in its four lanes); the lane's share of the sum
  f32x4 o[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  load_tile(tile_lo * KT);
  uint32_t vis_next = load_visible(tile_lo * KT);
  for (int tile = tile_lo; tile <= tile_hi; ++tile) {
    const int tile0 = tile * KT;
    const uint32_t vis = vis_next;
    __syncthreads();  // every wave is done with the tile before
    stage_tile<DT, DH>(k_lds, v_lds, kreg, vreg, tid);
    __syncthreads();
    if (tile < tile_hi) {  // travel while this tile is worked on
      load_tile(tile0 + KT);
      vis_next = load_visible(tile0 + KT);
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
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (qr < TG) {
    const float inv = l > 0.0f ? 1.0f / l : 0.0f;  // a query that saw nothing: zeros
    char *op = out_at(qr);
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) {
      const float y[4] = {o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv};
      store4<DT>(op + dt * 16 * ES, y);
    }
  }
}

}  // namespace

extern "C" int glb_batch_attention_tile(const void *q, const int64_t q_strides[3], const void *k, const int64_t k_strides[3],
                                        const void *v, const int64_t v_strides[3], const uint8_t *mask, int64_t mask_stride_row,
                                        int64_t mask_stride_query, int64_t n_rows, int64_t heads, int64_t kv_heads, int64_t q_len,
                                        int64_t k_len, int64_t head_dim, float scale, int32_t dtype, void *out, void *stream) {
  const char *entry = "glb_batch_attention_tile";
  if (!q || !k || !v || !out || !q_strides || !k_strides || !v_strides) return glb::api_fail(GLB_EINVAL, "%s: null pointer", entry);
  if (const int rc = check_dtype(dtype)) return rc;
  if (n_rows <= 0 || heads <= 0 || kv_heads <= 0 || heads % kv_heads || n_rows > 0x7fffffffll || heads > 0xffffffll)
    return glb::api_fail(GLB_EINVAL, "%s: bad sizes", entry);
  if (q_len < 1 || k_len < q_len || k_len > GLB_BATCH_ATTENTION_MAX_KEYS)
    return glb::api_fail(GLB_EINVAL, "%s: q_len %lld, k_len %lld (1 <= q_len <= k_len <= %d)", entry, (long long)q_len, (long long)k_len,
                         GLB_BATCH_ATTENTION_MAX_KEYS);
  if (mask && (mask_stride_row < 0 || mask_stride_query < 0)) return glb::api_fail(GLB_EINVAL, "%s: negative mask stride", entry);
  if (const int rc = check_head_dim_and_alignment(
          entry, kTileHeadDims, dtype, head_dim, {q, k, v, out},
          {q_strides[0], q_strides[1], q_strides[2], k_strides[0], k_strides[1], k_strides[2], v_strides[0], v_strides[1], v_strides[2]}))
    return rc;
  // one workgroup per (row, KV head, block of QROWS query rows): bounded factors above, then their product
  const int64_t q_blocks = (q_len * (heads / kv_heads) + QROWS - 1) / QROWS;
  if (n_rows * kv_heads * q_blocks > 0x7fffffffll) return glb::api_fail(GLB_EINVAL, "%s: bad sizes", entry);
  BatchArgs a{};
  a.q = (const char *)q;
  a.k = (const char *)k;
  a.v = (const char *)v;
  a.mask = mask;
  a.out = (char *)out;
  a.q_sr = q_strides[0], a.q_sh = q_strides[1], a.q_sp = q_strides[2];
  a.k_sr = k_strides[0], a.k_sh = k_strides[1], a.k_sp = k_strides[2];
  a.v_sr = v_strides[0], a.v_sh = v_strides[1], a.v_sp = v_strides[2];
  a.m_sr = mask_stride_row, a.m_sq = mask_stride_query;
  a.H = (int32_t)heads;
  a.Hkv = (int32_t)kv_heads;
  a.Lq = (int32_t)q_len;
  a.Lk = (int32_t)k_len;
  a.QB = (int32_t)q_blocks;
  a.scale = scale;
  const dim3 grid((unsigned)(n_rows * kv_heads * q_blocks));
  const hipError_t e = launch_attention_form(kTileHeadDims, dtype, head_dim, [&](auto dt, auto dh) {
    hipLaunchKernelGGL((batch_attention_tile_kernel<decltype(dt)::value, decltype(dh)::value>), grid, dim3(THREADS), 0, (hipStream_t)stream, a);
  });
  if (e != hipSuccess) return glb::api_hip_fail(e, "batch_attention_tile launch");
  return GLB_OK;
}
