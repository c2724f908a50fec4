// glb_attn_prefix.hip - glb_slab_attention_prefix (include/glb.h): glb_slab_attention's one-token decode over KV
// slab rows that stand BEHIND A PROMPT STORED ONCE.  Row r attends the prefix_len[prefix_of[r]] positions of its prefix, then
// its own slab positions 0 .. pos[r] - 1, then the new token; the rows hold the tails only.  Two launches, neither clever:
//
// Launch A (prefix_partials_kernel): the prefix part on MFMA, as §36 walks a shared prompt.  A workgroup of 4 waves serves
//   (block of 64 query rows, KV head, split s); query row qr = r * G + g is slab row r under query head hk * G + g, a wave owns
//   one 16-row fragment and lane (col = lane & 15, quad = lane >> 4) belongs to query row col of it throughout (glb_attn_mfma.hpp).
//   Q stays in registers.  The block takes the distinct prefixes its rows name in ascending order (the smallest above the one
//   served last, a reduction over the 256 lanes) and for each walks split s's share of its 32-key tiles, tiles
//   [nt s / S, nt (s + 1) / S) of nt = ceil(len / 32): loaded one tile ahead in registers, staged through LDS (stage_tile),
//   S^T = K Q^T and O^T = V^T P^T (tile_scores, tile_pv; §34's rounding of P).  Lanes whose row names another prefix see
//   nothing in that pass, a fragment without a matching lane skips the MFMAs, keys at or past len are masked; a key position
//   past the prefix's end is read from its last valid key.  Every (row, head, split) gets one float32 partial - running
//   maximum m, sum l, unnormalised O[head_dim] - written by exactly one block; an empty share, a row without a prefix and a
//   bad row write the empty state (m = -inf, l = 0, O = 0), so launch B never reads memory nobody wrote.
// Launch B (prefix_tail_kernel): slab_attention_kernel's wave per (row, query head) - WaveShape, unpack16, slot_score, its
//   position -> slot deal, its online softmax and slot merge, written out again - whose slots first fold the S partials in
//   (slot j takes partials j, j + PP, ...; a lane reads its own dims of O; an empty partial is skipped, so exp(-inf - -inf) is
//   never taken), then walk the own positions and the new token, append, normalise and store.  It validates pos and prefix_of
//   itself.  A row with prefix_of = -1 folds nothing and runs slab_attention_kernel's arithmetic.
//
// Workspace: [n_rows * heads][S] records of head_dim + 4 floats - O, then (m, l, 0, 0) - so that A's stores and B's loads are
// 16-byte vectors.  No atomics, no allocation; writes `out`, the appended slab positions and the workspace only.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/glb.h"
#include "glb_attn.hpp"
#include "glb_attn_host.hpp"
#include "glb_attn_mfma.hpp"
#include "glb_common.hpp"

namespace {

typedef unsigned long long u64;

constexpr int MAX_SPLITS = 8;
constexpr int64_t MAX_PREFIX_CAP = 1 << 30;  // a key position past the end of a tile stays an int

struct PrefixArgs {
  const char *q, *k_new, *v_new;
  char *k_slab, *v_slab, *out;
  const int32_t *pos;
  const char *pk, *pv;                         // [U, Hkv, pcap, DH]
  const int32_t *prefix_len, *prefix_of;       // [U], [R]
  float *ws;                                   // [R * H][S][DH + 4]
  int64_t q_sr, q_sh, k_sr, k_sh, v_sr, v_sh;  // element strides (row, head) of the query, the new K, the new V
  int32_t R, H, Hkv, cap, U, pcap, S;
  float scale;
};

// what both kernels make of a row: 0 .. U - 1 its prefix, -1 none, -2 a bad row (NaN out, nothing appended, no prefix walked)
__device__ __forceinline__ int row_prefix(const PrefixArgs &a, int r) {
  const int p = a.pos[r], pf = a.prefix_of[r];
  return (p < 0 || p >= a.cap || pf >= a.U || pf < -1) ? -2 : pf;
}

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

// ---- launch A -----------------------------------------------------------------------------------------------------------------
template <int DT, int DH>
__global__ __launch_bounds__(THREADS) void prefix_partials_kernel(const PrefixArgs a) {
  using S = TileShape<DT, DH>;
  constexpr bool F32 = S::F32;
  constexpr int ES = S::ES, VPR = S::VPR, NQ = S::NQ, NK = S::NK, NV = S::NV, ND = S::ND;
  __shared__ __attribute__((aligned(16))) char k_lds[S::K_BYTES];
  __shared__ __attribute__((aligned(16))) char v_lds[S::V_BYTES];
  __shared__ u64 red_lds[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, quad = lane >> 4;
  const int split = blockIdx.x % a.S, hk = (blockIdx.x / a.S) % a.Hkv, qb = blockIdx.x / (a.S * a.Hkv);
  const int G = a.H / a.Hkv;
  const int qr = qb * QROWS + wave * 16 + col;  // this lane's query row (the host bounds R G + 64 below 2^31)
  const int row_q = qr / G, h_q = hk * G + (qr - row_q * G);
  const bool in_batch = row_q < a.R;
  const int rowc = in_batch ? row_q : a.R - 1;  // a row past the batch reads the last row's query and stores nothing
  const int pf = in_batch ? row_prefix(a, row_q) : -2;
  const u64 my_key = pf >= 0 ? (u64)pf + 1 : ~0ull;  // (never 0)

  u32x4 qv[NQ];  // the fragment's Q operand (tile_scores)
  {
    const char *qp = a.q + ((int64_t)rowc * a.q_sr + (int64_t)h_q * a.q_sh) * ES;
#pragma unroll
    for (int c = 0; c < NQ; ++c) qv[c] = *reinterpret_cast<const u32x4 *>(qp + (c * 4 + quad) * 16);
  }
  const int vkey = S::v_key(tid), vch = tid % VPR;  // 16-bit V: this thread's two keys of a tile and its chunk of them
  const char *kb = nullptr, *vb = nullptr;          // the running pass's prefix under this KV head
  u32x4 kreg[NK], vreg[NV];
  // the tile of prefix positions tile0 .. tile0 + 31; positions past `last` (< len <= pcap) are read from `last` and masked
  const auto load_tile = [&](int tile0, int last) {
    const auto fetch = [&](const char *base, int p, int ch) {
      const int pc = p < last ? p : last;
      return *reinterpret_cast<const u32x4 *>(base + ((int64_t)pc * DH) * ES + ch * 16);
    };
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      const int x = tid + i * THREADS, key = x / VPR, ch = x - key * VPR;
      kreg[i] = fetch(kb, tile0 + key, ch);
      if constexpr (F32) vreg[i] = fetch(vb, tile0 + key, ch);
    }
    if constexpr (!F32) {
      if (tid < (KT / 2) * VPR) {
        vreg[0] = fetch(vb, tile0 + vkey, vch);
        vreg[1] = fetch(vb, tile0 + vkey + 1, vch);
      }
    }
  };

  float m = -__builtin_huge_valf(), l = 0.0f;  // the lane's query: running maximum (the same in its four lanes); the lane's share of the sum
  f32x4 o[ND];
#pragma unroll
  for (int dt = 0; dt < ND; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (u64 served = 0;;) {  // prefixes are walked in ascending order
    const u64 next = block_min(my_key > served ? my_key : ~0ull, red_lds, wave, lane);
    if (next == ~0ull) break;  // (block-uniform)
    served = next;
    const int p = (int)(next - 1);  // 0 <= p < U: a lane's row_prefix
    int len = a.prefix_len[p];
    len = len < 0 ? 0 : (len < a.pcap ? len : a.pcap);  // device data: 0 .. pcap whatever it says
    const int nt = (len + KT - 1) / KT;
    const int t0 = (int)((int64_t)nt * split / a.S), t1 = (int)((int64_t)nt * (split + 1) / a.S);
    if (t0 >= t1) continue;  // (block-uniform) an empty share; len >= 1 below
    const int start = t0 * KT, end = t1 * KT, last = len - 1;
    const bool mine = my_key == next;
    const int64_t slab = ((int64_t)p * a.Hkv + hk) * a.pcap;
    kb = a.pk + slab * DH * ES;
    vb = a.pv + slab * DH * ES;
    load_tile(start, last);
    for (int tile0 = start; tile0 < end; tile0 += KT) {
      __syncthreads();  // every wave is done with the tile before
      stage_tile<DT, DH>(k_lds, v_lds, kreg, vreg, tid);
      __syncthreads();
      if (tile0 + KT < end) load_tile(tile0 + KT, last);  // travel while this tile is worked on
      // bit i: this lane's query sees key tile0 + 16 (i >> 2) + 4 quad + (i & 3) - the accumulator layout of tile_scores
      uint32_t vis = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int s = tile0 + 16 * (i >> 2) + 4 * quad + (i & 3);
        vis |= (mine && s <= last ? 1u : 0u) << i;
      }
      if (!__any(vis != 0)) continue;  // (wave-uniform) no query of the fragment names this prefix
      f32x4 s[2];
      tile_scores<DT, DH>(k_lds, qv, s, col, quad);
      // ---- online softmax on the accumulator layout
      const bool full = __all(vis == 0xffu);  // (wave-uniform)
      float pr[8], tm = -__builtin_huge_valf();
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float x = s[i >> 2][i & 3] * a.scale;
        if (!full && !((vis >> i) & 1u)) x = -__builtin_huge_valf();
        pr[i] = x;
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
        pr[i] = __expf(pr[i] - mref);
        ps += pr[i];
      }
      l = l * c + ps;
      m = m2;
#pragma unroll
      for (int dt = 0; dt < ND; ++dt) o[dt] *= c;
      tile_pv<DT, DH>(v_lds, pr, o, col, quad);
    }
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  if (in_batch) {  // one record per (row, head, split), this block's alone
    float *rec = a.ws + (((int64_t)row_q * a.H + h_q) * a.S + split) * (DH + 4);
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) *reinterpret_cast<f32x4 *>(rec + 16 * dt + 4 * quad) = o[dt];
    if (quad == 0) *reinterpret_cast<f32x4 *>(rec + DH) = f32x4{m, l, 0.f, 0.f};
  }
}

// ---- launch B -----------------------------------------------------------------------------------------------------------------
template <int DT, int DH>
__global__ __launch_bounds__(64) void prefix_tail_kernel(const PrefixArgs a) {
  using W = WaveShape<DT, DH>;
  constexpr int ES = W::ES, EPV = W::EPV, LP = W::LP, PP = W::PP;
  const int lane = threadIdx.x, j = lane / LP, i = lane - j * LP;
  const int r = blockIdx.x / a.H, h = blockIdx.x - r * a.H;
  const int G = a.H / a.Hkv, hk = h / G;
  int p_new = a.pos[r];  // the token being appended sits at p_new; own positions 0 .. p_new are attended to
  const int pf = row_prefix(a, r);
  const bool bad = pf == -2;  // the caller's bug - no fault, no plausible answer: NaN out, nothing appended
  p_new = p_new < 0 ? 0 : (p_new < a.cap ? p_new : a.cap - 1);
  float qf[EPV], kn[EPV], vn[EPV];
  unpack16<DT>(*reinterpret_cast<const u32x4 *>(a.q + ((int64_t)r * a.q_sr + (int64_t)h * a.q_sh + i * EPV) * ES), qf);
  const u32x4 kn_raw = *reinterpret_cast<const u32x4 *>(a.k_new + ((int64_t)r * a.k_sr + (int64_t)hk * a.k_sh + i * EPV) * ES);
  const u32x4 vn_raw = *reinterpret_cast<const u32x4 *>(a.v_new + ((int64_t)r * a.v_sr + (int64_t)hk * a.v_sh + i * EPV) * ES);
  unpack16<DT>(kn_raw, kn);
  unpack16<DT>(vn_raw, vn);
  const int64_t slab_row = ((int64_t)r * a.Hkv + hk) * a.cap;
  if (h == hk * G && j == 0 && !bad) {  // the append: once per (row, KV head)
    *reinterpret_cast<u32x4 *>(a.k_slab + ((slab_row + p_new) * DH + i * EPV) * ES) = kn_raw;
    *reinterpret_cast<u32x4 *>(a.v_slab + ((slab_row + p_new) * DH + i * EPV) * ES) = vn_raw;
  }
  float m = -__builtin_huge_valf(), l = 0.0f, acc[EPV];
#pragma unroll
  for (int k = 0; k < EPV; ++k) acc[k] = 0.0f;
  // ---- the prefix: slot j folds partials j, j + PP, ... (launch A wrote every record of this row)
  if (pf >= 0) {
    const float *rec0 = a.ws + ((int64_t)r * a.H + h) * a.S * (DH + 4);
    for (int s = j; s < a.S; s += PP) {
      const float *rec = rec0 + (int64_t)s * (DH + 4);
      const f32x4 ml = *reinterpret_cast<const f32x4 *>(rec + DH);
      if (!(ml[1] > 0.0f)) continue;  // an empty partial (m = -inf)
      const float m2 = fmaxf(m, ml[0]), c = m == m2 ? 1.0f : __expf(m - m2), co = ml[0] == m2 ? 1.0f : __expf(ml[0] - m2);
      l = l * c + ml[1] * co;
#pragma unroll
      for (int v = 0; v < EPV / 4; ++v) {
        const f32x4 ov = *reinterpret_cast<const f32x4 *>(rec + i * EPV + 4 * v);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[4 * v + k] = acc[4 * v + k] * c + ov[k] * co;
      }
      m = m2;
    }
  }
  // ---- the own positions and the new token: slab_attention_kernel's walk
  for (int p0 = 0; p0 <= p_new; p0 += PP) {
    const int p = p0 + j;
    float kf[EPV], vf[EPV];
    if (p < p_new) {
      unpack16<DT>(*reinterpret_cast<const u32x4 *>(a.k_slab + ((slab_row + p) * DH + i * EPV) * ES), kf);
      unpack16<DT>(*reinterpret_cast<const u32x4 *>(a.v_slab + ((slab_row + p) * DH + i * EPV) * ES), vf);
    } else {
#pragma unroll
      for (int k = 0; k < EPV; ++k) kf[k] = kn[k], vf[k] = vn[k];
    }
    float s = slot_score<LP, EPV>(qf, kf);
    if (p <= p_new) {
      s *= a.scale;
      const float m2 = fmaxf(m, s), c = __expf(m - m2), w = __expf(s - m2);
      l = l * c + w;
#pragma unroll
      for (int k = 0; k < EPV; ++k) acc[k] = __builtin_fmaf(acc[k], c, w * vf[k]);
      m = m2;
    }
  }
  // merge the PP position slots (lanes i, i + LP, i + 2 LP, ...)
#pragma unroll
  for (int o = LP; o < 64; o <<= 1) {
    const float mo = __shfl_xor(m, o, 64), lo = __shfl_xor(l, o, 64);
    const float m2 = fmaxf(m, mo);
    const float c = m == m2 ? 1.0f : __expf(m - m2), co = mo == m2 ? 1.0f : __expf(mo - m2);  // (-inf - -inf: an empty slot)
    l = l * c + lo * co;
#pragma unroll
    for (int k = 0; k < EPV; ++k) acc[k] = acc[k] * c + __shfl_xor(acc[k], o, 64) * co;
    m = m2;
  }
  if (j == 0) {
    const float inv = bad ? __builtin_nanf("") : 1.0f / l;
#pragma unroll
    for (int k = 0; k < EPV; ++k) acc[k] *= inv;
    *reinterpret_cast<u32x4 *>(a.out + (((int64_t)r * a.H + h) * DH + i * EPV) * ES) = pack16v<DT>(acc);
  }
}

}  // namespace

extern "C" size_t glb_slab_attention_prefix_workspace(int64_t n_rows, int64_t heads, int64_t head_dim, int32_t splits) {
  if (n_rows <= 0 || heads <= 0 || head_dim <= 0 || splits < 1 || splits > MAX_SPLITS || n_rows * heads > 0x7fffffffll) return 0;
  return (size_t)(n_rows * heads) * (size_t)splits * (size_t)(head_dim + 4) * sizeof(float);
}

extern "C" int glb_slab_attention_prefix(const void *q, int64_t q_stride_row, int64_t q_stride_head, const void *k_new,
                                         int64_t k_stride_row, int64_t k_stride_head, const void *v_new, int64_t v_stride_row,
                                         int64_t v_stride_head, void *k_slab, void *v_slab, const int32_t *pos, int64_t n_rows,
                                         int64_t heads, int64_t kv_heads, int64_t cap, int64_t head_dim, float scale, int32_t dtype,
                                         void *out, const void *prefix_k, const void *prefix_v, const int32_t *prefix_len,
                                         const int32_t *prefix_of, int64_t n_prefixes, int64_t prefix_cap, int32_t splits,
                                         void *workspace, size_t workspace_bytes, void *stream) {
  const char *entry = "glb_slab_attention_prefix";
  if (!q || !k_new || !v_new || !k_slab || !v_slab || !pos || !out || !prefix_k || !prefix_v || !prefix_len || !prefix_of || !workspace)
    return glb::api_fail(GLB_EINVAL, "%s: null pointer", entry);
  if (const int rc = check_dtype(dtype)) return rc;
  if (n_rows <= 0 || heads <= 0 || kv_heads <= 0 || cap <= 0 || heads % kv_heads || n_rows * heads > 0x7fffffffll || cap > 0x7fffffffll ||
      n_prefixes <= 0 || n_prefixes > 0x7ffffffell || prefix_cap <= 0 || prefix_cap > MAX_PREFIX_CAP)
    return glb::api_fail(GLB_EINVAL, "%s: bad sizes", entry);
  if (splits < 1 || splits > MAX_SPLITS) return glb::api_fail(GLB_EINVAL, "%s: %d splits (1 .. %d)", entry, (int)splits, MAX_SPLITS);
  if (const int rc = check_head_dim_and_alignment(entry, kTileHeadDims, dtype, head_dim,
                                                  {q, k_new, v_new, k_slab, v_slab, out, prefix_k, prefix_v, workspace},
                                                  {q_stride_row, q_stride_head, k_stride_row, k_stride_head, v_stride_row, v_stride_head}))
    return rc;
  const size_t need = glb_slab_attention_prefix_workspace(n_rows, heads, head_dim, splits);
  if (workspace_bytes < need)
    return glb::api_fail(GLB_EINVAL, "%s: workspace of %zu bytes, %zu needed", entry, workspace_bytes, need);
  // launch A: one workgroup per (block of QROWS query rows, KV head, split); a query row past the batch's end stays an int
  const int64_t q_rows = n_rows * (heads / kv_heads), q_blocks = (q_rows + QROWS - 1) / QROWS;
  if (q_rows > 0x7fffffffll - QROWS || q_blocks * kv_heads * splits > 0x7fffffffll) return glb::api_fail(GLB_EINVAL, "%s: bad sizes", entry);
  PrefixArgs a{};
  a.q = (const char *)q;
  a.k_new = (const char *)k_new;
  a.v_new = (const char *)v_new;
  a.k_slab = (char *)k_slab;
  a.v_slab = (char *)v_slab;
  a.out = (char *)out;
  a.pos = pos;
  a.pk = (const char *)prefix_k;
  a.pv = (const char *)prefix_v;
  a.prefix_len = prefix_len;
  a.prefix_of = prefix_of;
  a.ws = (float *)workspace;
  a.q_sr = q_stride_row, a.q_sh = q_stride_head;
  a.k_sr = k_stride_row, a.k_sh = k_stride_head;
  a.v_sr = v_stride_row, a.v_sh = v_stride_head;
  a.R = (int32_t)n_rows;
  a.H = (int32_t)heads;
  a.Hkv = (int32_t)kv_heads;
  a.cap = (int32_t)cap;
  a.U = (int32_t)n_prefixes;
  a.pcap = (int32_t)prefix_cap;
  a.S = splits;
  a.scale = scale;
  const hipStream_t s = (hipStream_t)stream;
  const dim3 grid_a((unsigned)(q_blocks * kv_heads * splits)), grid_b((unsigned)(n_rows * heads));
  hipError_t e = launch_attention_form(kTileHeadDims, dtype, head_dim, [&](auto dt, auto dh) {
    hipLaunchKernelGGL((prefix_partials_kernel<decltype(dt)::value, decltype(dh)::value>), grid_a, dim3(THREADS), 0, s, a);
  });
  if (e != hipSuccess) return glb::api_hip_fail(e, "slab_attention_prefix partials launch");
  e = launch_attention_form(kTileHeadDims, dtype, head_dim, [&](auto dt, auto dh) {
    hipLaunchKernelGGL((prefix_tail_kernel<decltype(dt)::value, decltype(dh)::value>), grid_b, dim3(64), 0, s, a);
  });
  if (e != hipSuccess) return glb::api_hip_fail(e, "slab_attention_prefix tail launch");
  return GLB_OK;
}
