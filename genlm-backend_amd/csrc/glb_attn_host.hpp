// glb_attn_host.hpp - the host side the attention entries of glb_kv.hip and glb_attn_tile.hip share: the
// dispatch over the built forms, the checks around an entry's own size checks, and glb_slab_attention_chunk's contract
// (fill_chunk_args) for the entries under it.  The device side is glb_attn.hpp.
#pragma once
#include <initializer_list>
#include <type_traits>

#include "glb_common.hpp"

namespace {

// The head sizes an entry's kernels are built for, and how GLB_EUNSUPPORTED names them.  (The compiler emits the kernels of a
// launch in the reverse of this order; it is the order the code objects had when the dispatch was an if-chain.)
template <int... DH>
struct HeadDims {
  const char *built;
};
constexpr HeadDims<16, 32, 128, 64> kWaveHeadDims{"16, 32, 64 and 128"};  // the wave kernels of glb_kv.hip
constexpr HeadDims<128, 64> kTileHeadDims{"64 and 128"};                  // the MFMA tile kernel

// ---- the dispatch over the built forms: f gets the element type / the head size as an std::integral_constant ------------
template <class F>
hipError_t with_dtype(int32_t dtype, F f) {
  switch (dtype) {
    case GLB_F32: return f(std::integral_constant<int, GLB_F32>{});
    case GLB_BF16: return f(std::integral_constant<int, GLB_BF16>{});
    default: return f(std::integral_constant<int, GLB_F16>{});
  }
}

template <int... DH, class F>
hipError_t with_head_dim(HeadDims<DH...>, int64_t head_dim, F f) {
  hipError_t e = hipErrorInvalidValue;
  (void)((head_dim == DH && ((e = f(std::integral_constant<int, DH>{})), true)) || ...);
  return e;
}

// launch(dt, dh) enqueues the kernel of that form; the launch's error
template <int... DH, class F>
hipError_t launch_attention_form(HeadDims<DH...> dims, int32_t dtype, int64_t head_dim, F launch) {
  return with_dtype(dtype, [&](auto dt) {
    return with_head_dim(dims, head_dim, [&](auto dh) {
      launch(dt, dh);
      return hipGetLastError();
    });
  });
}

// What the attention entries check, around their own size checks: the element type before them ...
inline int check_dtype(int32_t dtype) {
  if (dtype < GLB_F32 || dtype > GLB_F16) return glb::api_fail(GLB_EINVAL, "bad dtype %d", dtype);
  return GLB_OK;
}

// ... and behind them the head size, then 16-byte alignment of every pointer and every byte stride (`aligned`: what else the
// entry reports under that message)
template <int... DH>
int check_head_dim_and_alignment(const char *entry, HeadDims<DH...> dims, int32_t dtype, int64_t head_dim,
                                 std::initializer_list<const void *> ptrs, std::initializer_list<int64_t> strides, bool aligned = true) {
  if (!((head_dim == DH) || ...))
    return glb::api_fail(GLB_EUNSUPPORTED, "%s: head_dim %lld (%s are built)", entry, (long long)head_dim, dims.built);
  const int es = dtype == GLB_F32 ? 4 : 2;
  for (const void *p : ptrs) aligned = aligned && (uintptr_t)p % 16 == 0;
  for (const int64_t st : strides) aligned = aligned && (st * es) % 16 == 0;
  if (!aligned) return glb::api_fail(GLB_EINVAL, "%s: pointers and strides must be 16-byte aligned", entry);
  return GLB_OK;
}

// glb_slab_attention_chunk's contract (include/glb.h), for every entry under it: the checks that do not depend on how the
// kernel splits the work - the entry bounds its own grid afterwards - and the argument block `a` (ChunkAttnArgs, TileArgs: the
// same fields up to n_slab_rows).  limit: the most new tokens per row the entry takes.
template <class Args, int... DH>
int fill_chunk_args(const char *entry, int64_t limit, HeadDims<DH...> dims, const void *q, const int64_t q_strides[3],
                    const void *k_new, const int64_t k_strides[3], const void *v_new, const int64_t v_strides[3], void *k_slab,
                    void *v_slab, const int32_t *pos, const int32_t *n_new, const int32_t *row_of, int64_t n_rows,
                    int64_t n_slab_rows, int64_t heads, int64_t kv_heads, int64_t cap, int64_t head_dim, int64_t max_new,
                    float scale, int32_t dtype, void *out, Args &a) {
  if (!q || !k_new || !v_new || !k_slab || !v_slab || !pos || !n_new || !out || !q_strides || !k_strides || !v_strides)
    return glb::api_fail(GLB_EINVAL, "%s: null pointer", entry);
  if (const int rc = check_dtype(dtype)) return rc;
  if (max_new < 1 || max_new > limit)
    return glb::api_fail(GLB_EINVAL, "%s: %lld query positions per row (1 .. %d)", entry, (long long)max_new, (int)limit);
  if (n_rows <= 0 || n_slab_rows <= 0 || heads <= 0 || kv_heads <= 0 || cap <= 0 || heads % kv_heads || cap > 0x7fffffffll ||
      n_slab_rows > 0x7fffffffll)
    return glb::api_fail(GLB_EINVAL, "%s: bad sizes", entry);
  if (const int rc = check_head_dim_and_alignment(
          entry, dims, dtype, head_dim, {q, k_new, v_new, k_slab, v_slab, out},
          {q_strides[0], q_strides[1], q_strides[2], k_strides[0], k_strides[1], k_strides[2], v_strides[0], v_strides[1], v_strides[2]}))
    return rc;
  a.q = (const char *)q;
  a.k_new = (const char *)k_new;
  a.v_new = (const char *)v_new;
  a.k_slab = (char *)k_slab;
  a.v_slab = (char *)v_slab;
  a.out = (char *)out;
  a.pos = pos;
  a.n_new = n_new;
  a.row_of = row_of;
  a.q_sr = q_strides[0], a.q_sh = q_strides[1], a.q_sp = q_strides[2];
  a.k_sr = k_strides[0], a.k_sh = k_strides[1], a.k_sp = k_strides[2];
  a.v_sr = v_strides[0], a.v_sh = v_strides[1], a.v_sp = v_strides[2];
  a.n = (int32_t)n_rows;
  a.H = (int32_t)heads;
  a.Hkv = (int32_t)kv_heads;
  a.cap = (int32_t)cap;
  a.T = (int32_t)max_new;
  a.n_slab_rows = (int32_t)n_slab_rows;
  a.scale = scale;
  return GLB_OK;
}

}  // namespace
