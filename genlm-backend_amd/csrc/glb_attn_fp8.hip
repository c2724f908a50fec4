// glb_attn_fp8.hip - KV rows in OCP e4m3 (include/glb.h): glb_slab_attention_fp8, the one-token decode over
// slab rows kept as one-byte codes plus one float32 scale per (row, KV head, position), and glb_kv_quantize_rows, the fan-out
// of freshly encoded contexts into such rows.
//
// The quantisation rule (both kernels, bit for bit what torch does on the CPU): for the head_dim elements x of one (row, KV
// head, position) as float32, amax = max |x|, s = amax / 448 (IEEE division; s = 1 when amax == 0), code = e4m3_rne(x / s)
// (IEEE division, v_cvt_pk_fp8_f32), value = float(code) * s.  |x / s| never passes 448, so saturation plays no part.
//
// Layout of a wave (both kernels): a 16-byte vector is 16 codes, LP = head_dim / 16 lanes cover a position (lane i of a slot:
// dims 16 i .. 16 i + 15), PP = 64 / LP positions arrive per load instruction; the LP lanes of slot j read position p0 + j's
// two scales from one address.
//
// glb_slab_attention_fp8: one wave per (row, KV head, group of GW query heads), GW = min(G, 4): a K / V vector is loaded and
// converted ONCE (v_cvt_pk_f32_fp8, eight per vector) and used by GW heads, the next step's vectors and scales travel while
// this step's are worked on.  Scales never touch elements: the score is (q . codes) * (k_scale[p] * scale) and V accumulates
// codes * (w * v_scale[p]) - one multiply per position and head.  The arithmetic is on float2 (v_pk_mul_f32 / v_pk_fma_f32).
// Every slot keeps an online softmax per head; the PP slots merge once at the end.  The new token: every wave computes its
// amax (a slot reduction), codes and scales in registers and attends it AT ITS DEQUANTISED VALUE - it is slot 0's first
// position, folded by the code that folds a slab position, so the output is attention over the slab as it stands after the
// call; the wave of the group's first head group writes codes and scales to position pos[r].  No MFMA: one query per head,
// far fewer multiply-adds than bytes, and quantising Q for the fp8 MFMA would change the accuracy contract.
// No atomics, no allocation, no workspace; no address depends on K / V data.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/glb.h"
#include "glb_attn.hpp"
#include "glb_attn_host.hpp"
#include "glb_common.hpp"

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr float E4M3_MAX = 448.0f;

template <int DH>
struct Fp8Shape {
  static constexpr int LP = DH / 16, PP = 64 / LP;
  static_assert(LP == 4 || LP == 8, "head_dim 64 or 128");
};

// 16 elements of the model's type (16 * ES consecutive bytes, 16-byte aligned) as float32
template <int DT>
__device__ __forceinline__ void load16(const char *p, f32x2 *x) {
  constexpr int ES = DT == GLB_F32 ? 4 : 2, EPV = 16 / ES;
  float f[16];
#pragma unroll
  for (int c = 0; c < 16 / EPV; ++c) unpack16<DT>(*reinterpret_cast<const u32x4 *>(p + c * 16), f + c * EPV);
#pragma unroll
  for (int k = 0; k < 8; ++k) x[k] = f32x2{f[2 * k], f[2 * k + 1]};
}

// 16 codes as float32: the codes' own values, no scale
__device__ __forceinline__ void decode16(const u32x4 &w, f32x2 *x) {
  const uint32_t v[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    x[2 * k] = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[k], false);
    x[2 * k + 1] = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[k], true);
  }
}

// the largest value of the slot's LP lanes, in every one of them
template <int LP>
__device__ __forceinline__ float slot_max(float v) {
#pragma unroll
  for (int o = 1; o < LP; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// The rule: this lane's 16 elements of a position -> its 16 codes and the position's scale (the same in the slot's LP lanes)
template <int LP>
__device__ __forceinline__ u32x4 quantize16(const f32x2 *x, float &s) {
  float amax = 0.0f;
#pragma unroll
  for (int k = 0; k < 8; ++k) amax = fmaxf(amax, fmaxf(fabsf(x[k].x), fabsf(x[k].y)));
  amax = slot_max<LP>(amax);
  s = amax == 0.0f ? 1.0f : amax / E4M3_MAX;
  uint32_t w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int c = __builtin_amdgcn_cvt_pk_fp8_f32(x[2 * k].x / s, x[2 * k].y / s, 0, false);
    c = __builtin_amdgcn_cvt_pk_fp8_f32(x[2 * k + 1].x / s, x[2 * k + 1].y / s, c, true);
    w[k] = (uint32_t)c;
  }
  return u32x4{w[0], w[1], w[2], w[3]};
}

// ---- glb_slab_attention_fp8 ---------------------------------------------------------------------------------------------------
struct Fp8AttnArgs {
  const char *q, *k_new, *v_new;
  char *k_codes, *v_codes, *out;
  float *k_scale, *v_scale;
  const int32_t *pos;
  int64_t q_sr, q_sh, k_sr, k_sh, v_sr, v_sh;  // element strides (row, head) of the query, the new K, the new V
  int32_t R, H, Hkv, cap;
  float scale;
};

// One position folded into the slot's online softmax of GW heads: kc / vc its codes, ks = k_scale * scale, vs = v_scale
template <int GW, int LP>
__device__ __forceinline__ void fold(const f32x2 (*qf)[8], const u32x4 &kc, const u32x4 &vc, float ks, float vs, bool seen, float *m,
                                     float *l, f32x2 (*acc)[8]) {
  f32x2 kf[8], vf[8];
  decode16(kc, kf);
  decode16(vc, vf);
#pragma unroll
  for (int g = 0; g < GW; ++g) {
    f32x2 d = qf[g][0] * kf[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) d = __builtin_elementwise_fma(qf[g][k], kf[k], d);
    const float s = slot_sum<LP>(d.x + d.y) * ks;
    if (seen) {  // (the same in the slot's lanes)
      const float m2 = fmaxf(m[g], s), c = __expf(m[g] - m2), w = __expf(s - m2), wv = w * vs;
      l[g] = l[g] * c + w;
      const f32x2 c2{c, c}, w2{wv, wv};
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[g][k] = __builtin_elementwise_fma(vf[k], w2, acc[g][k] * c2);
      m[g] = m2;
    }
  }
}

template <int DT, int DH, int GW>
__global__ __launch_bounds__(64) void slab_attention_fp8_kernel(const Fp8AttnArgs a) {
  constexpr int ES = DT == GLB_F32 ? 4 : 2, EPV = 16 / ES, LP = Fp8Shape<DH>::LP, PP = Fp8Shape<DH>::PP;
  const int lane = threadIdx.x, j = lane / LP, i = lane - j * LP;
  const int G = a.H / a.Hkv, NG = G / GW;  // head groups of a KV head: adjacent blocks, so the codes they share meet in L2
  const int gg = blockIdx.x % NG, hk = (blockIdx.x / NG) % a.Hkv, r = blockIdx.x / (NG * a.Hkv);
  const int h0 = hk * G + gg * GW;
  int p_new = a.pos[r];  // the token being appended sits at p_new; positions 0 .. p_new are attended to
  const bool bad_pos = p_new < 0 || p_new >= a.cap;  // the caller's bug - no fault, no plausible answer: NaN out, nothing appended
  p_new = p_new < 0 ? 0 : (p_new < a.cap ? p_new : a.cap - 1);
  const int64_t slab_row = ((int64_t)r * a.Hkv + hk) * a.cap;
  const char *kb = a.k_codes + slab_row * DH + i * 16, *vb = a.v_codes + slab_row * DH + i * 16;
  const float *ksb = a.k_scale + slab_row, *vsb = a.v_scale + slab_row;

  f32x2 qf[GW][8];
#pragma unroll
  for (int g = 0; g < GW; ++g) load16<DT>(a.q + ((int64_t)r * a.q_sr + (int64_t)(h0 + g) * a.q_sh + i * 16) * ES, qf[g]);
  float m[GW], l[GW];
  f32x2 acc[GW][8];
#pragma unroll
  for (int g = 0; g < GW; ++g) {
    m[g] = -__builtin_huge_valf(), l[g] = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[g][k] = f32x2{0.f, 0.f};
  }
  {  // the new token: quantised here, appended once per (row, KV head), slot 0's first position
    f32x2 x[8];
    float sk, sv;
    load16<DT>(a.k_new + ((int64_t)r * a.k_sr + (int64_t)hk * a.k_sh + i * 16) * ES, x);
    const u32x4 kc = quantize16<LP>(x, sk);
    load16<DT>(a.v_new + ((int64_t)r * a.v_sr + (int64_t)hk * a.v_sh + i * 16) * ES, x);
    const u32x4 vc = quantize16<LP>(x, sv);
    if (gg == 0 && j == 0 && !bad_pos) {
      *reinterpret_cast<u32x4 *>(a.k_codes + (slab_row + p_new) * DH + i * 16) = kc;
      *reinterpret_cast<u32x4 *>(a.v_codes + (slab_row + p_new) * DH + i * 16) = vc;
      if (i == 0) a.k_scale[slab_row + p_new] = sk, a.v_scale[slab_row + p_new] = sv;
    }
    fold<GW, LP>(qf, kc, vc, sk * a.scale, sv, j == 0, m, l, acc);
  }
  // ---- the held positions 0 .. p_new - 1, PP a step; a slot past the end reads position p_new - 1 again and folds nothing
  if (p_new > 0) {
    const int last = p_new - 1;
    int pc = j < last ? j : last;
    u32x4 kc = *reinterpret_cast<const u32x4 *>(kb + (int64_t)pc * DH), vc = *reinterpret_cast<const u32x4 *>(vb + (int64_t)pc * DH);
    float ks = ksb[pc], vs = vsb[pc];
    for (int p0 = 0; p0 < p_new; p0 += PP) {
      const u32x4 kc0 = kc, vc0 = vc;
      const float ks0 = ks, vs0 = vs;
      if (p0 + PP < p_new) {  // (wave-uniform) the next step's vectors travel under this step's arithmetic
        pc = p0 + PP + j;
        pc = pc < last ? pc : last;
        kc = *reinterpret_cast<const u32x4 *>(kb + (int64_t)pc * DH);
        vc = *reinterpret_cast<const u32x4 *>(vb + (int64_t)pc * DH);
        ks = ksb[pc], vs = vsb[pc];
      }
      fold<GW, LP>(qf, kc0, vc0, ks0 * a.scale, vs0, p0 + j < p_new, m, l, acc);
    }
  }
  // ---- merge the PP position slots (lanes i, i + LP, i + 2 LP, ...)
#pragma unroll
  for (int g = 0; g < GW; ++g) {
#pragma unroll
    for (int o = LP; o < 64; o <<= 1) {
      const float mo = __shfl_xor(m[g], o, 64), lo = __shfl_xor(l[g], o, 64);
      const float m2 = fmaxf(m[g], mo);
      const float c = m[g] == m2 ? 1.0f : __expf(m[g] - m2), co = mo == m2 ? 1.0f : __expf(mo - m2);  // (-inf - -inf: an empty slot)
      l[g] = l[g] * c + lo * co;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        acc[g][k].x = acc[g][k].x * c + __shfl_xor(acc[g][k].x, o, 64) * co;
        acc[g][k].y = acc[g][k].y * c + __shfl_xor(acc[g][k].y, o, 64) * co;
      }
      m[g] = m2;
    }
    if (j == 0) {
      const float inv = bad_pos ? __builtin_nanf("") : 1.0f / l[g];
      float o16[16];
#pragma unroll
      for (int k = 0; k < 8; ++k) o16[2 * k] = acc[g][k].x * inv, o16[2 * k + 1] = acc[g][k].y * inv;
      char *op = a.out + (((int64_t)r * a.H + h0 + g) * DH + i * 16) * ES;
#pragma unroll
      for (int c = 0; c < 16 / EPV; ++c) *reinterpret_cast<u32x4 *>(op + c * 16) = pack16v<DT>(o16 + c * EPV);
    }
  }
}

// ---- glb_kv_quantize_rows -------------------------------------------------------------------------------------------------------
// One wave per (tensor, destination row, KV head, step of PP positions): loads in the source type, stores 16-byte code vectors
// and the positions' scales.  Row, head and step are the wave's, so the early returns are wave-uniform.
template <int DT, int DH>
__global__ __launch_bounds__(64) void kv_quantize_rows_kernel(const char *const *src, char *const *dst_codes, float *const *dst_scale,
                                                              int32_t n_src, int32_t heads, int32_t steps, int32_t src_cap,
                                                              int32_t dst_cap, const int32_t *src_row_of, const int32_t *len_of) {
  constexpr int ES = DT == GLB_F32 ? 4 : 2, LP = Fp8Shape<DH>::LP, PP = Fp8Shape<DH>::PP;
  const int lane = threadIdx.x, j = lane / LP, i = lane - j * LP, t = blockIdx.y;
  const int step = blockIdx.x % steps, h = (blockIdx.x / steps) % heads, row = blockIdx.x / (steps * heads);
  const int sr = src_row_of[row];
  int len = len_of[row];
  len = len < src_cap ? len : src_cap;
  len = len < dst_cap ? len : dst_cap;
  if (sr < 0 || sr >= n_src || step * PP >= len) return;
  const int p = step * PP + j, pc = p < len ? p : len - 1;  // a slot past the end reads the last position and stores nothing
  f32x2 x[8];
  float s;
  load16<DT>(src[t] + ((((int64_t)sr * heads + h) * src_cap + pc) * DH + i * 16) * ES, x);
  const u32x4 c = quantize16<LP>(x, s);
  if (p < len) {
    const int64_t at = ((int64_t)row * heads + h) * dst_cap + p;
    *reinterpret_cast<u32x4 *>(dst_codes[t] + at * DH + i * 16) = c;
    if (i == 0) dst_scale[t][at] = s;
  }
}

}  // namespace

extern "C" int glb_slab_attention_fp8(const void *q, int64_t q_stride_row, int64_t q_stride_head, const void *k_new,
                                      int64_t k_stride_row, int64_t k_stride_head, const void *v_new, int64_t v_stride_row,
                                      int64_t v_stride_head, void *k_codes, void *v_codes, float *k_scale, float *v_scale,
                                      const int32_t *pos, int64_t n_rows, int64_t heads, int64_t kv_heads, int64_t cap,
                                      int64_t head_dim, float scale, int32_t dtype, void *out, void *stream) {
  const char *entry = "glb_slab_attention_fp8";
  if (!q || !k_new || !v_new || !k_codes || !v_codes || !k_scale || !v_scale || !pos || !out)
    return glb::api_fail(GLB_EINVAL, "%s: null pointer", entry);
  if (const int rc = check_dtype(dtype)) return rc;
  if (n_rows <= 0 || heads <= 0 || kv_heads <= 0 || cap <= 0 || heads % kv_heads || n_rows * heads > 0x7fffffffll || cap > 0x7fffffffll)
    return glb::api_fail(GLB_EINVAL, "%s: bad sizes", entry);
  const bool aligned = (uintptr_t)k_scale % 4 == 0 && (uintptr_t)v_scale % 4 == 0;
  if (const int rc = check_head_dim_and_alignment(entry, kTileHeadDims, dtype, head_dim, {q, k_new, v_new, k_codes, v_codes, out},
                                                  {q_stride_row, q_stride_head, k_stride_row, k_stride_head, v_stride_row, v_stride_head},
                                                  aligned))
    return rc;
  const int64_t G = heads / kv_heads;
  if (G != 1 && G != 2 && G != 4 && G != 8)
    return glb::api_fail(GLB_EUNSUPPORTED, "%s: %lld query heads per KV head (1, 2, 4 and 8 are built)", entry, (long long)G);
  Fp8AttnArgs a{};
  a.q = (const char *)q;
  a.k_new = (const char *)k_new;
  a.v_new = (const char *)v_new;
  a.k_codes = (char *)k_codes;
  a.v_codes = (char *)v_codes;
  a.out = (char *)out;
  a.k_scale = k_scale;
  a.v_scale = v_scale;
  a.pos = pos;
  a.q_sr = q_stride_row, a.q_sh = q_stride_head;
  a.k_sr = k_stride_row, a.k_sh = k_stride_head;
  a.v_sr = v_stride_row, a.v_sh = v_stride_head;
  a.R = (int32_t)n_rows;
  a.H = (int32_t)heads;
  a.Hkv = (int32_t)kv_heads;
  a.cap = (int32_t)cap;
  a.scale = scale;
  const int gw = G < 4 ? (int)G : 4;  // query heads a wave serves
  const dim3 grid((unsigned)(n_rows * kv_heads * (G / gw))), block(64);
  const hipStream_t s = (hipStream_t)stream;
  const hipError_t e = launch_attention_form(kTileHeadDims, dtype, head_dim, [&](auto dt, auto dh) {
    constexpr int DT = decltype(dt)::value, DH = decltype(dh)::value;
    if (gw == 1) hipLaunchKernelGGL((slab_attention_fp8_kernel<DT, DH, 1>), grid, block, 0, s, a);
    else if (gw == 2) hipLaunchKernelGGL((slab_attention_fp8_kernel<DT, DH, 2>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((slab_attention_fp8_kernel<DT, DH, 4>), grid, block, 0, s, a);
  });
  if (e != hipSuccess) return glb::api_hip_fail(e, "slab_attention_fp8 launch");
  return GLB_OK;
}

extern "C" int glb_kv_quantize_rows(const void *const *src, void *const *dst_codes, float *const *dst_scale, int64_t n_tensors,
                                    int64_t n_src_rows, int64_t n_rows, int64_t kv_heads, int64_t head_dim, int64_t src_cap,
                                    int64_t dst_cap, const int32_t *src_row_of, const int32_t *len_of, int32_t dtype, void *stream) {
  const char *entry = "glb_kv_quantize_rows";
  if (!src || !dst_codes || !dst_scale || !src_row_of || !len_of) return glb::api_fail(GLB_EINVAL, "%s: null pointer", entry);
  if (const int rc = check_dtype(dtype)) return rc;
  if (n_tensors <= 0 || n_tensors > 65535 || n_src_rows <= 0 || n_src_rows > 0x7fffffffll || n_rows <= 0 || kv_heads <= 0 ||
      src_cap <= 0 || dst_cap <= 0 || src_cap > 0x7fffffffll || dst_cap > 0x7fffffffll)
    return glb::api_fail(GLB_EINVAL, "%s: bad sizes", entry);
  if (const int rc = check_head_dim_and_alignment(entry, kTileHeadDims, dtype, head_dim, {}, {})) return rc;
  const int64_t pp = 64 / (head_dim / 16), span = src_cap < dst_cap ? src_cap : dst_cap, steps = (span + pp - 1) / pp;
  if (n_rows * kv_heads * steps > 0x7fffffffll) return glb::api_fail(GLB_EINVAL, "%s: bad sizes", entry);
  const dim3 grid((unsigned)(n_rows * kv_heads * steps), (unsigned)n_tensors), block(64);
  const hipError_t e = launch_attention_form(kTileHeadDims, dtype, head_dim, [&](auto dt, auto dh) {
    hipLaunchKernelGGL((kv_quantize_rows_kernel<decltype(dt)::value, decltype(dh)::value>), grid, block, 0, (hipStream_t)stream,
                       (const char *const *)src, (char *const *)dst_codes, dst_scale, (int32_t)n_src_rows, (int32_t)kv_heads,
                       (int32_t)steps, (int32_t)src_cap, (int32_t)dst_cap, src_row_of, len_of);
  });
  if (e != hipSuccess) return glb::api_hip_fail(e, "kv_quantize_rows launch");
  return GLB_OK;
}
