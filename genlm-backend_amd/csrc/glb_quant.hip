// glb_quant.hip - 4-bit block-quantised weights (include/glb.h: glb_w4_bytes, glb_w4_quantize, glb_w4_dequantize,
// glb_w4_gemm_workspace_bytes, glb_w4_gemm_max_rows, glb_w4_gemm).
//
// Format: a weight W[N, K] is cut into blocks of 64 consecutive elements along K; a block stores absmax = max |w| (float32)
// and 64 four-bit codes into a 16-entry float32 codebook that the caller passes as data (NF4 and FP4 are two tables).
//   quantise:   sort the codebook, m_i = (c_i + c_{i+1}) * 0.5f; the code of w is the sorted entry whose index is the number
//               of float32 products m_i * absmax strictly below w (no division)
//   dequantise: w' = codebook[code] * absmax, ONE float32 multiplication, then one round-to-nearest-even to the output dtype
// Both are restated bit for bit in tests/quant4_engine.py.
//
// Image (N K / 2 bytes of codes, then N K / 64 floats of absmax).  Rows are taken 16 at a time (the last group has the
// rows that are left: rb = min(16, N - 16 nb)); row group nb starts at byte nb * 16 * K / 2 and holds, for K block kb and
// row r of the group, the 32-byte unit (kb * rb + r): byte b = code of k = 2 b (low nibble) and of k = 2 b + 1 (high
// nibble).  absmax mirrors it: float nb * 16 * K / 64 + kb * rb + r.  In the GEMM lane l (column r = l & 15, g = l >> 4) of a
// wave reads the 8 bytes g of unit (kb, r) - a wave's load is 512 contiguous bytes - and owns k = 16 g .. 16 g + 15 of the
// block: the first four bytes are its B operand of the block's first v_mfma_f32_16x16x32, the last four of the second (the
// MFMA sums over k in any assignment of k to (lane group, element) that A and B share; A is read to match).
//
// GEMM (few rows: M <= glb_w4_gemm_max_rows()): a wave owns 16 output columns and a slice of K for all rows (up to 8
// row fragments of 16), expands codes in registers and writes float32 partial sums; a second launch adds the slices in
// ascending order, adds the bias and rounds once.  The K split depends on (N, K) only and there are no atomics: the
// bits are the same run to run.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/glb.h"
#include "glb_common.hpp"

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

constexpr int QB = 64;             // elements of a block
constexpr int UNIT = QB / 2;       // bytes of a block's codes
constexpr int GEMM_MAX_MF = 8;     // row fragments of 16 a wave can hold
// Rows glb_w4_gemm serves: the largest M at which it was measured faster than dequantise + library GEMM on any shape of
// profiles/r09/w4_gemm_ab.txt, rounded up to the 16-row fragment.
constexpr int GEMM_MAX_ROWS = 128;
constexpr int GEMM_TARGET_WAVES = 4096;  // 4 per SIMD on 256 CUs
constexpr int64_t MAX_ELEMS = (int64_t)1 << 34;

struct Codebook {
  float v[16];
};
struct QuantTable {
  float mid[15];     // midpoints of the sorted codebook
  uint64_t code_of;  // nibble i: the code of the i-th smallest entry
};

__device__ __forceinline__ float load_elem(const void *p, int64_t idx, int dt) {
  if (dt == GLB_F32) return ((const float *)p)[idx];
  const uint16_t h = ((const uint16_t *)p)[idx];
  if (dt == GLB_BF16) return __uint_as_float((uint32_t)h << 16);
  return __half2float(__ushort_as_half(h));
}

__device__ __forceinline__ uint16_t bf16_rne(float f) {
  uint32_t u = __float_as_uint(f);
  u += 0x7fffu + ((u >> 16) & 1u);  // (finite input: absmax is finite and every codebook entry is)
  return (uint16_t)(u >> 16);
}

__device__ __forceinline__ void store_elem(void *p, int64_t idx, int dt, float f) {
  // (the barrier keeps the f32 product: multiply + convert must not become one v_fma_mix*_f16, a single rounding)
  asm volatile("" : "+v"(f));
  if (dt == GLB_F32) ((float *)p)[idx] = f;
  else if (dt == GLB_BF16) ((uint16_t *)p)[idx] = bf16_rne(f);
  else ((uint16_t *)p)[idx] = __half_as_ushort(__float2half_rn(f));
}

__device__ __forceinline__ uint32_t quant_code(float w, float absmax, const QuantTable &q) {
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < 15; ++i) cnt += (q.mid[i] * absmax < w) ? 1 : 0;
  return (uint32_t)(q.code_of >> (4 * cnt)) & 15u;
}

// byte offset of unit (row n, K block kb) in the codes, and its index in the absmax array
__device__ __forceinline__ int64_t unit_index(int64_t n, int64_t kb, int64_t n_rows, int64_t kb_count) {
  const int64_t nb = n >> 4, r = n & 15, rb = min((int64_t)16, n_rows - 16 * nb);
  return nb * 16 * kb_count + kb * rb + r;
}

// W [N, K] (K contiguous): 16 lanes per block, 4 consecutive elements each
__global__ __launch_bounds__(256) void quantize_rows_kernel(const void *__restrict__ w, int64_t ldw, int dt, int64_t n_rows,
                                                            int64_t kb_count, QuantTable q, char *__restrict__ image) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t blk = t >> 4;
  if (blk >= n_rows * kb_count) return;  // (whole 16-lane groups leave together)
  const int sub = (int)(t & 15);
  const int64_t n = blk / kb_count, kb = blk % kb_count;
  const int64_t src = n * ldw + kb * QB + 4 * sub;
  float v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = load_elem(w, src + j, dt);
  float amax = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])));
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) amax = fmaxf(amax, __shfl_xor(amax, d, 16));
  uint32_t packed = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) packed |= quant_code(v[j], amax, q) << (4 * j);
  const int64_t u = unit_index(n, kb, n_rows, kb_count);
  *(uint16_t *)(image + u * UNIT + 2 * sub) = (uint16_t)packed;
  if (sub == 0) ((float *)(image + n_rows * kb_count * UNIT))[u] = amax;
}

// W^T [K, N] (N contiguous: GPT-2's Conv1D): one thread per block, adjacent threads adjacent n
__global__ __launch_bounds__(256) void quantize_cols_kernel(const void *__restrict__ w, int64_t ldw, int dt, int64_t n_rows,
                                                            int64_t kb_count, QuantTable q, char *__restrict__ image) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_rows * kb_count) return;
  const int64_t kb = t / n_rows, n = t % n_rows;
  float v[QB];
  float amax = 0.0f;
#pragma unroll
  for (int j = 0; j < QB; ++j) {
    v[j] = load_elem(w, (kb * QB + j) * ldw + n, dt);
    amax = fmaxf(amax, fabsf(v[j]));
  }
  uint32_t words[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    uint32_t p = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) p |= quant_code(v[8 * i + j], amax, q) << (4 * j);
    words[i] = p;
  }
  const int64_t u = unit_index(n, kb, n_rows, kb_count);
  u32x4 *dst = (u32x4 *)(image + u * UNIT);
  dst[0] = u32x4{words[0], words[1], words[2], words[3]};
  dst[1] = u32x4{words[4], words[5], words[6], words[7]};
  ((float *)(image + n_rows * kb_count * UNIT))[u] = amax;
}

__global__ __launch_bounds__(256) void dequantize_rows_kernel(const char *__restrict__ image, Codebook cb, int64_t n_rows,
                                                              int64_t kb_count, void *__restrict__ out, int64_t ldo, int dt) {
  __shared__ float lut[16];
  if (threadIdx.x < 16) lut[threadIdx.x] = cb.v[threadIdx.x];
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t blk = t >> 4;
  if (blk >= n_rows * kb_count) return;
  const int sub = (int)(t & 15);
  const int64_t n = blk / kb_count, kb = blk % kb_count;
  const int64_t u = unit_index(n, kb, n_rows, kb_count);
  const uint32_t packed = *(const uint16_t *)(image + u * UNIT + 2 * sub);
  const float amax = ((const float *)(image + n_rows * kb_count * UNIT))[u];
  const int64_t dst = n * ldo + kb * QB + 4 * sub;
#pragma unroll
  for (int j = 0; j < 4; ++j) store_elem(out, dst + j, dt, lut[(packed >> (4 * j)) & 15u] * amax);
}

__global__ __launch_bounds__(256) void dequantize_cols_kernel(const char *__restrict__ image, Codebook cb, int64_t n_rows,
                                                              int64_t kb_count, void *__restrict__ out, int64_t ldo, int dt) {
  __shared__ float lut[16];
  if (threadIdx.x < 16) lut[threadIdx.x] = cb.v[threadIdx.x];
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_rows * kb_count) return;
  const int64_t kb = t / n_rows, n = t % n_rows;
  const int64_t u = unit_index(n, kb, n_rows, kb_count);
  const u32x4 *src = (const u32x4 *)(image + u * UNIT);
  const u32x4 c0 = src[0], c1 = src[1];
  const uint32_t words[8] = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]};
  const float amax = ((const float *)(image + n_rows * kb_count * UNIT))[u];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j)
      store_elem(out, (kb * QB + 8 * i + j) * ldo + n, dt, lut[(words[i] >> (4 * j)) & 15u] * amax);
}

// eight codes of one word -> lane's B operand (8 values of the 16-bit dtype), each codebook[code] * absmax rounded once
template <int DT>
__device__ __forceinline__ u32x4 expand8(uint32_t word, float amax, const float *lut) {
  u32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float a = lut[(word >> (8 * i)) & 15u] * amax, b = lut[(word >> (8 * i + 4)) & 15u] * amax;
    if constexpr (DT == GLB_BF16) {
      o[i] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{a, b}, bf16x2));  // v_cvt_pk_bf16_f32 (RNE)
    } else {
      asm volatile("" : "+v"(a), "+v"(b));  // (as store_elem: no fused multiply-convert)
      o[i] = (uint32_t)__half_as_ushort(__float2half_rn(a)) | ((uint32_t)__half_as_ushort(__float2half_rn(b)) << 16);
    }
  }
  return o;
}

template <int DT>
__device__ __forceinline__ f32x4 mfma16(u32x4 a, u32x4 b, f32x4 c) {
  if constexpr (DT == GLB_BF16)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// One wave per (16 columns, K slice): part[ks][row][col] = sum over the slice of X[row, k] * W'[col, k].
template <int DT, int MF>
__global__ __launch_bounds__(256) void w4_gemm_kernel(const uint16_t *__restrict__ x, int64_t ldx, const char *__restrict__ image,
                                                      Codebook cb, float *__restrict__ part, int m, int n, int k, int ksplit) {
  __shared__ float lut[16];
  if (threadIdx.x < 16) lut[threadIdx.x] = cb.v[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int kb_count = k / QB, nb_count = n / 16;
  const int64_t unit = (int64_t)blockIdx.x * 4 + wave;
  if (unit >= (int64_t)nb_count * ksplit) return;
  const int nb = (int)(unit / ksplit), ks = (int)(unit % ksplit);
  const int kb0 = (int)((int64_t)ks * kb_count / ksplit), kb1 = (int)((int64_t)(ks + 1) * kb_count / ksplit);
  const int r = lane & 15, g = lane >> 4;
  const char *codes = image + (int64_t)nb * 16 * kb_count * UNIT + r * UNIT + g * 8;        // + kb * 16 * UNIT
  const float *amax = (const float *)(image + (int64_t)n * kb_count * UNIT) + (int64_t)nb * 16 * kb_count + r;  // + kb * 16
  const uint16_t *xp[MF];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
    int row = mf * 16 + r;
    row = row < m ? row : m - 1;  // rows past M read the last row; their results are never stored
    xp[mf] = x + (int64_t)row * ldx + g * 16;
  }
  f32x4 acc[MF];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) acc[mf] = f32x4{0.f, 0.f, 0.f, 0.f};

  // software pipeline: block kb + 1 is loaded before block kb is expanded and multiplied
  u32x2 c = *(const u32x2 *)(codes + (int64_t)kb0 * 16 * UNIT);
  float a = amax[(int64_t)kb0 * 16];
  u32x4 xa[MF][2];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
    xa[mf][0] = *(const u32x4 *)(xp[mf] + kb0 * QB);
    xa[mf][1] = *(const u32x4 *)(xp[mf] + kb0 * QB + 8);
  }
  for (int kb = kb0; kb < kb1; ++kb) {
    const int nx = kb + 1 < kb1 ? kb + 1 : kb;  // (the last block is loaded twice, never past the slice)
    const u32x2 cn = *(const u32x2 *)(codes + (int64_t)nx * 16 * UNIT);
    const float an = amax[(int64_t)nx * 16];
    u32x4 xn[MF][2];
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) {
      xn[mf][0] = *(const u32x4 *)(xp[mf] + nx * QB);
      xn[mf][1] = *(const u32x4 *)(xp[mf] + nx * QB + 8);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const u32x4 b = expand8<DT>(c[s], a, lut);
#pragma unroll
      for (int mf = 0; mf < MF; ++mf) acc[mf] = mfma16<DT>(xa[mf][s], b, acc[mf]);
    }
    c = cn;
    a = an;
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) xa[mf][0] = xn[mf][0], xa[mf][1] = xn[mf][1];
  }
  // C/D map of the 16x16 MFMA: col = lane & 15, row = 4 * (lane >> 4) + reg
  float *dst = part + (int64_t)ks * m * n + nb * 16 + r;
#pragma unroll
  for (int mf = 0; mf < MF; ++mf)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = mf * 16 + 4 * g + j;
      if (row < m) dst[(int64_t)row * n] = acc[mf][j];
    }
}

// y[row, col] = round(sum of the K slices, ascending, + bias)
__global__ __launch_bounds__(256) void w4_reduce_kernel(const float *__restrict__ part, int ksplit, int m, int n,
                                                        const uint16_t *__restrict__ bias, uint16_t *__restrict__ y, int64_t ldy,
                                                        int dt) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)m * n) return;
  const int row = (int)(t / n), col = (int)(t % n);
  float s = part[t];
  for (int ks = 1; ks < ksplit; ++ks) s += part[(int64_t)ks * m * n + t];
  if (bias) s += load_elem(bias, col, dt);
  store_elem(y, (int64_t)row * ldy + col, dt, s);
}

bool dtype_ok(int32_t dt) { return dt == GLB_F32 || dt == GLB_BF16 || dt == GLB_F16; }
size_t elem_bytes(int32_t dt) { return dt == GLB_F32 ? 4 : 2; }
bool shape_served(int64_t n, int64_t k) { return n > 0 && k > 0 && k % QB == 0 && n <= MAX_ELEMS / k; }

bool codebook_ok(const float *cb) {
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(cb[i])) return false;
  return true;
}

QuantTable make_table(const float *cb) {
  int order[16];
  for (int i = 0; i < 16; ++i) order[i] = i;
  std::stable_sort(order, order + 16, [&](int a, int b) { return cb[a] < cb[b]; });
  QuantTable q{};
  for (int i = 0; i < 16; ++i) q.code_of |= (uint64_t)order[i] << (4 * i);
  for (int i = 0; i < 15; ++i) {
    volatile float s = cb[order[i]] + cb[order[i + 1]];  // (one float32 addition, then an exact halving)
    q.mid[i] = s * 0.5f;
  }
  return q;
}

int gemm_ksplit(int64_t n, int64_t k) {
  const int64_t nb = n / 16, kb = k / QB;
  int64_t ks = (GEMM_TARGET_WAVES + nb - 1) / nb;
  ks = std::min(ks, std::max<int64_t>(1, kb / 2));  // at least two blocks of K per wave
  return (int)std::max<int64_t>(1, ks);
}

bool gemm_shape_served(int64_t n, int64_t k) { return shape_served(n, k) && n % 16 == 0 && n <= (1 << 24) && k <= (1 << 24); }

int check_quant_args(const glb_w4_args *args, const char *what) {
  if (!args) return glb::api_fail(GLB_EINVAL, "%s: null argument block", what);
  if (args->struct_size != sizeof(glb_w4_args))
    return glb::api_fail(GLB_EINVAL, "glb_w4_args.struct_size %u != %zu (ABI mismatch)", args->struct_size, sizeof(glb_w4_args));
  const glb_w4_args &a = *args;
  if (!dtype_ok(a.dtype) || (a.transposed != 0 && a.transposed != 1))
    return glb::api_fail(GLB_EINVAL, "%s: bad dtype / layout (%d, %d)", what, a.dtype, a.transposed);
  if (!a.w || !a.image || !a.codebook) return glb::api_fail(GLB_EINVAL, "%s: null pointer", what);
  if (a.n <= 0 || a.k <= 0 || a.ldw < (a.transposed ? a.n : a.k))
    return glb::api_fail(GLB_EINVAL, "%s: bad shape (n %lld, k %lld, ldw %lld)", what, (long long)a.n, (long long)a.k,
                         (long long)a.ldw);
  if (!codebook_ok(a.codebook)) return glb::api_fail(GLB_EINVAL, "%s: codebook entry not finite", what);
  if ((uintptr_t)a.w % elem_bytes(a.dtype)) return glb::api_fail(GLB_EINVAL, "%s: w not aligned to its element", what);
  if (!shape_served(a.n, a.k)) return glb::api_fail(GLB_EUNSUPPORTED, "%s: k %% 64 != 0 or too many elements", what);
  if (a.image_bytes < glb_w4_bytes(a.n, a.k) || (uintptr_t)a.image % 16)
    return glb::api_fail(GLB_ENOSPC, "%s: image buffer too small or not 16-byte aligned", what);
  return GLB_OK;
}

template <int DT, int MF>
void launch_gemm_mf(const glb_w4_gemm_args &g, const Codebook &cb, int ksplit, hipStream_t stream) {
  const int64_t waves = (g.n / 16) * ksplit;
  hipLaunchKernelGGL((w4_gemm_kernel<DT, MF>), dim3(blocks_for(waves, 4)), dim3(256), 0, stream, (const uint16_t *)g.x, g.ldx,
                     (const char *)g.image, cb, (float *)g.workspace, (int)g.m, (int)g.n, (int)g.k, ksplit);
}

template <int DT>
void launch_gemm(const glb_w4_gemm_args &g, const Codebook &cb, int ksplit, hipStream_t stream) {
  switch ((g.m + 15) / 16) {
    case 1: launch_gemm_mf<DT, 1>(g, cb, ksplit, stream); break;
    case 2: launch_gemm_mf<DT, 2>(g, cb, ksplit, stream); break;
    case 3: launch_gemm_mf<DT, 3>(g, cb, ksplit, stream); break;
    case 4: launch_gemm_mf<DT, 4>(g, cb, ksplit, stream); break;
    case 5: launch_gemm_mf<DT, 5>(g, cb, ksplit, stream); break;
    case 6: launch_gemm_mf<DT, 6>(g, cb, ksplit, stream); break;
    case 7: launch_gemm_mf<DT, 7>(g, cb, ksplit, stream); break;
    default: launch_gemm_mf<DT, 8>(g, cb, ksplit, stream); break;
  }
}

}  // namespace

extern "C" {

size_t glb_w4_bytes(int64_t n, int64_t k) {
  return shape_served(n, k) ? (size_t)n * (size_t)k / 2 + sizeof(float) * ((size_t)n * (size_t)k / QB) : 0;
}

int glb_w4_quantize(const glb_w4_args *args, void *stream) {
  const int rc = check_quant_args(args, "glb_w4_quantize");
  if (rc != GLB_OK) return rc;
  const glb_w4_args &a = *args;
  const QuantTable q = make_table(a.codebook);
  const int64_t kb = a.k / QB;
  if (a.transposed)
    hipLaunchKernelGGL(quantize_cols_kernel, dim3(blocks_for(a.n * kb, 256)), dim3(256), 0, (hipStream_t)stream, a.w, a.ldw,
                       a.dtype, a.n, kb, q, (char *)a.image);
  else
    hipLaunchKernelGGL(quantize_rows_kernel, dim3(blocks_for(a.n * kb * 16, 256)), dim3(256), 0, (hipStream_t)stream, a.w,
                       a.ldw, a.dtype, a.n, kb, q, (char *)a.image);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return glb::api_hip_fail(e, "w4 quantize launch");
  return GLB_OK;
}

int glb_w4_dequantize(const glb_w4_args *args, void *stream) {
  const int rc = check_quant_args(args, "glb_w4_dequantize");
  if (rc != GLB_OK) return rc;
  const glb_w4_args &a = *args;
  Codebook cb;
  for (int i = 0; i < 16; ++i) cb.v[i] = a.codebook[i];
  const int64_t kb = a.k / QB;
  if (a.transposed)
    hipLaunchKernelGGL(dequantize_cols_kernel, dim3(blocks_for(a.n * kb, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const char *)a.image, cb, a.n, kb, a.w, a.ldw, a.dtype);
  else
    hipLaunchKernelGGL(dequantize_rows_kernel, dim3(blocks_for(a.n * kb * 16, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const char *)a.image, cb, a.n, kb, a.w, a.ldw, a.dtype);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return glb::api_hip_fail(e, "w4 dequantize launch");
  return GLB_OK;
}

int glb_w4_gemm_max_rows(void) { return GEMM_MAX_ROWS; }

size_t glb_w4_gemm_workspace_bytes(int64_t m, int64_t n, int64_t k) {
  if (m <= 0 || m > GEMM_MAX_ROWS || !gemm_shape_served(n, k)) return 0;
  return (size_t)gemm_ksplit(n, k) * (size_t)m * (size_t)n * sizeof(float);
}

int glb_w4_gemm(const glb_w4_gemm_args *args, void *stream) {
  if (!args) return glb::api_fail(GLB_EINVAL, "null argument block");
  if (args->struct_size != sizeof(glb_w4_gemm_args))
    return glb::api_fail(GLB_EINVAL, "glb_w4_gemm_args.struct_size %u != %zu (ABI mismatch)", args->struct_size,
                         sizeof(glb_w4_gemm_args));
  const glb_w4_gemm_args &g = *args;
  if (g.dtype != GLB_BF16 && g.dtype != GLB_F16) return glb::api_fail(GLB_EINVAL, "glb_w4_gemm: dtype %d is not 16-bit", g.dtype);
  if (!g.x || !g.image || !g.y || !g.codebook || !g.workspace) return glb::api_fail(GLB_EINVAL, "glb_w4_gemm: null pointer");
  if (g.m <= 0 || g.n <= 0 || g.k <= 0 || g.ldx < g.k || g.ldy < g.n)
    return glb::api_fail(GLB_EINVAL, "glb_w4_gemm: bad shape (m %lld, n %lld, k %lld, ldx %lld, ldy %lld)", (long long)g.m,
                         (long long)g.n, (long long)g.k, (long long)g.ldx, (long long)g.ldy);
  if (!codebook_ok(g.codebook)) return glb::api_fail(GLB_EINVAL, "glb_w4_gemm: codebook entry not finite");
  if ((uintptr_t)g.y % 2 || (uintptr_t)g.bias % 2) return glb::api_fail(GLB_EINVAL, "glb_w4_gemm: y / bias not aligned");
  if (g.m > GEMM_MAX_ROWS)
    return glb::api_fail(GLB_EUNSUPPORTED, "glb_w4_gemm serves up to %d rows (dequantise and use the library GEMM)", GEMM_MAX_ROWS);
  if (!gemm_shape_served(g.n, g.k)) return glb::api_fail(GLB_EUNSUPPORTED, "glb_w4_gemm needs n %% 16 == 0 and k %% 64 == 0");
  if ((uintptr_t)g.x % 16 || g.ldx % 8 || (uintptr_t)g.image % 16)
    return glb::api_fail(GLB_EUNSUPPORTED, "glb_w4_gemm needs X, its row pitch and the image 16-byte aligned");
  if (g.workspace_bytes < glb_w4_gemm_workspace_bytes(g.m, g.n, g.k) || (uintptr_t)g.workspace % 16)
    return glb::api_fail(GLB_ENOSPC, "glb_w4_gemm: workspace too small or not 16-byte aligned");
  static_assert(GEMM_MAX_ROWS <= 16 * GEMM_MAX_MF, "row fragments");
  Codebook cb;
  for (int i = 0; i < 16; ++i) cb.v[i] = g.codebook[i];
  const int ksplit = gemm_ksplit(g.n, g.k);
  if (g.dtype == GLB_BF16) launch_gemm<GLB_BF16>(g, cb, ksplit, (hipStream_t)stream);
  else launch_gemm<GLB_F16>(g, cb, ksplit, (hipStream_t)stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return glb::api_hip_fail(e, "w4 GEMM launch");
  hipLaunchKernelGGL(w4_reduce_kernel, dim3(blocks_for(g.m * g.n, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const float *)g.workspace, ksplit, (int)g.m, (int)g.n, (const uint16_t *)g.bias, (uint16_t *)g.y, g.ldy,
                     g.dtype);
  e = hipGetLastError();
  if (e != hipSuccess) return glb::api_hip_fail(e, "w4 GEMM reduce launch");
  return GLB_OK;
}

}  // extern "C"
