// glb_lora.hip - LoRA merge (include/glb.h: glb_lora_merge_workspace_bytes, glb_lora_merge): out = W + scale * B . A for
// every matrix of an adapter in one launch per W dtype (an adapter has one; grids above 2^24 - 1 blocks are split), so
// switching adapters costs one pass over W.
//
// Contract: for every element (i output feature, j input feature)
//   acc = +0; for t = 0 .. r-1 ascending: acc = fmaf(f32(B[i, t]), f32(A[t, j]), acc)
//   out = round_to_w_dtype(fmaf(scale, acc, f32(W[i, j])))           (round to nearest even)
// The chain runs on v_mfma_f32_32x32x2_f32, which is bit-for-bit such an ascending fmaf chain (two k per instruction,
// k0 then k1; C and D never flush, hipcc keeps f32 denormals on A / B); an odd r is padded with a zero product, exact
// because acc is never -0.  No atomics and no split over t: the bits do not depend on the launch geometry.
//
// Both layouts are one product L . R in the memory layout of W: a tile element (row, col) of W is
//   nn.Linear (W [n_out, k_in]):   row = i, col = j: L[row][t] = B[row, t], R[t][col] = A[t, col]
//   Conv1D    (W [k_in, n_out]):   row = j, col = i: L[row][t] = A[t, row], R[t][col] = B[col, t]
// (fmaf(a, b, c) == fmaf(b, a, c), so the chain is the same one), with L / R read by element strides.
//
// Tiling: 128 x 128 tile of W per 256-thread block; wave w owns rows 32 w .. 32 w + 31 and all 128 columns as four 32 x 32
// MFMA tiles, tile c holding the columns 4 n + c (n = lane & 31): every lane then has four CONSECUTIVE columns of each of
// its 16 accumulator rows, and W / out move as 4-element vectors.  W is loaded into registers before the MFMAs (its
// latency hides under them), A and B are staged through LDS as f32, 32 values of t at a time.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/glb.h"
#include "glb_common.hpp"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

constexpr int BM = 128, BN = 128, TK = 32, THREADS = 256;
constexpr int LDS_PITCH = BM + 4;  // floats per t row of the staged chunks: 4 t + row spreads a t-fastest wave over 64 banks
constexpr int MAX_GRID = (1 << 24) - 1;  // blocks per launch (an HSA dispatch holds at most 2^32 work-items)
constexpr int MAX_RANK = 256;
constexpr int64_t MAX_DIM = 1 << 30;

// one matrix as the kernel reads it (the workspace holds an array of these, in launch order)
struct Job {
  const void *w;
  void *out;
  const void *l;  // L[row][t] = l[row * l_row + t * l_t]
  const void *rm; // R[t][col] = rm[t * r_t + col * r_col]
  int64_t ldw, ldo, l_row, l_t, r_t, r_col;
  int32_t rows, cols, rank, ab_dtype;
  float scale;
  int32_t tiles_n;     // column tiles
  int32_t tile_begin;  // first block of this job in its launch
  int32_t vec;         // W / out and their pitches allow 4-element vector accesses
};

__device__ __forceinline__ float ab_load(const void *p, int64_t idx, int dt) {
  if (dt == GLB_F32) return ((const float *)p)[idx];
  const uint16_t h = ((const uint16_t *)p)[idx];
  if (dt == GLB_BF16) return __uint_as_float((uint32_t)h << 16);
  return __half2float(__ushort_as_half(h));
}

__device__ __forceinline__ uint16_t bf16_rne(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);  // NaN stays NaN (quiet)
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// W element types: how a 4-element group is held in registers, widened and narrowed
template <int WDT>
struct WType;
template <>
struct WType<GLB_F32> {
  typedef u32x4 raw4;
  typedef float elem;
  static __device__ __forceinline__ uint32_t get(const raw4 &r, int c) { return r[c]; }
  static __device__ __forceinline__ void set(raw4 &r, int c, uint32_t v) { r[c] = v; }
  static __device__ __forceinline__ float widen(uint32_t v) { return __uint_as_float(v); }
  static __device__ __forceinline__ uint32_t narrow(float f) { return __float_as_uint(f); }
};
template <int WDT>
struct WType16 {
  typedef u32x2 raw4;
  typedef uint16_t elem;
  static __device__ __forceinline__ uint32_t get(const raw4 &r, int c) { return (r[c >> 1] >> (16 * (c & 1))) & 0xffffu; }
  static __device__ __forceinline__ void set(raw4 &r, int c, uint32_t v) {
    const int s = 16 * (c & 1);
    r[c >> 1] = (r[c >> 1] & ~(0xffffu << s)) | (v << s);
  }
  static __device__ __forceinline__ float widen(uint32_t v) {
    return WDT == GLB_BF16 ? __uint_as_float(v << 16) : __half2float(__ushort_as_half((uint16_t)v));
  }
  static __device__ __forceinline__ uint32_t narrow(float f) {
    // (the barrier keeps the f32 result: otherwise fma + convert become ONE v_fma_mix*_f16 - a single rounding of the exact
    // value straight to f16, not the contract's f32 rounding first)
    asm volatile("" : "+v"(f));
    return WDT == GLB_BF16 ? bf16_rne(f) : __half_as_ushort(__float2half_rn(f));
  }
};
template <>
struct WType<GLB_BF16> : WType16<GLB_BF16> {};
template <>
struct WType<GLB_F16> : WType16<GLB_F16> {};

template <int WDT>
__global__ __launch_bounds__(THREADS, 2) void lora_merge_kernel(const Job *__restrict__ jobs, int n_jobs, int block_base) {
  typedef WType<WDT> T;
  typedef typename T::elem elem;
  typedef typename T::raw4 raw4;
  __shared__ __attribute__((aligned(16))) float ls[TK][LDS_PITCH];  // L chunk, t-major: a wave's 32 lanes read 32 consecutive rows
  __shared__ __attribute__((aligned(16))) float rs[TK][LDS_PITCH];  // R chunk: lane n reads columns 4 n .. 4 n + 3

  // this block's job: the last one whose first block is <= blockIdx.x
  int lo = 0, hi = n_jobs - 1;
  const int bid = block_base + (int)blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].tile_begin <= bid) lo = mid;
    else hi = mid - 1;
  }
  const Job &J = jobs[lo];
  const int tile = bid - J.tile_begin;
  const int row0 = (tile / J.tiles_n) * BM, col0 = (tile % J.tiles_n) * BN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, h = lane >> 5;
  const int rows = J.rows, cols = J.cols, g = col0 + 4 * n;
  const bool gfull = J.vec && g + 3 < cols;

  // W in the accumulators' layout, loaded ahead: register reg holds row (reg & 3) + 8 (reg >> 2) + 4 h of the wave's 32
  raw4 wr[16];
  const elem *w = (const elem *)J.w;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int row = row0 + wave * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
    wr[reg] = raw4{};
    if (row < rows) {
      const elem *src = w + (int64_t)row * J.ldw + g;
      if (gfull) {
        wr[reg] = *(const raw4 *)src;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (g + c >= cols) break;
          if constexpr (WDT == GLB_F32) T::set(wr[reg], c, __float_as_uint(src[c]));
          else T::set(wr[reg], c, (uint32_t)src[c]);
        }
      }
    }
  }

  f32x16 acc[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc[c] = f32x16{};

  const int rank = J.rank, adt = J.ab_dtype;
  const bool l_t_fast = J.l_t == 1, r_t_fast = J.r_t == 1;
  for (int t0 = 0; t0 < rank; t0 += TK) {
    // this chunk's values of t, rounded up to a power of two >= 2: only those are staged (r = 16 stages 16, not 32)
    const int tk = min(TK, rank - t0), lg = tk <= 2 ? 1 : 32 - __builtin_clz(tk - 1), tkp = 1 << lg;
    __syncthreads();  // (the previous chunk is read by every wave)
    for (int idx = tid; idx < tkp * BM; idx += THREADS) {
      const int t = l_t_fast ? idx & (tkp - 1) : idx / BM, row = l_t_fast ? idx >> lg : idx % BM;
      const int gt = t0 + t, gr = row0 + row;
      ls[t][row] = (gt < rank && gr < rows) ? ab_load(J.l, (int64_t)gr * J.l_row + (int64_t)gt * J.l_t, adt) : 0.0f;
    }
    for (int idx = tid; idx < tkp * BN; idx += THREADS) {
      const int t = r_t_fast ? idx & (tkp - 1) : idx / BN, col = r_t_fast ? idx >> lg : idx % BN;
      // column col of the chunk is memory column col0 + col; it sits at rs[t][col] (lane n reads 4 n .. 4 n + 3)
      const int gt = t0 + t, gc = col0 + col;
      rs[t][col] = (gt < rank && gc < cols) ? ab_load(J.rm, (int64_t)gt * J.r_t + (int64_t)gc * J.r_col, adt) : 0.0f;
    }
    __syncthreads();
    const int steps = (tk + 1) >> 1;  // (an odd tail takes one zero product: slot tk < tkp was staged as 0)
    for (int s = 0; s < steps; ++s) {
      const float a = ls[2 * s + h][wave * 32 + n];
      const f32x4 b = *(const f32x4 *)&rs[2 * s + h][4 * n];
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[c], acc[c], 0, 0, 0);
    }
  }

  // epilogue: out = round(fmaf(scale, acc, W)); accumulator tile c holds memory column g + c
  const float scale = J.scale;
  elem *out = (elem *)J.out;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int row = row0 + wave * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
    if (row >= rows) continue;
    raw4 o{};
#pragma unroll
    for (int c = 0; c < 4; ++c) T::set(o, c, T::narrow(__builtin_fmaf(scale, acc[c][reg], T::widen(T::get(wr[reg], c)))));
    elem *dst = out + (int64_t)row * J.ldo + g;
    if (gfull) {
      *(raw4 *)dst = o;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (g + c >= cols) break;
        if constexpr (WDT == GLB_F32) dst[c] = __uint_as_float(T::get(o, c));
        else dst[c] = (uint16_t)T::get(o, c);
      }
    }
  }
}

size_t elem_bytes(int32_t dt) { return dt == GLB_F32 ? 4 : 2; }
bool dtype_ok(int32_t dt) { return dt == GLB_F32 || dt == GLB_BF16 || dt == GLB_F16; }

// byte ranges [lo, hi) of a strided matrix
void extent(const void *p, int64_t rows, int64_t cols, int64_t ld, size_t es, uintptr_t &lo, uintptr_t &hi) {
  lo = (uintptr_t)p;
  hi = lo + ((size_t)(rows - 1) * (size_t)ld + (size_t)cols) * es;
}
bool overlap(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; }
struct Extents {
  uintptr_t o0, o1;
  uintptr_t in[6];  // w, a, b
};

}  // namespace

extern "C" {

size_t glb_lora_merge_workspace_bytes(int32_t n_jobs) {
  if (n_jobs <= 0) return 0;
  return ((size_t)n_jobs * sizeof(Job) + 255) & ~(size_t)255;
}

int glb_lora_merge(const glb_lora_job *jobs, int32_t n_jobs, void *workspace, size_t workspace_bytes, void *stream) {
  if (!jobs || n_jobs <= 0) return glb::api_fail(GLB_EINVAL, "no jobs");
  if (!workspace) return glb::api_fail(GLB_EINVAL, "null workspace");
  if (workspace_bytes < glb_lora_merge_workspace_bytes(n_jobs))
    return glb::api_fail(GLB_ENOSPC, "lora workspace %zu bytes < %zu", workspace_bytes, glb_lora_merge_workspace_bytes(n_jobs));
  if (((uintptr_t)workspace) % 16) return glb::api_fail(GLB_EINVAL, "lora workspace not 16-byte aligned");
  std::vector<Job> table;
  std::vector<int32_t> wdt;
  std::vector<Extents> ext;
  table.reserve(n_jobs);
  for (int32_t i = 0; i < n_jobs; ++i) {
    const glb_lora_job &q = jobs[i];
    if (q.struct_size != sizeof(glb_lora_job))
      return glb::api_fail(GLB_EINVAL, "glb_lora_job[%d].struct_size %u != %zu (ABI mismatch)", i, q.struct_size,
                           sizeof(glb_lora_job));
    if (!dtype_ok(q.w_dtype) || !dtype_ok(q.ab_dtype) || (q.w_transposed != 0 && q.w_transposed != 1))
      return glb::api_fail(GLB_EINVAL, "glb_lora_job[%d]: bad dtype / layout (%d, %d, %d)", i, q.w_dtype, q.ab_dtype,
                           q.w_transposed);
    if (!q.w || !q.a || !q.b || !q.out) return glb::api_fail(GLB_EINVAL, "glb_lora_job[%d]: null pointer", i);
    if (q.n_out <= 0 || q.k_in <= 0 || q.r <= 0)
      return glb::api_fail(GLB_EINVAL, "glb_lora_job[%d]: bad shape (n_out %lld, k_in %lld, r %lld)", i, (long long)q.n_out,
                           (long long)q.k_in, (long long)q.r);
    const int64_t rows = q.w_transposed ? q.k_in : q.n_out, cols = q.w_transposed ? q.n_out : q.k_in;
    if (q.ldw < cols || q.ldo < cols || q.lda < q.k_in || q.ldb < q.r)
      return glb::api_fail(GLB_EINVAL, "glb_lora_job[%d]: row pitch below the row (ldw %lld, ldo %lld, lda %lld, ldb %lld)", i,
                           (long long)q.ldw, (long long)q.ldo, (long long)q.lda, (long long)q.ldb);
    const size_t es = elem_bytes(q.w_dtype), as = elem_bytes(q.ab_dtype);
    if ((uintptr_t)q.w % es || (uintptr_t)q.out % es || (uintptr_t)q.a % as || (uintptr_t)q.b % as)
      return glb::api_fail(GLB_EINVAL, "glb_lora_job[%d]: pointer not aligned to its element", i);
    if (q.r > MAX_RANK) return glb::api_fail(GLB_EUNSUPPORTED, "glb_lora_job[%d]: rank %lld > %d", i, (long long)q.r, MAX_RANK);
    if (rows > MAX_DIM || cols > MAX_DIM)
      return glb::api_fail(GLB_EUNSUPPORTED, "glb_lora_job[%d]: more than 2^30 rows or columns", i);
    Extents x;
    extent(q.out, rows, cols, q.ldo, es, x.o0, x.o1);
    extent(q.w, rows, cols, q.ldw, es, x.in[0], x.in[1]);
    extent(q.a, q.r, q.k_in, q.lda, as, x.in[2], x.in[3]);
    extent(q.b, q.n_out, q.r, q.ldb, as, x.in[4], x.in[5]);
    ext.push_back(x);
    Job j{};
    j.w = q.w;
    j.out = q.out;
    j.ldw = q.ldw;
    j.ldo = q.ldo;
    if (q.w_transposed) {  // L[row = j][t] = A[t, j], R[t][col = i] = B[i, t]
      j.l = q.a, j.l_row = 1, j.l_t = q.lda;
      j.rm = q.b, j.r_t = 1, j.r_col = q.ldb;
    } else {  // L[row = i][t] = B[i, t], R[t][col = j] = A[t, j]
      j.l = q.b, j.l_row = q.ldb, j.l_t = 1;
      j.rm = q.a, j.r_t = q.lda, j.r_col = 1;
    }
    j.rows = (int32_t)rows;
    j.cols = (int32_t)cols;
    j.rank = (int32_t)q.r;
    j.ab_dtype = q.ab_dtype;
    j.scale = q.scale;
    j.tiles_n = (int32_t)((cols + BN - 1) / BN);
    j.vec = ((uintptr_t)q.w % (4 * es) == 0 && (uintptr_t)q.out % (4 * es) == 0 && q.ldw % 4 == 0 && q.ldo % 4 == 0);
    table.push_back(j);
    wdt.push_back(q.w_dtype);
  }
  // no job's out may overlap any job's w, a, b or (another job's) out: blocks of one call run in any order
  for (int32_t i = 0; i < n_jobs; ++i)
    for (int32_t k = 0; k < n_jobs; ++k) {
      const Extents &o = ext[i], &x = ext[k];
      if (overlap(o.o0, o.o1, x.in[0], x.in[1]) || overlap(o.o0, o.o1, x.in[2], x.in[3]) ||
          overlap(o.o0, o.o1, x.in[4], x.in[5]) || (k != i && overlap(o.o0, o.o1, x.o0, x.o1)))
        return glb::api_fail(GLB_EINVAL, "glb_lora_job[%d]: out overlaps w, a, b or out of job %d", i, k);
    }
  // one launch per W dtype present, its jobs contiguous in the table
  std::vector<Job> sorted;
  sorted.reserve(n_jobs);
  int64_t first[3] = {0, 0, 0}, count[3] = {0, 0, 0}, blocks[3] = {0, 0, 0};
  for (int dt = 0; dt < 3; ++dt) {
    first[dt] = (int64_t)sorted.size();
    for (int32_t i = 0; i < n_jobs; ++i) {
      if (wdt[i] != dt) continue;
      Job j = table[i];
      const int64_t tiles = (((int64_t)j.rows + BM - 1) / BM) * j.tiles_n;
      if (blocks[dt] + tiles > INT32_MAX / 2) return glb::api_fail(GLB_EUNSUPPORTED, "lora merge: too many tiles in one call");
      j.tile_begin = (int32_t)blocks[dt];
      blocks[dt] += tiles;
      sorted.push_back(j);
      ++count[dt];
    }
  }
  // (pageable source: the copy is staged before hipMemcpyAsync returns, so `sorted` may go when this call does)
  hipError_t e = hipMemcpyAsync(workspace, sorted.data(), sorted.size() * sizeof(Job), hipMemcpyHostToDevice,
                                (hipStream_t)stream);
  if (e != hipSuccess) return glb::api_hip_fail(e, "lora job table copy");
  const Job *dev = (const Job *)workspace;
  for (int dt = 0; dt < 3; ++dt) {
    // (a grid of at most MAX_GRID blocks per launch; more blocks take further launches over the same table)
    for (int64_t base = 0; base < blocks[dt]; base += MAX_GRID) {
      const dim3 grid((unsigned)std::min<int64_t>(MAX_GRID, blocks[dt] - base)), block(THREADS);
      const Job *tab = dev + first[dt];
      const int nj = (int)count[dt], b0 = (int)base;
      if (dt == GLB_F32)
        hipLaunchKernelGGL(lora_merge_kernel<GLB_F32>, grid, block, 0, (hipStream_t)stream, tab, nj, b0);
      else if (dt == GLB_BF16)
        hipLaunchKernelGGL(lora_merge_kernel<GLB_BF16>, grid, block, 0, (hipStream_t)stream, tab, nj, b0);
      else
        hipLaunchKernelGGL(lora_merge_kernel<GLB_F16>, grid, block, 0, (hipStream_t)stream, tab, nj, b0);
      e = hipGetLastError();
      if (e != hipSuccess) return glb::api_hip_fail(e, "lora merge launch");
    }
  }
  return GLB_OK;
}

}  // extern "C"
