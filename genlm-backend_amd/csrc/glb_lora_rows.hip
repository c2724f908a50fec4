// glb_lora_rows.hip - LoRA in peft's UNMERGED form with the adapter chosen per row (include/glb.h: glb_lora_rows_table_bytes,
// glb_lora_rows_table_upload, glb_lora_rows_workspace_bytes, glb_lora_rows):
//   slot = row_slot[m];  slot < 0 or no entry for this module: Y[m, :] is not written
//   else Y[m, n] = round_to_y_dtype(fmaf(scale, sum_t B[n, t] * T[m, t], f32(Y[m, n]))),  T[m, t] = sum_k A[t, k] * X[m, k]
// Two launches, no atomics: SHRINK makes T [M, r] in the caller's workspace, EXPAND adds B . T to Y in place.
//
// Arithmetic (the contract of the header).  Both phases run on MFMA with float32 accumulation.
//   * X and A / B of ONE 16-bit dtype: v_mfma_f32_16x16x32_{bf16,f16}; T is rounded once to that dtype (RNE) between the
//     phases - what a 16-bit framework GEMM pair does as well.
//   * every other combination (float32 X, or A / B of another dtype than X): the operands are widened to float32 (exact) and
//     both phases run on v_mfma_f32_16x16x4_f32; T stays float32.
//   * k is summed in chunks of 32; chunk c belongs to wave c % 4 of the block, every wave sums its chunks in ascending order
//     and the four partial sums are added as ((w0 + w1) + w2) + w3 through LDS.  t is summed ascending by one wave.
// The bits of row m therefore depend on X[m, :], Y[m, :] and its slot's A, B, scale only - not on M, on other rows' slots or
// values, or on the position of the launch in a graph: a row of an MFMA tile is computed from that row of the operand alone,
// and rows of other slots (or beyond M) enter a tile as zeros.
//
// Rows of several adapters in one tile: a block takes the distinct slots of its rows one after the other (first appearance),
// each pass with the other rows' operand zeroed and only its own rows written.
//
// Tiling.  SHRINK: a 256-thread block owns 16 rows and all r columns of T; lane (c = lane & 15, q = lane >> 4) holds X[m0 + c]
// [k0 + 8 q .. + 8) as the A operand and A[16 tt + c][k0 + 8 q .. + 8) as the B operand of tile tt (16-byte loads; A comes
// from L2 - it is read by every block).  EXPAND: a block owns 32 rows x 512 columns, a wave 32 x 128 as two passes of 64; the
// roles are swapped (B rows are the MFMA's A operand, T rows its B operand) and MFMA row rho of tile c stands for column
// n0 + 16 (rho >> 2) + 4 c + (rho & 3), so that a lane ends up with 16 CONSECUTIVE columns of one row: Y moves as 16-byte
// vectors.  Vector accesses need 16-byte aligned pointers and pitches (flags made by the host); anything else is served by
// element accesses, so every N, K >= 1 works.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cstdint>
#include <type_traits>
#include <vector>

#include "../../include/glb.h"
#include "glb_common.hpp"

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

constexpr int MAX_RANK = 256, MAX_SLOTS = 64, MAX_MODULES = 4096;
constexpr int WAVES = 4, THREADS = 64 * WAVES;
constexpr int ROWS_S = 16;                             // rows of a shrink block
constexpr int ROWS_E = 32, COLS_P = 64, PASSES = 2;    // expand: rows of a block, columns of a wave's pass, passes of a wave
constexpr int COLS_E = WAVES * PASSES * COLS_P;        // columns of an expand block
constexpr int64_t MAX_DIM = 1 << 30;

// one (slot, module) of the device table; rank 0: the adapter does not target the module
struct Entry {
  const void *a, *b;
  int64_t lda, ldb;
  int32_t n_out, k_in, rank, dtype;
  float scale;
  int32_t vec_a, vec_b;  // 16-byte loads of 8 elements are allowed on a / b rows
  int32_t pad;
};
static_assert(sizeof(Entry) == 64, "Entry layout");

struct Params {
  const void *x;
  void *y;
  const int32_t *row_slot;
  const Entry *table;
  char *t;  // workspace: row m at t + m * t_pitch bytes
  int64_t m, ldx, ldy, t_pitch;
  int32_t n, k, n_slots, n_modules, module, r_max, vec_x, vec_y;
};

__device__ __forceinline__ uint16_t bf16_rne(float f) {
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);  // NaN stays NaN (quiet)
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

__device__ __forceinline__ float widen16(uint32_t h, int dt) {
  return dt == GLB_BF16 ? __uint_as_float(h << 16) : __half2float(__ushort_as_half((uint16_t)h));
}

template <int DT>
__device__ __forceinline__ uint32_t narrow16(float f) {
  // (the barrier keeps the f32 value: fma + convert must not become one v_fma_mix*_f16 with a single rounding)
  asm volatile("" : "+v"(f));
  return DT == GLB_BF16 ? (uint32_t)bf16_rne(f) : (uint32_t)__half_as_ushort(__float2half_rn(f));
}

// elements [i0, i0 + 8) of a 16-bit row whose valid elements are [0, lim), raw; zeros where invalid or !on
__device__ __forceinline__ u32x4 load8_raw16(const void *row, int i0, int lim, bool vec, bool on) {
  u32x4 r{};
  if (!on || i0 >= lim) return r;
  const uint16_t *p = (const uint16_t *)row + i0;
  if (vec && i0 + 8 <= lim) return *(const u32x4 *)p;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (i0 + j < lim) r[j >> 1] |= (uint32_t)p[j] << (16 * (j & 1));
  return r;
}

// the same elements of a row of dtype dt, widened to float32
__device__ __forceinline__ void load8_f32(const void *row, int dt, int i0, int lim, bool vec, bool on, float (&o)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = 0.0f;
  if (!on || i0 >= lim) return;
  if (dt == GLB_F32) {
    const float *p = (const float *)row + i0;
    if (vec && i0 + 8 <= lim) {
      const f32x4 lo = *(const f32x4 *)p, hi = *(const f32x4 *)(p + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = lo[j], o[4 + j] = hi[j];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (i0 + j < lim) o[j] = p[j];
    }
  } else {
    const u32x4 r = load8_raw16(row, i0, lim, vec, true);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = widen16((r[j >> 1] >> (16 * (j & 1))) & 0xffffu, dt);
  }
}

template <int DT>
__device__ __forceinline__ f32x4 mma16(u32x4 a, u32x4 b, f32x4 c) {
  if constexpr (DT == GLB_BF16)
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// eight k of a chunk on the float32 MFMA: step j takes element j of every quarter (k = k0 + 8 q + j), ascending j
__device__ __forceinline__ f32x4 mma32(const float (&a)[8], const float (&b)[8], f32x4 c) {
#pragma unroll
  for (int j = 0; j < 8; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], c, 0, 0, 0);
  return c;
}

// the slot of row m as both kernels see it: -1 for rows beyond M, base rows, slots outside the table, adapters without this
// module and entries that do not fit the call
__device__ __forceinline__ int row_slot_of(const Params &P, int64_t m) {
  if (m >= P.m) return -1;
  const int s = P.row_slot[m];
  if (s < 0 || s >= P.n_slots) return -1;
  const Entry &e = P.table[(int64_t)s * P.n_modules + P.module];
  if (e.rank <= 0 || e.rank > P.r_max || e.n_out != P.n || e.k_in != P.k) return -1;
  return s;
}

constexpr size_t elem_size(int dt) { return dt == GLB_F32 ? 4 : 2; }

// ---- shrink: T[m, t] = sum_k X[m, k] A[t, k] -----------------------------------------------------------------------------
template <int XDT, int NT>  // NT: 16-column tiles of T a block can hold (r_max <= 16 NT)
__global__ __launch_bounds__(THREADS) void lora_shrink_kernel(const Params P) {
  __shared__ f32x4 red[WAVES - 1][NT][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c16 = lane & 15, q = lane >> 4;
  const int64_t m0 = (int64_t)blockIdx.x * ROWS_S, mrow = m0 + c16;
  const int slot = row_slot_of(P, mrow);
  const int K = P.k;
  const char *xrow = (const char *)P.x + (mrow < P.m ? mrow : 0) * P.ldx * (int64_t)elem_size(XDT);
  uint32_t todo = (uint32_t)(__ballot(slot >= 0) & 0xffffull);  // (the same in all four waves: they hold the same rows)
  while (todo) {
    const int s = __shfl(slot, __builtin_ctz(todo));
    const bool mine = slot == s;
    todo &= ~(uint32_t)(__ballot(mine) & 0xffffull);
    const Entry e = P.table[(int64_t)s * P.n_modules + P.module];
    const int rank = e.rank, nt = (rank + 15) >> 4;
    const bool m16 = XDT != GLB_F32 && e.dtype == XDT;
    const int64_t a_pitch = e.lda * (int64_t)elem_size(e.dtype);
    f32x4 acc[NT];
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) acc[tt] = f32x4{};
    for (int k0 = wave * 32; k0 < K; k0 += WAVES * 32) {
      const int kk = k0 + 8 * q;
      if (m16) {
        if constexpr (XDT != GLB_F32) {
          const u32x4 xa = load8_raw16(xrow, kk, K, P.vec_x, mine);
#pragma unroll
          for (int tt = 0; tt < NT; ++tt) {
            if (tt >= nt) continue;
            const int t = tt * 16 + c16;
            const u32x4 b = load8_raw16((const char *)e.a + (t < rank ? t : 0) * a_pitch, kk, K, e.vec_a, t < rank);
            acc[tt] = mma16<XDT>(xa, b, acc[tt]);
          }
        }
      } else {
        float xa[8];
        load8_f32(xrow, XDT, kk, K, P.vec_x, mine, xa);
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
          if (tt >= nt) continue;
          const int t = tt * 16 + c16;
          float b[8];
          load8_f32((const char *)e.a + (t < rank ? t : 0) * a_pitch, e.dtype, kk, K, e.vec_a, t < rank, b);
          acc[tt] = mma32(xa, b, acc[tt]);
        }
      }
    }
    if (wave > 0) {
#pragma unroll
      for (int tt = 0; tt < NT; ++tt)
        if (tt < nt) red[wave - 1][tt][lane] = acc[tt];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) {
        if (tt >= nt) continue;
        f32x4 v = acc[tt];
#pragma unroll
        for (int w = 0; w < WAVES - 1; ++w) v += red[w][tt][lane];
        const int t = tt * 16 + c16;  // accumulator layout: column on lane & 15, rows 4 q + i in the registers
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = 4 * q + i;
          if (__shfl(slot, r) != s) continue;
          char *trow = P.t + (m0 + r) * P.t_pitch;
          if (m16) {
            if constexpr (XDT != GLB_F32) ((uint16_t *)trow)[t] = (uint16_t)narrow16<XDT>(v[i]);
          } else {
            ((float *)trow)[t] = v[i];
          }
        }
      }
    }
    __syncthreads();  // (red is written again by the next pass)
  }
}

// ---- expand: Y[m, n] += scale * sum_t B[n, t] T[m, t] --------------------------------------------------------------------
template <int XDT>
__global__ __launch_bounds__(THREADS) void lora_expand_kernel(const Params P) {
  typedef typename std::conditional<XDT == GLB_F32, float, uint16_t>::type elem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c16 = lane & 15, q = lane >> 4;
  const int64_t m0 = (int64_t)blockIdx.x * ROWS_E;
  const int N = P.n, nbase = (int)blockIdx.y * COLS_E + wave * PASSES * COLS_P;
  if (nbase >= N) return;  // (no barrier below)
  int slot[2];
  uint32_t todo = 0;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    slot[mt] = row_slot_of(P, m0 + mt * 16 + c16);
    todo |= (uint32_t)(__ballot(slot[mt] >= 0) & 0xffffull) << (16 * mt);
  }
  while (todo) {
    const int first = __builtin_ctz(todo);
    const int s0 = __shfl(slot[0], first & 15), s1 = __shfl(slot[1], first & 15);
    const int s = first < 16 ? s0 : s1;
    bool mine[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      mine[mt] = slot[mt] == s;
      todo &= ~((uint32_t)(__ballot(mine[mt]) & 0xffffull) << (16 * mt));
    }
    const Entry e = P.table[(int64_t)s * P.n_modules + P.module];
    const int rank = e.rank;
    const bool m16 = XDT != GLB_F32 && e.dtype == XDT;
    const int64_t b_pitch = e.ldb * (int64_t)elem_size(e.dtype);
    const char *trow[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) trow[mt] = P.t + (mine[mt] ? m0 + mt * 16 + c16 : 0) * P.t_pitch;
    for (int pass = 0; pass < PASSES; ++pass) {
      const int n0 = nbase + pass * COLS_P;
      if (n0 >= N) break;
      f32x4 acc[2][4];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[mt][c] = f32x4{};
      for (int t0 = 0; t0 < rank; t0 += 32) {
        const int tk = t0 + 8 * q;
        if (m16) {
          if constexpr (XDT != GLB_F32) {
            u32x4 tb[2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) tb[mt] = load8_raw16(trow[mt], tk, rank, true, mine[mt]);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const int n = n0 + 16 * (c16 >> 2) + 4 * c + (c16 & 3);
              const u32x4 bf = load8_raw16((const char *)e.b + (n < N ? n : 0) * b_pitch, tk, rank, e.vec_b, n < N);
#pragma unroll
              for (int mt = 0; mt < 2; ++mt) acc[mt][c] = mma16<XDT>(bf, tb[mt], acc[mt][c]);
            }
          }
        } else {
          float tb[2][8];
#pragma unroll
          for (int mt = 0; mt < 2; ++mt) load8_f32(trow[mt], GLB_F32, tk, rank, true, mine[mt], tb[mt]);
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int n = n0 + 16 * (c16 >> 2) + 4 * c + (c16 & 3);
            float bf[8];
            load8_f32((const char *)e.b + (n < N ? n : 0) * b_pitch, e.dtype, tk, rank, e.vec_b, n < N, bf);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) acc[mt][c] = mma32(bf, tb[mt], acc[mt][c]);
          }
        }
      }
      // epilogue: the lane holds columns ncol + 4 c + i (c tile, i register) of row m0 + 16 mt + c16
      const int ncol = n0 + 16 * q;
      if (ncol >= N) continue;
      const bool full = P.vec_y && ncol + 16 <= N;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        if (!mine[mt]) continue;
        elem *yp = (elem *)P.y + (m0 + mt * 16 + c16) * P.ldy + ncol;
        if (full) {
          if constexpr (XDT == GLB_F32) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              f32x4 v = *(const f32x4 *)(yp + 4 * c);
#pragma unroll
              for (int i = 0; i < 4; ++i) v[i] = __builtin_fmaf(e.scale, acc[mt][c][i], v[i]);
              *(f32x4 *)(yp + 4 * c) = v;
            }
          } else {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              u32x4 v = *(const u32x4 *)(yp + 8 * h);
#pragma unroll
              for (int j = 0; j < 8; ++j) {
                const int c = 2 * h + (j >> 2), i = j & 3, sh = 16 * (j & 1);
                const float y = widen16((v[j >> 1] >> sh) & 0xffffu, XDT);
                const uint32_t o = narrow16<XDT>(__builtin_fmaf(e.scale, acc[mt][c][i], y));
                v[j >> 1] = (v[j >> 1] & ~(0xffffu << sh)) | (o << sh);
              }
              *(u32x4 *)(yp + 8 * h) = v;
            }
          }
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int j = 4 * c + i;
              if (ncol + j >= N) continue;
              if constexpr (XDT == GLB_F32) yp[j] = __builtin_fmaf(e.scale, acc[mt][c][i], yp[j]);
              else yp[j] = (uint16_t)narrow16<XDT>(__builtin_fmaf(e.scale, acc[mt][c][i], widen16(yp[j], XDT)));
            }
        }
      }
    }
  }
}

bool dtype_ok(int32_t dt) { return dt == GLB_F32 || dt == GLB_BF16 || dt == GLB_F16; }
int64_t t_pitch_bytes(int32_t r_max) { return (int64_t)((r_max + 31) / 32 * 32) * 4; }

template <int XDT>
hipError_t launch(const Params &P, hipStream_t stream) {
  const dim3 block(THREADS);
  const dim3 gs((unsigned)((P.m + ROWS_S - 1) / ROWS_S));
  if (P.r_max <= 64) hipLaunchKernelGGL((lora_shrink_kernel<XDT, 4>), gs, block, 0, stream, P);
  else hipLaunchKernelGGL((lora_shrink_kernel<XDT, 16>), gs, block, 0, stream, P);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 ge((unsigned)((P.m + ROWS_E - 1) / ROWS_E), (unsigned)((P.n + COLS_E - 1) / COLS_E));
  hipLaunchKernelGGL(lora_expand_kernel<XDT>, ge, block, 0, stream, P);
  return hipGetLastError();
}

}  // namespace

extern "C" {

size_t glb_lora_rows_table_bytes(int32_t n_slots, int32_t n_modules) {
  if (n_slots <= 0 || n_modules <= 0 || n_slots > MAX_SLOTS || n_modules > MAX_MODULES) return 0;
  return ((size_t)n_slots * (size_t)n_modules * sizeof(Entry) + 255) & ~(size_t)255;
}

int glb_lora_rows_table_upload(const glb_lora_rows_entry *entries, int32_t n_slots, int32_t n_modules, void *table,
                               size_t table_bytes, void *stream) {
  if (!entries || n_slots <= 0 || n_modules <= 0) return glb::api_fail(GLB_EINVAL, "lora rows table: no entries");
  if (n_slots > MAX_SLOTS || n_modules > MAX_MODULES)
    return glb::api_fail(GLB_EUNSUPPORTED, "lora rows table: %d slots x %d modules (at most %d x %d)", n_slots, n_modules,
                         MAX_SLOTS, MAX_MODULES);
  if (!table || ((uintptr_t)table) % 16) return glb::api_fail(GLB_EINVAL, "lora rows table: null or not 16-byte aligned");
  if (table_bytes < glb_lora_rows_table_bytes(n_slots, n_modules))
    return glb::api_fail(GLB_ENOSPC, "lora rows table %zu bytes < %zu", table_bytes, glb_lora_rows_table_bytes(n_slots, n_modules));
  const size_t count = (size_t)n_slots * (size_t)n_modules;
  std::vector<Entry> host(count);
  for (size_t i = 0; i < count; ++i) {
    const glb_lora_rows_entry &q = entries[i];
    const int si = (int)(i / n_modules), mi = (int)(i % n_modules);
    if (q.struct_size != sizeof(glb_lora_rows_entry))
      return glb::api_fail(GLB_EINVAL, "glb_lora_rows_entry[%d][%d].struct_size %u != %zu (ABI mismatch)", si, mi, q.struct_size,
                           sizeof(glb_lora_rows_entry));
    Entry e{};
    if (q.r == 0) {  // the adapter does not target the module
      host[i] = e;
      continue;
    }
    if (!dtype_ok(q.ab_dtype)) return glb::api_fail(GLB_EINVAL, "glb_lora_rows_entry[%d][%d]: bad dtype %d", si, mi, q.ab_dtype);
    if (!q.a || !q.b) return glb::api_fail(GLB_EINVAL, "glb_lora_rows_entry[%d][%d]: null pointer", si, mi);
    if (q.n_out <= 0 || q.k_in <= 0 || q.r < 0)
      return glb::api_fail(GLB_EINVAL, "glb_lora_rows_entry[%d][%d]: bad shape (n_out %lld, k_in %lld, r %lld)", si, mi,
                           (long long)q.n_out, (long long)q.k_in, (long long)q.r);
    if (q.lda < q.k_in || q.ldb < q.r)
      return glb::api_fail(GLB_EINVAL, "glb_lora_rows_entry[%d][%d]: row pitch below the row (lda %lld, ldb %lld)", si, mi,
                           (long long)q.lda, (long long)q.ldb);
    const size_t as = elem_size(q.ab_dtype);
    if ((uintptr_t)q.a % as || (uintptr_t)q.b % as)
      return glb::api_fail(GLB_EINVAL, "glb_lora_rows_entry[%d][%d]: pointer not aligned to its element", si, mi);
    if (q.r > MAX_RANK)
      return glb::api_fail(GLB_EUNSUPPORTED, "glb_lora_rows_entry[%d][%d]: rank %lld > %d", si, mi, (long long)q.r, MAX_RANK);
    if (q.n_out > MAX_DIM || q.k_in > MAX_DIM || q.lda > MAX_DIM || q.ldb > MAX_DIM)
      return glb::api_fail(GLB_EUNSUPPORTED, "glb_lora_rows_entry[%d][%d]: more than 2^30 rows or columns", si, mi);
    e.a = q.a, e.b = q.b, e.lda = q.lda, e.ldb = q.ldb;
    e.n_out = (int32_t)q.n_out, e.k_in = (int32_t)q.k_in, e.rank = (int32_t)q.r, e.dtype = q.ab_dtype;
    e.scale = q.scale;
    e.vec_a = (uintptr_t)q.a % 16 == 0 && (q.lda * as) % 16 == 0;
    e.vec_b = (uintptr_t)q.b % 16 == 0 && (q.ldb * as) % 16 == 0;
    host[i] = e;
  }
  // (pageable source: the copy is staged before hipMemcpyAsync returns, so `host` may go when this call does)
  hipError_t err = hipMemcpyAsync(table, host.data(), count * sizeof(Entry), hipMemcpyHostToDevice, (hipStream_t)stream);
  if (err != hipSuccess) return glb::api_hip_fail(err, "lora rows table copy");
  return GLB_OK;
}

size_t glb_lora_rows_workspace_bytes(int64_t m, int32_t r_max) {
  if (m <= 0 || r_max <= 0 || r_max > MAX_RANK || m > ((int64_t)1 << 40)) return 0;
  return ((size_t)m * (size_t)t_pitch_bytes(r_max) + 255) & ~(size_t)255;
}

int glb_lora_rows(const glb_lora_rows_args *a, void *stream) {
  if (!a) return glb::api_fail(GLB_EINVAL, "null glb_lora_rows_args");
  if (a->struct_size != sizeof(glb_lora_rows_args))
    return glb::api_fail(GLB_EINVAL, "glb_lora_rows_args.struct_size %u != %zu (ABI mismatch)", a->struct_size,
                         sizeof(glb_lora_rows_args));
  if (!dtype_ok(a->dtype)) return glb::api_fail(GLB_EINVAL, "lora rows: bad dtype %d", a->dtype);
  if (!a->x || !a->y || !a->row_slot || !a->table || !a->workspace) return glb::api_fail(GLB_EINVAL, "lora rows: null pointer");
  if (a->m <= 0 || a->n <= 0 || a->k <= 0)
    return glb::api_fail(GLB_EINVAL, "lora rows: bad shape (m %lld, n %lld, k %lld)", (long long)a->m, (long long)a->n,
                         (long long)a->k);
  if (a->ldx < a->k || a->ldy < a->n)
    return glb::api_fail(GLB_EINVAL, "lora rows: row pitch below the row (ldx %lld, ldy %lld)", (long long)a->ldx, (long long)a->ldy);
  if (a->n_slots <= 0 || a->n_modules <= 0 || a->module < 0 || a->module >= a->n_modules || a->r_max <= 0)
    return glb::api_fail(GLB_EINVAL, "lora rows: bad table shape (%d slots, %d modules, module %d, r_max %d)", a->n_slots,
                         a->n_modules, a->module, a->r_max);
  const size_t es = elem_size(a->dtype);
  if ((uintptr_t)a->x % es || (uintptr_t)a->y % es || (uintptr_t)a->row_slot % 4 || (uintptr_t)a->table % 16 ||
      (uintptr_t)a->workspace % 16)
    return glb::api_fail(GLB_EINVAL, "lora rows: pointer not aligned (x, y: element; row_slot: 4; table, workspace: 16 bytes)");
  if (a->r_max > MAX_RANK) return glb::api_fail(GLB_EUNSUPPORTED, "lora rows: r_max %d > %d", a->r_max, MAX_RANK);
  if (a->n_slots > MAX_SLOTS || a->n_modules > MAX_MODULES)
    return glb::api_fail(GLB_EUNSUPPORTED, "lora rows: %d slots x %d modules (at most %d x %d)", a->n_slots, a->n_modules,
                         MAX_SLOTS, MAX_MODULES);
  if (a->n > MAX_DIM || a->k > MAX_DIM || a->ldx > MAX_DIM || a->ldy > MAX_DIM || a->m > ((int64_t)1 << 31) - 1 - ROWS_S)
    return glb::api_fail(GLB_EUNSUPPORTED, "lora rows: more than 2^30 columns or 2^31 rows");
  if ((a->n + COLS_E - 1) / COLS_E > 65535) return glb::api_fail(GLB_EUNSUPPORTED, "lora rows: n %lld too wide", (long long)a->n);
  const size_t need = glb_lora_rows_workspace_bytes(a->m, a->r_max);
  if (a->workspace_bytes < need) return glb::api_fail(GLB_ENOSPC, "lora rows workspace %zu bytes < %zu", a->workspace_bytes, need);
  const uintptr_t x0 = (uintptr_t)a->x, x1 = x0 + ((size_t)(a->m - 1) * a->ldx + a->k) * es;
  const uintptr_t y0 = (uintptr_t)a->y, y1 = y0 + ((size_t)(a->m - 1) * a->ldy + a->n) * es;
  if (x0 < y1 && y0 < x1) return glb::api_fail(GLB_EINVAL, "lora rows: x and y overlap");
  Params P{};
  P.x = a->x, P.y = a->y, P.row_slot = (const int32_t *)a->row_slot, P.table = (const Entry *)a->table;
  P.t = (char *)a->workspace;
  P.m = a->m, P.ldx = a->ldx, P.ldy = a->ldy, P.t_pitch = t_pitch_bytes(a->r_max);
  P.n = (int32_t)a->n, P.k = (int32_t)a->k, P.n_slots = a->n_slots, P.n_modules = a->n_modules, P.module = a->module;
  P.r_max = a->r_max;
  P.vec_x = x0 % 16 == 0 && (a->ldx * es) % 16 == 0;
  P.vec_y = y0 % 16 == 0 && (a->ldy * es) % 16 == 0;
  hipError_t e = a->dtype == GLB_F32    ? launch<GLB_F32>(P, (hipStream_t)stream)
                 : a->dtype == GLB_BF16 ? launch<GLB_BF16>(P, (hipStream_t)stream)
                                        : launch<GLB_F16>(P, (hipStream_t)stream);
  if (e != hipSuccess) return glb::api_hip_fail(e, "lora rows launch");
  return GLB_OK;
}

}  // extern "C"
