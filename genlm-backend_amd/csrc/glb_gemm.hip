// glb_gemm.hip - fp32 projection GEMM on bf16 MFMA (include/glb.h: glb_gemm_split_bytes, glb_gemm_split_weights,
// glb_gemm_f32_split): C[M, N] = A[M, K] . W[K, N] + bias, optionally followed by the tanh GELU, for GPT-2's Conv1D
// projections (hf modeling_gpt2.py: `addmm(bias, x, weight)`); or followed by the block's residual, C = (A . W + bias) + R
// (glb_gemm_f32_split_residual: the add behind `c_proj` in the GEMM's epilogue).
//
// Numerics ("split bf16"): every fp32 operand element is written as x = hi + mid + lo, three bf16 values made by
// round-to-nearest-even (v_cvt_pk_bf16_f32), each residual an exact fp32 subtraction; the sum is exact for every finite x
// whose parts stay normal.  a.b is then the sum of nine exact bf16 products; the three smallest (mid.lo, lo.mid, lo.lo) are
// below 2^-24 |a||b| together and are dropped.  The other six of one 32-deep K step go into ONE fresh fp32 accumulator,
// smallest first:
//   mid.mid, lo.hi, hi.lo, mid.hi, hi.mid, hi.hi
// and that partial is added to the running sum by a round-to-nearest v_add_f32.  (Chaining every K step through the MFMA's
// own accumulator instead measured 1.6-2.6x torch.addmm's fp32 error on random data: the MFMA's additions into a large
// running sum cost more than 24 rounded adds.)  The result is fp32-accurate - tests/test_split_gemm_cpu.py bounds the
// truncation against float64, tests/test_split_gemm_gpu.py the whole GEMM against torch.addmm - at 6/16 of the MFMA
// cycles of the fp32-input MFMA.
//
// Layout.  W is split once per weight (glb_gemm_split_weights) into a packed image of 1 KiB pieces, one per
// (16 columns, 32 rows of K, plane): piece ((nb * K/32 + kb) * 3 + p) holds, at byte 16 * l, the eight plane-p values
// W[kb*32 + 8(l>>4) + j][nb*16 + (l&15)], j = 0..7 - exactly the B operand of lane l of v_mfma_f32_16x16x32_bf16, so a
// piece is staged with one contiguous 1 KiB global_load_lds per wave and read back with one lane-linear ds_read_b128.
// A stays fp32 and never passes through LDS: each of its elements is used by one wave only, so lane l loads its own operand
// of row fragment mf - the eight floats A[mf*16 + (l&15)][8(l>>4) .. +7], two float4 - straight from global memory into
// registers, one K step ahead of its use, and splits it there.  (The four lanes that share l & 15 read 128 contiguous bytes
// of one row.)
//
// Tiling: one output tile per 256-thread block, K step 32, two LDS stages of the B pieces; wave w owns MF row fragments
// (16 rows each) and all NF column fragments of the tile.  Two forms of the one kernel (Geom below):
//   large: 128 x 128, MF = 2, NF = 8, 48 KiB of LDS, three blocks per CU within 168 VGPRs - wave w owns rows 32w .. 32w+31;
//   small:  64 x  64, MF = 1, NF = 4, 24 KiB of LDS, six blocks per CU - wave w owns rows 16w .. 16w+15.  For launches whose
//          128 x 128 tiles would leave CUs empty (glb_gemm_split_pick).
// An output element is the same chain in either form - six MFMAs on a fresh accumulator per K step, partial sums added in K
// order, bias, GELU - so a call's bits do not depend on the form (tests/test_split_gemm_forms_gpu.py).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "../../include/glb.h"
#include "glb_common.hpp"

namespace {

typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

constexpr int BK = 32, THREADS = 256, WAVES = THREADS / 64;
constexpr int PIECE = 1024;  // bytes of one staged piece (64 lanes x 16 B)

// tile geometry: MF row fragments per wave, NF column fragments per block, BLOCKS blocks per CU
template <int MF_, int NF_, int BLOCKS_>
struct Geom {
  static constexpr int MF = MF_, NF = NF_, BLOCKS_PER_CU = BLOCKS_;
  static constexpr int BM = WAVES * MF * 16, BN = NF * 16;
  static constexpr int B_PIECES = NF * 3;                 // large 24, small 12
  static constexpr int WAVE_PIECES = B_PIECES / WAVES;    // pieces one wave stages per K step: 6, 3
  static constexpr int STAGE_BYTES = B_PIECES * PIECE;    // 24 KiB, 12 KiB
  static constexpr int LDS_BYTES = 2 * STAGE_BYTES;       // 48 KiB, 24 KiB
  static_assert(B_PIECES % WAVES == 0, "every wave stages the same number of pieces");
  static_assert(BLOCKS_PER_CU * LDS_BYTES <= 160 * 1024, "the CU has 160 KiB of LDS");
};
using Large = Geom<2, 8, 3>;  // 128 x 128: 144 of the CU's 160 KiB of LDS
using Small = Geom<1, 4, 6>;  //  64 x  64: 144 KiB as well
constexpr int BN_MAX = Large::BN;  // what shape_supported asks of n (a multiple of every form's BN)

// round-to-nearest-even split of two fp32 values into packed bf16 pairs hi / mid / lo (hi + mid + lo == x)
__device__ __forceinline__ void split2(f32x2 x, uint32_t &h, uint32_t &m, uint32_t &l) {
  h = __builtin_bit_cast(uint32_t, __builtin_convertvector(x, bf16x2));
  const f32x2 hf = {__builtin_bit_cast(float, h << 16), __builtin_bit_cast(float, h & 0xffff0000u)};
  const f32x2 r1 = x - hf;
  m = __builtin_bit_cast(uint32_t, __builtin_convertvector(r1, bf16x2));
  const f32x2 mf = {__builtin_bit_cast(float, m << 16), __builtin_bit_cast(float, m & 0xffff0000u)};
  const f32x2 r2 = r1 - mf;
  l = __builtin_bit_cast(uint32_t, __builtin_convertvector(r2, bf16x2));
}

__device__ __forceinline__ void split8(f32x4 x0, f32x4 x1, bf16x8 &h, bf16x8 &m, bf16x8 &l) {
  uint32_t h0, h1, h2, h3, m0, m1, m2, m3, l0, l1, l2, l3;
  split2(f32x2{x0[0], x0[1]}, h0, m0, l0);
  split2(f32x2{x0[2], x0[3]}, h1, m1, l1);
  split2(f32x2{x1[0], x1[1]}, h2, m2, l2);
  split2(f32x2{x1[2], x1[3]}, h3, m3, l3);
  const u32x4 H = {h0, h1, h2, h3}, M = {m0, m1, m2, m3}, L = {l0, l1, l2, l3};
  h = __builtin_bit_cast(bf16x8, H);
  m = __builtin_bit_cast(bf16x8, M);
  l = __builtin_bit_cast(bf16x8, L);
}

__device__ __forceinline__ float gelu_tanh(float x) {
  const float kBeta = 0.7978845608028654f;  // sqrt(2 / pi)
  const float kKappa = 0.044715f;
  const float inner = kBeta * (x + kKappa * x * x * x);
  return 0.5f * x * (1.0f + tanhf(inner));
}

// One thread per (16-column block, 32-row K block, lane): reads lane l's eight values of W, writes their three planes.
__global__ __launch_bounds__(256) void split_weights_kernel(const float *__restrict__ w, int64_t k, int64_t n, int64_t ldw,
                                                            u32x4 *__restrict__ out) {
  const int64_t kb_count = k / BK;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (n / 16) * kb_count * 64) return;
  const int l = (int)(t & 63);
  const int64_t blk = t >> 6, kb = blk % kb_count, nb = blk / kb_count;
  const int64_t col = nb * 16 + (l & 15), row = kb * BK + 8 * (l >> 4);
  f32x4 x0, x1;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    x0[j] = w[(row + j) * ldw + col];
    x1[j] = w[(row + 4 + j) * ldw + col];
  }
  bf16x8 h, m, lo;
  split8(x0, x1, h, m, lo);
  u32x4 *dst = out + blk * 3 * 64 + l;
  dst[0] = __builtin_bit_cast(u32x4, h);
  dst[64] = __builtin_bit_cast(u32x4, m);
  dst[128] = __builtin_bit_cast(u32x4, lo);
}

// 16-byte LDS-DMA of lane l's source to byte 16 * l of the piece at `lds` (wave-uniform)
__device__ __forceinline__ void glds16(const void *src, char *lds) {
  __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void *)lds, 16, 0, 0);
}

// what follows acc + bias in the epilogue
enum Epi { EPI_NONE, EPI_GELU, EPI_RESIDUAL };

// The residual operand of the EPI_RESIDUAL instantiations: R fp32 [m, n] of row pitch ld.  The other instantiations take an
// empty last argument, so their argument block and their code are what they were without it.
template <bool ON>
struct Residual {
  const float *p;
  int64_t ld;
};
template <>
struct Residual<false> {};

// EPI_RESIDUAL: C[row, col] = (acc + bias[col]) + R[row, col], two separately rounded adds.  R may be C itself (same pointer,
// same pitch: every element is read and written by one thread, the read first), so that instantiation's C is not __restrict__.
template <class G, Epi EPI>
__global__ __launch_bounds__(THREADS, G::BLOCKS_PER_CU) void gemm_split_kernel(
    const float *__restrict__ a, int64_t lda, const char *__restrict__ wsplit, const float *__restrict__ bias,
    typename std::conditional<EPI == EPI_RESIDUAL, float *, float *__restrict__>::type c, int64_t ldc, int m, int n, int k,
    Residual<EPI == EPI_RESIDUAL> res) {
  constexpr int MF = G::MF, NF = G::NF, BM = G::BM, BN = G::BN, WAVE_PIECES = G::WAVE_PIECES, STAGE_BYTES = G::STAGE_BYTES;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ntn = n / BN, ntm = (m + BM - 1) / BM;
  // bijective XCD remap: blocks that share blockIdx.x % 8 run on one XCD; give each such group a contiguous run of tiles
  const int nwg = ntm * ntn, orig = blockIdx.x, xcd = orig & 7, q = nwg >> 3, r = nwg & 7;
  const int wgid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
  const int tm = wgid / ntn, tn = wgid % ntn;
  const int m0 = tm * BM, n0 = tn * BN;
  const int kt_count = k / BK;

  // sources (per lane, advanced by one K step each iteration)
  // A operand of this lane for the wave's row fragments mf = MF * wave + i: eight floats of one row
  const float *a_src[MF];
#pragma unroll
  for (int i = 0; i < MF; ++i) {
    int row = m0 + (MF * wave + i) * 16 + (lane & 15);
    row = row < m ? row : m - 1;  // rows past M read the last row; their results are never stored
    a_src[i] = a + (int64_t)row * lda + 8 * (lane >> 4);
  }
  // B pieces of this wave: p = WAVE_PIECES * wave + i -> (nf = p / 3, plane = p % 3); LDS image: plane-major (plane * NF + nf)
  const char *b_src[WAVE_PIECES];
  int b_dst[WAVE_PIECES];
#pragma unroll
  for (int i = 0; i < WAVE_PIECES; ++i) {
    const int p = WAVE_PIECES * wave + i, nf = p / 3, pl = p % 3;
    const int64_t nb = n0 / 16 + nf;
    b_src[i] = wsplit + ((nb * kt_count) * 3 + pl) * PIECE + lane * 16;
    b_dst[i] = (pl * NF + nf) * PIECE;
  }
  const int64_t b_step = 3 * PIECE;  // one K step further in the packed image

  f32x4 ax[MF][2];  // this lane's A operand of the next K step (prefetched: the loop's closing wait retires it)
  auto load_a = [&](int kt) {
#pragma unroll
    for (int i = 0; i < MF; ++i) {
      ax[i][0] = *(const f32x4 *)(a_src[i] + kt * BK);
      ax[i][1] = *(const f32x4 *)(a_src[i] + kt * BK + 4);
    }
  };
  auto stage_b = [&](int buf, int kt) {
    char *base = lds + buf * STAGE_BYTES;
#pragma unroll
    for (int i = 0; i < WAVE_PIECES; ++i) glds16(b_src[i] + kt * b_step, base + b_dst[i]);
  };

  f32x4 acc[MF][NF];
#pragma unroll
  for (int i = 0; i < MF; ++i)
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  float bcol[NF];  // (loaded ahead: the loop's waits retire it)
#pragma unroll
  for (int nf = 0; nf < NF; ++nf) bcol[nf] = bias ? bias[n0 + nf * 16 + (lane & 15)] : 0.0f;

  load_a(0);
  stage_b(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int kt = 0; kt < kt_count; ++kt) {
    const int cur = kt & 1;
    const char *base = lds + cur * STAGE_BYTES;
    bf16x8 ah[MF], am[MF], al[MF];
#pragma unroll
    for (int i = 0; i < MF; ++i) split8(ax[i][0], ax[i][1], ah[i], am[i], al[i]);
    // (after the split: the prefetch registers are free, and nothing beyond column K of a row is ever addressed)
    if (kt + 1 < kt_count) {
      load_a(kt + 1);
      stage_b(cur ^ 1, kt + 1);
    }
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
      const bf16x8 bh = *(const bf16x8 *)(base + (0 * NF + nf) * PIECE + lane * 16);
      const bf16x8 bm = *(const bf16x8 *)(base + (1 * NF + nf) * PIECE + lane * 16);
      const bf16x8 bl = *(const bf16x8 *)(base + (2 * NF + nf) * PIECE + lane * 16);
#pragma unroll
      for (int i = 0; i < MF; ++i) {
        f32x4 t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am[i], bm, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], bh, t, 0, 0, 0);
        t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bl, t, 0, 0, 0);
        t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am[i], bh, t, 0, 0, 0);
        t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bm, t, 0, 0, 0);
        t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bh, t, 0, 0, 0);
        acc[i][nf] += t;  // (round-to-nearest add of this K step's partial: see the header)
      }
    }
    // the next stage and this lane's next A operand have landed, and every wave is done reading this stage (it is restaged
    // next iteration)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // the residual's elements of this lane, all loaded before the first store (C may be R: loads issued one by one between
  // the stores would each wait out a trip to memory), under the store's own guard
  float rv[EPI == EPI_RESIDUAL ? MF : 1][EPI == EPI_RESIDUAL ? NF : 1][4];
  if constexpr (EPI == EPI_RESIDUAL) {
#pragma unroll
    for (int nf = 0; nf < NF; ++nf)
#pragma unroll
      for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int row = m0 + wave * (MF * 16) + i * 16 + 4 * (lane >> 4) + j;
          rv[i][nf][j] = row < m ? res.p[(int64_t)row * res.ld + n0 + nf * 16 + (lane & 15)] : 0.0f;
        }
  }

  // epilogue: C/D map of 16x16 MFMA - col = lane & 15, row = 4 * (lane >> 4) + reg
#pragma unroll
  for (int nf = 0; nf < NF; ++nf) {
    const int col = n0 + nf * 16 + (lane & 15);
    const float b = bcol[nf];
#pragma unroll
    for (int i = 0; i < MF; ++i) {
      const int row0 = m0 + wave * (MF * 16) + i * 16 + 4 * (lane >> 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = row0 + j;
        if (row < m) {
          float v = acc[i][nf][j] + b;
          if (EPI == EPI_GELU) v = gelu_tanh(v);
          if (EPI == EPI_RESIDUAL) v += rv[i][nf][j];
          c[(int64_t)row * ldc + col] = v;
        }
      }
    }
  }
}

bool shape_supported(int64_t k, int64_t n) { return k > 0 && n > 0 && n % BN_MAX == 0 && k % 64 == 0 && k <= (1 << 20) && n <= (1 << 20); }

// one instantiation's host side: its LDS attribute (one bit per device), its launch and its residency
template <class G, Epi EPI>
struct Form {
  static inline std::atomic<uint64_t> lds_done{0};
  static const void *kernel() { return (const void *)gemm_split_kernel<G, EPI>; }
  static int launch(const glb_gemm_args &g, hipStream_t stream, Residual<EPI == EPI_RESIDUAL> res = {}) {
    const int64_t tiles = ((g.m + G::BM - 1) / G::BM) * (g.n / G::BN);
    if (tiles > INT32_MAX / 2 || g.m > INT32_MAX / 2) return glb::api_fail(GLB_EUNSUPPORTED, "too many rows");
    hipError_t e = glb::allow_dynamic_lds(kernel(), G::LDS_BYTES, lds_done);
    if (e != hipSuccess) return glb::api_hip_fail(e, "split GEMM LDS attribute");
    hipLaunchKernelGGL((gemm_split_kernel<G, EPI>), dim3((unsigned)tiles), dim3(THREADS), G::LDS_BYTES, stream, g.a, g.lda,
                       (const char *)g.w_split, g.bias, g.c, g.ldc, (int)g.m, (int)g.n, (int)g.k, res);
    e = hipGetLastError();
    if (e != hipSuccess) return glb::api_hip_fail(e, "split GEMM launch");
    return GLB_OK;
  }
  static int blocks_per_cu(int *blocks) {
    hipError_t e = glb::allow_dynamic_lds(kernel(), G::LDS_BYTES, lds_done);
    if (e != hipSuccess) return glb::api_hip_fail(e, "split GEMM LDS attribute");
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, gemm_split_kernel<G, EPI>, THREADS, G::LDS_BYTES);
    if (e != hipSuccess) return glb::api_hip_fail(e, "split GEMM occupancy query");
    return GLB_OK;
  }
};

bool form_ok(int form) { return form == GLB_GEMM_FORM_LARGE || form == GLB_GEMM_FORM_SMALL; }

// the CU count of the current device (asked once per device)
hipError_t device_cus(int *n_cus) {
  static std::atomic<int> cached[64];
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const bool slot = dev >= 0 && dev < 64;
  if (slot && (*n_cus = cached[dev].load(std::memory_order_relaxed)) > 0) return hipSuccess;
  e = hipDeviceGetAttribute(n_cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e == hipSuccess && slot) cached[dev].store(*n_cus, std::memory_order_relaxed);
  return e;
}

// The small form is picked while the launch's 128 x 128 tiles number fewer than 3/2 per CU.  One threshold serves the four
// projections (profiles/r28/split_gemm_forms_ab.txt, 256 CUs): below it the small form wins at every measured point, its
// slowest round faster than the large form's fastest (0.41-0.93 of its time); from it on the large form wins or the two lie
// within each other's spread.  For every (n, k) it is below the first row count from which the large form wins at every
// larger one.
constexpr int PICK_TILES_NUM = 3, PICK_TILES_DEN = 2;

}  // namespace

extern "C" {

size_t glb_gemm_split_bytes(int64_t k, int64_t n) {
  return shape_supported(k, n) ? (size_t)k * (size_t)n * 3 * sizeof(uint16_t) : 0;
}

int glb_gemm_split_weights(const float *w, int64_t k, int64_t n, int64_t ldw, void *out, size_t out_bytes, void *stream) {
  if (!w || !out) return glb::api_fail(GLB_EINVAL, "null pointer");
  if (k <= 0 || n <= 0 || ldw < n) return glb::api_fail(GLB_EINVAL, "bad shape (k %lld, n %lld, ldw %lld)", (long long)k,
                                                          (long long)n, (long long)ldw);
  if (!shape_supported(k, n)) return glb::api_fail(GLB_EUNSUPPORTED, "split GEMM needs n %% 128 == 0 and k %% 64 == 0");
  if (out_bytes < glb_gemm_split_bytes(k, n) || ((uintptr_t)out) % 16)
    return glb::api_fail(GLB_ENOSPC, "split weight buffer too small or not 16-byte aligned");
  const int64_t threads = (n / 16) * (k / BK) * 64;
  hipLaunchKernelGGL(split_weights_kernel, dim3(blocks_for(threads, 256)), dim3(256), 0, (hipStream_t)stream, w, k, n, ldw,
                     (u32x4 *)out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return glb::api_hip_fail(e, "split_weights launch");
  return GLB_OK;
}


int glb_gemm_split_pick(int64_t m, int64_t n, int64_t k, int n_cus, int *form) {
  if (!form) return glb::api_fail(GLB_EINVAL, "null pointer");
  if (m <= 0 || n <= 0 || k <= 0 || n_cus <= 0)
    return glb::api_fail(GLB_EINVAL, "bad shape (m %lld, n %lld, k %lld, %d CUs)", (long long)m, (long long)n, (long long)k,
                         n_cus);
  // (monotone in m: the tile count never falls as m grows; k does not enter today's rule)
  if (m > INT32_MAX || n > INT32_MAX) return *form = GLB_GEMM_FORM_LARGE, GLB_OK;  // (the product below stays in 64 bits)
  const int64_t tiles = ((m + Large::BM - 1) / Large::BM) * ((n + Large::BN - 1) / Large::BN);
  *form = tiles * PICK_TILES_DEN < (int64_t)PICK_TILES_NUM * n_cus ? GLB_GEMM_FORM_SMALL : GLB_GEMM_FORM_LARGE;
  return GLB_OK;
}

// the argument checks every split GEMM entry point shares; picks the form where `form` is 0
static int split_check(const glb_gemm_args *args, int &form) {
  if (!args) return glb::api_fail(GLB_EINVAL, "null argument block");
  if (args->struct_size != sizeof(glb_gemm_args))
    return glb::api_fail(GLB_EINVAL, "glb_gemm_args.struct_size %u != %zu (ABI mismatch)", args->struct_size,
                         sizeof(glb_gemm_args));
  if (form != 0 && !form_ok(form)) return glb::api_fail(GLB_EINVAL, "bad form %d", form);
  const glb_gemm_args &g = *args;
  if (!g.a || !g.w_split || !g.c) return glb::api_fail(GLB_EINVAL, "null pointer");
  if (g.m <= 0 || g.n <= 0 || g.k <= 0 || g.lda < g.k || g.ldc < g.n)
    return glb::api_fail(GLB_EINVAL, "bad shape (m %lld, n %lld, k %lld, lda %lld, ldc %lld)", (long long)g.m,
                         (long long)g.n, (long long)g.k, (long long)g.lda, (long long)g.ldc);
  if (g.epilogue != GLB_GEMM_BIAS && g.epilogue != GLB_GEMM_BIAS_GELU_TANH)
    return glb::api_fail(GLB_EINVAL, "bad epilogue %d", g.epilogue);
  if (!shape_supported(g.k, g.n)) return glb::api_fail(GLB_EUNSUPPORTED, "split GEMM needs n %% 128 == 0 and k %% 64 == 0");
  if (((uintptr_t)g.a) % 16 || g.lda % 4 || ((uintptr_t)g.w_split) % 16)
    return glb::api_fail(GLB_EUNSUPPORTED, "split GEMM needs A and its row pitch 16-byte aligned");
  if (form == 0) {
    int n_cus = 0;
    const hipError_t e = device_cus(&n_cus);
    if (e != hipSuccess) return glb::api_hip_fail(e, "split GEMM CU count");
    const int rc = glb_gemm_split_pick(g.m, g.n, g.k, n_cus, &form);
    if (rc != GLB_OK) return rc;
  }
  return GLB_OK;
}

int glb_gemm_f32_split_form(const glb_gemm_args *args, int form, void *stream) {
  const int rc = split_check(args, form);
  if (rc != GLB_OK) return rc;
  const glb_gemm_args &g = *args;
  const bool gelu = g.epilogue == GLB_GEMM_BIAS_GELU_TANH;
  hipStream_t s = (hipStream_t)stream;
  if (form == GLB_GEMM_FORM_SMALL) return gelu ? Form<Small, EPI_GELU>::launch(g, s) : Form<Small, EPI_NONE>::launch(g, s);
  return gelu ? Form<Large, EPI_GELU>::launch(g, s) : Form<Large, EPI_NONE>::launch(g, s);
}

int glb_gemm_f32_split_residual(const glb_gemm_args *args, const float *residual, int64_t ldr, int form, void *stream) {
  const int rc = split_check(args, form);
  if (rc != GLB_OK) return rc;
  const glb_gemm_args &g = *args;
  if (g.epilogue != GLB_GEMM_BIAS) return glb::api_fail(GLB_EINVAL, "the residual epilogue takes GLB_GEMM_BIAS only (epilogue %d)", g.epilogue);
  if (!residual) return glb::api_fail(GLB_EINVAL, "null residual");
  if (ldr < g.n || ((uintptr_t)residual) % sizeof(float))
    return glb::api_fail(GLB_EINVAL, "residual misaligned or its pitch %lld below n %lld", (long long)ldr, (long long)g.n);
  // C may be the residual itself (same pointer, same pitch: an element is read and written by one thread); no other overlap
  if (!(residual == g.c && ldr == g.ldc)) {
    const uintptr_t c0 = (uintptr_t)g.c, c1 = c0 + ((uint64_t)(g.m - 1) * (uint64_t)g.ldc + (uint64_t)g.n) * sizeof(float);
    const uintptr_t r0 = (uintptr_t)residual, r1 = r0 + ((uint64_t)(g.m - 1) * (uint64_t)ldr + (uint64_t)g.n) * sizeof(float);
    if (r0 < c1 && c0 < r1) return glb::api_fail(GLB_EINVAL, "the residual overlaps C without being C");
  }
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return glb::api_hip_fail(e, "split GEMM device");
  hipPointerAttribute_t at;
  e = hipPointerGetAttributes(&at, residual);
  if (e != hipSuccess || at.type != hipMemoryTypeDevice || at.device != dev) {
    (void)hipGetLastError();  // (a pointer the runtime does not know leaves its error behind)
    return glb::api_fail(GLB_EINVAL, "the residual is not memory of the current device");
  }
  hipStream_t s = (hipStream_t)stream;
  const Residual<true> res{residual, ldr};
  if (form == GLB_GEMM_FORM_SMALL) return Form<Small, EPI_RESIDUAL>::launch(g, s, res);
  return Form<Large, EPI_RESIDUAL>::launch(g, s, res);
}

int glb_gemm_f32_split(const glb_gemm_args *args, void *stream) { return glb_gemm_f32_split_form(args, 0, stream); }

int glb_gemm_split_form_blocks_per_cu(int form, int gelu, int *blocks) {
  if (!blocks) return glb::api_fail(GLB_EINVAL, "null pointer");
  if (!form_ok(form)) return glb::api_fail(GLB_EINVAL, "bad form %d", form);
  if (form == GLB_GEMM_FORM_SMALL) return gelu ? Form<Small, EPI_GELU>::blocks_per_cu(blocks) : Form<Small, EPI_NONE>::blocks_per_cu(blocks);
  return gelu ? Form<Large, EPI_GELU>::blocks_per_cu(blocks) : Form<Large, EPI_NONE>::blocks_per_cu(blocks);
}

int glb_gemm_split_blocks_per_cu(int gelu, int *blocks) {
  return glb_gemm_split_form_blocks_per_cu(GLB_GEMM_FORM_LARGE, gelu, blocks);
}

}  // extern "C"
