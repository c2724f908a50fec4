// glb_quant_tiled.hip - the many-row 4-bit GEMM (include/glb.h: glb_w4_gemm_tiled_forms, glb_w4_gemm_tiled).
//
// Y[m, n] = X[m, k] . W'^T (+ bias) on the image of glb_quant.hip, one launch, no workspace, no atomics, no second pass.
//
// Work split.  A workgroup of 4 waves owns a tile of 16 MF rows x 4 * 16 NF columns over the whole of K; wave w owns NF
// column groups of 16 (the image's row groups) for all rows of the tile: MF x NF accumulators of v_mfma_f32_16x16x32.
// Row tiles are the fastest-moving part of the block index: the workgroups that read the same codes run together and
// the codes stay in L2.
//
// Weights never touch LDS: lane (r = lane & 15, g = lane >> 4) loads the 8 bytes g of unit (kb, r) of its column group and
// the block's absmax, exactly as the few-row kernel does, and expands them into its B operands of the block's two MFMAs
// (k = 16 g .. 16 g + 15 of the block).  No two waves of a workgroup expand the same codes.
//
// X goes through LDS once per workgroup: the 256 threads load the tile's 16 MF x 64 elements of K block kb with 16-byte
// loads, 8 threads a row, and store them into one of two buffers; every wave reads its A operands from there with 16-byte
// LDS reads (row mf * 16 + r, elements 16 g + 8 s ..).  Rows lie at a pitch of 72 elements (144 bytes = 36 banks): the 16
// rows that one lane group reads at one k offset start 36 words apart - 4-bank groups 0, 36, 8, 44, ... that do not
// repeat within 16 rows on 64 banks, nor within 8 rows on 32 - where a pitch of 64 elements would put all 16 on one group.
// Rows past m are zeros in LDS (X is not read there) and their results are not stored.
//
// K loop: one barrier per K block.  The global loads of block kb + 1 (X chunk into registers, codes, absmax) are issued
// before the MFMAs of block kb, the LDS store into the other buffer comes after them, then the barrier: a buffer is written
// only after the barrier that ends the block that read it.
//
// Arithmetic: the few-row kernel's without a K split - one float32 accumulator per element of Y, started at +0, fed by the K
// blocks in ascending order and the two MFMAs of a block in order, then one float32 addition of the bias and one rounding
// (store_elem, as w4_reduce_kernel).  An element's bits depend on its row of X, its row of W' and its bias alone.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "../../include/glb.h"
#include "glb_common.hpp"
#include "glb_w4.hpp"

namespace {

constexpr int X_PITCH = QB + 8;  // elements between rows of X in LDS (see above)

struct TileForm {
  int mf, nf;
};
// form 1 .. 3 of glb_w4_tiled_args: tiles of 64 x 64, 128 x 64, 128 x 128
constexpr TileForm FORMS[] = {{4, 1}, {8, 1}, {8, 2}};
constexpr int N_FORMS = (int)(sizeof(FORMS) / sizeof(FORMS[0]));

template <int DT, int MF, int NF>
__global__ __launch_bounds__(256) void w4_gemm_tiled_kernel(const uint16_t *__restrict__ x, int64_t ldx,
                                                            const char *__restrict__ image, Codebook cb,
                                                            const uint16_t *__restrict__ bias, uint16_t *__restrict__ y,
                                                            int64_t ldy, int64_t m, int n, int k, int row_tiles) {
  constexpr int TM = 16 * MF;
  constexpr int XCH = TM * 8 / 256;  // 16-byte chunks of X a thread moves per K block
  static_assert(XCH * 256 == TM * 8, "whole chunks per thread");
  __shared__ float lut[16];
  __shared__ __attribute__((aligned(16))) uint16_t xs[2][TM * X_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  if (tid < 16) lut[tid] = cb.v[tid];
  const int kb_count = k / QB, nb_count = n / 16;
  const int64_t row0 = (int64_t)(blockIdx.x % (unsigned)row_tiles) * TM;
  const int nb0 = (int)(blockIdx.x / (unsigned)row_tiles) * (4 * NF) + wave * NF;

  // X staging: chunk id = i * 256 + tid -> row id / 8 of the tile, elements 8 (id % 8) .. of the K block
  const uint16_t *xg[XCH];
  bool x_in[XCH];
  int xs_at[XCH];
#pragma unroll
  for (int i = 0; i < XCH; ++i) {
    const int id = i * 256 + tid, row = id >> 3, c = id & 7;
    x_in[i] = row0 + row < m;
    xg[i] = x + (x_in[i] ? row0 + row : 0) * ldx + c * 8;
    xs_at[i] = row * X_PITCH + c * 8;
  }
  // the wave's column groups (ascending: a group past n / 16 has none after it that is inside)
  bool act[NF];
  const char *codes[NF];
  const float *amax[NF];
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    act[j] = nb0 + j < nb_count;
    const int64_t nb = act[j] ? nb0 + j : 0;
    codes[j] = image + nb * 16 * kb_count * UNIT + r * UNIT + g * 8;                                  // + kb * 16 * UNIT
    amax[j] = (const float *)(image + (int64_t)n * kb_count * UNIT) + nb * 16 * kb_count + r;  // + kb * 16
  }
  f32x4 acc[MF][NF];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf)
#pragma unroll
    for (int j = 0; j < NF; ++j) acc[mf][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 xr[XCH];
  u32x2 c[NF];
  float a[NF];
#pragma unroll
  for (int i = 0; i < XCH; ++i) xr[i] = x_in[i] ? *(const u32x4 *)xg[i] : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    c[j] = act[j] ? *(const u32x2 *)codes[j] : u32x2{0u, 0u};
    a[j] = act[j] ? amax[j][0] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < XCH; ++i) *(u32x4 *)(xs[0] + xs_at[i]) = xr[i];
  __syncthreads();

  for (int kb = 0; kb < kb_count; ++kb) {
    const bool has_next = kb + 1 < kb_count;  // (uniform)
    u32x2 cn[NF];
    float an[NF];
    if (has_next) {
#pragma unroll
      for (int i = 0; i < XCH; ++i) xr[i] = x_in[i] ? *(const u32x4 *)(xg[i] + (int64_t)(kb + 1) * QB) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        cn[j] = act[j] ? *(const u32x2 *)(codes[j] + (int64_t)(kb + 1) * 16 * UNIT) : u32x2{0u, 0u};
        an[j] = act[j] ? amax[j][(int64_t)(kb + 1) * 16] : 0.f;
      }
    }
    const uint16_t *buf = xs[kb & 1] + r * X_PITCH + g * 16;
    if (act[0]) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        u32x4 xa[MF];
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) xa[mf] = *(const u32x4 *)(buf + mf * 16 * X_PITCH + s * 8);
#pragma unroll
        for (int j = 0; j < NF; ++j) {
          if (j > 0 && !act[j]) continue;
          const u32x4 b = expand8<DT>(c[j][s], a[j], lut);
#pragma unroll
          for (int mf = 0; mf < MF; ++mf) acc[mf][j] = mfma16<DT>(xa[mf], b, acc[mf][j]);
        }
      }
    }
    if (has_next) {
#pragma unroll
      for (int i = 0; i < XCH; ++i) *(u32x4 *)(xs[(kb + 1) & 1] + xs_at[i]) = xr[i];
#pragma unroll
      for (int j = 0; j < NF; ++j) c[j] = cn[j], a[j] = an[j];
    }
    __syncthreads();
  }

  // C/D map of the 16x16 MFMA: col = lane & 15, row = 4 * (lane >> 4) + reg
#pragma unroll
  for (int j = 0; j < NF; ++j) {
    if (!act[j]) continue;
    const int col = (nb0 + j) * 16 + r;
    const float bv = bias ? load_elem(bias, col, DT) : 0.f;
#pragma unroll
    for (int mf = 0; mf < MF; ++mf)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t row = row0 + mf * 16 + 4 * g + i;
        if (row >= m) continue;
        float s = acc[mf][j][i];
        if (bias) s += bv;
        store_elem(y, row * ldy + col, DT, s);
      }
  }
}

int64_t tiles_of(const TileForm &f, int64_t m, int64_t n) { return ((m + 16 * f.mf - 1) / (16 * f.mf)) * ((n + 64 * f.nf - 1) / (64 * f.nf)); }

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

// form = 0: a speed choice only (every form gives the same bits), read from profiles/r34/w4_tiled_ab.txt.
// 128 x 128 where it was measured ahead: from 7/4 tiles per CU (it lost at 1, won at 7/4 and 2) and k >= 2048 (at k = 768
// the 64 x 64 form led even at 9/4); 128 x 64 from 2 tiles per CU: within 2 % of 64 x 64 on the Llama shapes, 6 % ahead on
// GPT-2's c_fc at 2048 rows and 7-9 % behind on c_attn at 2048 and 4096 rows; else 64 x 64.
int pick_form(int64_t m, int64_t n, int64_t k, int64_t cus) {
  if (k >= 2048 && 4 * tiles_of(FORMS[2], m, n) >= 7 * cus) return 3;
  if (tiles_of(FORMS[1], m, n) >= 2 * cus) return 2;
  return 1;
}

template <int DT, int MF, int NF>
void launch_form(const glb_w4_tiled_args &g, const Codebook &cb, hipStream_t stream) {
  const int64_t row_tiles = (g.m + 16 * MF - 1) / (16 * MF), col_tiles = (g.n + 64 * NF - 1) / (64 * NF);
  hipLaunchKernelGGL((w4_gemm_tiled_kernel<DT, MF, NF>), dim3((unsigned)(row_tiles * col_tiles)), dim3(256), 0, stream,
                     (const uint16_t *)g.x, g.ldx, (const char *)g.image, cb, (const uint16_t *)g.bias, (uint16_t *)g.y, g.ldy,
                     g.m, (int)g.n, (int)g.k, (int)row_tiles);
}

template <int DT>
void launch_tiled(int form, const glb_w4_tiled_args &g, const Codebook &cb, hipStream_t stream) {
  static_assert(N_FORMS == 3, "one case per form");
  switch (form) {
    case 1: launch_form<DT, 4, 1>(g, cb, stream); break;
    case 2: launch_form<DT, 8, 1>(g, cb, stream); break;
    default: launch_form<DT, 8, 2>(g, cb, stream); break;
  }
}

}  // namespace

extern "C" {

int glb_w4_gemm_tiled_forms(void) { return N_FORMS; }

int glb_w4_gemm_tiled(const glb_w4_tiled_args *args, void *stream) {
  const int rc = glb::block_ok(args, "glb_w4_gemm_tiled", "glb_w4_tiled_args");
  if (rc != GLB_OK) return rc;
  const glb_w4_tiled_args &g = *args;
  if (g.dtype != GLB_BF16 && g.dtype != GLB_F16)
    return glb::api_fail(GLB_EINVAL, "glb_w4_gemm_tiled: dtype %d is not 16-bit", g.dtype);
  if (g.form < 0 || g.form > N_FORMS) return glb::api_fail(GLB_EINVAL, "glb_w4_gemm_tiled: form %d not in 0 .. %d", g.form, N_FORMS);
  if (!g.x || !g.image || !g.y || !g.codebook) return glb::api_fail(GLB_EINVAL, "glb_w4_gemm_tiled: null pointer");
  if (g.m <= 0 || g.n <= 0 || g.k <= 0 || g.ldx < g.k || g.ldy < g.n)
    return glb::api_fail(GLB_EINVAL, "glb_w4_gemm_tiled: bad shape (m %lld, n %lld, k %lld, ldx %lld, ldy %lld)", (long long)g.m,
                         (long long)g.n, (long long)g.k, (long long)g.ldx, (long long)g.ldy);
  if (!codebook_ok(g.codebook)) return glb::api_fail(GLB_EINVAL, "glb_w4_gemm_tiled: codebook entry not finite");
  if ((uintptr_t)g.y % 2 || (uintptr_t)g.bias % 2) return glb::api_fail(GLB_EINVAL, "glb_w4_gemm_tiled: y / bias not aligned");
  if (!gemm_shape_served(g.n, g.k))
    return glb::api_fail(GLB_EUNSUPPORTED, "glb_w4_gemm_tiled needs n %% 16 == 0 and k %% 64 == 0");
  if ((uintptr_t)g.x % 16 || g.ldx % 8 || (uintptr_t)g.image % 16)
    return glb::api_fail(GLB_EUNSUPPORTED, "glb_w4_gemm_tiled needs X, its row pitch and the image 16-byte aligned");
  // (the smallest tile gives the most workgroups: one bound for every form)
  if (g.m > ((int64_t)1 << 40) || tiles_of(FORMS[0], g.m, g.n) > 0x7fffffffll)
    return glb::api_fail(GLB_EUNSUPPORTED, "glb_w4_gemm_tiled: more than 2^31 - 1 tiles");
  Codebook cb;
  for (int i = 0; i < 16; ++i) cb.v[i] = g.codebook[i];
  int form = g.form;
  if (form == 0) {
    int cus = 0;
    const hipError_t e = device_cus(&cus);
    if (e != hipSuccess) return glb::api_hip_fail(e, "w4 tiled GEMM device query");
    form = pick_form(g.m, g.n, g.k, cus);
  }
  if (g.dtype == GLB_BF16) launch_tiled<GLB_BF16>(form, g, cb, (hipStream_t)stream);
  else launch_tiled<GLB_F16>(form, g, cb, (hipStream_t)stream);
  return glb::launched("w4 tiled GEMM launch");
}

}  // extern "C"
