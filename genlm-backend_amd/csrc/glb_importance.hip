// glb_importance.hip - the importance-weighted particle step (include/glb.h: glb_importance_step).
//
// Per particle, with target row p, proposal row q (null: the target's own row), y = fl32(q * scale) and mask row m:
//     qt(j) ∝ exp(y_j + m_j)      token ~ qt      dlogw = (p_tok - lse(p)) - (y_tok - lse(y + m))
// Two plain launches on the caller's stream; no wave waits inside a launch for anything another wave writes.
//   imp_stats_kernel   one wave per (unit, 4096-token chunk) - a unit is a logits row when the masks go by row (or there
//                      are none), else a particle.  The chunk of p and of q, and for each of p, y and y + m the chunk's
//                      binary scale and integer sum, as glb_rowlse.hpp reads and takes them.  Out: one 64-byte record
//                      {N_p, N_y, N_z, -, S_p, S_y, S_z}.
//   imp_finish_kernel  one wave per particle.  Folds its unit's records in double (chunk order, lane l the chunks
//                      [l B, l B + B)), log-sum-exps by a double logarithm, picks the chunk by R1 / 2^64 over the chunks' masses
//                      of y + m, reads that one chunk of q again - lane l the 64 CONSECUTIVE elements from 64 l, so that the
//                      walk is in index order - with its mask words or floats, sums the terms in double, picks the element
//                      by R2 / 2^64, reads p_tok and writes the outputs from lane 0 with vector stores.
// Every result is a function of the inputs alone: a record depends on one chunk of one row and one mask row, a particle's
// outputs on its unit's records, its chunk and its Philox block (counter = global particle index, offset; key = seed) - not
// on the grid, on what else the call holds, or on how the particles are cut into calls.
// Row and mask ids come from device memory and are range-checked: a particle with an id out of range is served as one whose
// mask allows nothing (token -1, dlogw -inf).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/glb.h"
#include "glb_chunk.hpp"
#include "glb_common.hpp"
#include "glb_rowlse.hpp"

namespace {
using namespace glb;

constexpr int kNoProposal = -1;  // DTQ of the kernels: the proposal is the target's own row
constexpr double kTwoM64 = 5.42101086242752217e-20;  // 2^-64

struct alignas(16) ImpRec {  // one (unit, chunk): the workspace holds [n_units][nch] of them
  float Np, Ny, Nz;          // binary scales of p, y, y + m (-inf: nothing finite)
  uint32_t pad0;
  uint64_t Sp, Sy, Sz;       // sum over the chunk of 2^(x log2 e - N - 1), times 2^40
  uint64_t pad1;
  uint64_t pad2[2];
};
static_assert(sizeof(ImpRec) == 64, "record layout");

struct ImpParams {
  const void *p, *q;
  int64_t ld_p, ld_q;
  int32_t V, nch;
  float scale;
  int32_t n_rows, n_particles, n_units, n_masks, by_row, mask_kind;
  const int32_t *row_of;    // [n_particles], null = identity
  const int32_t *unit_mask; // [n_units], null = (n_masks == 1 ? 0 : identity)
  const void *mask;
  int64_t mask_ld;
  uint64_t seed, offset;
  int64_t particle_base;
  int32_t *out_token;
  float *out_dlogw, *out_lse, *out_logZq;
  ImpRec *recs;
};

// the logits row and the mask row of unit u; false: an id out of range
__device__ __forceinline__ bool unit_rows(const ImpParams &a, int u, int &row, int &mid) {
  row = a.by_row ? u : (a.row_of ? a.row_of[u] : u);
  mid = 0;
  if (a.mask_kind != GLB_MASK_NONE) mid = a.unit_mask ? a.unit_mask[u] : (a.n_masks == 1 ? 0 : u);
  return row >= 0 && row < a.n_rows && mid >= 0 && (a.mask_kind == GLB_MASK_NONE || mid < a.n_masks);
}

template <int DTP, int DTQ>
__global__ __launch_bounds__(64) void imp_stats_kernel(const ImpParams a) {
  constexpr int DTY = DTQ == kNoProposal ? DTP : DTQ;  // the element type y is read in
  constexpr int EPVP = ElemTraits<DTP>::EPV;
  const int lane = threadIdx.x;
  const int u = (int)(blockIdx.x / (uint32_t)a.nch), c = (int)(blockIdx.x % (uint32_t)a.nch);
  const int e_base = c * kChunk, V = a.V;
  ImpRec *rec = a.recs + (int64_t)u * a.nch + c;
  int row, mid;
  float Np = kNegInf, Ny = kNegInf, Nz = kNegInf;
  uint64_t Sp = 0, Sy = 0, Sz = 0;
  if (unit_rows(a, u, row, mid)) {  // (wave-uniform)
    const char *prow = row_ptr<DTP>(a.p, row, a.ld_p);
    u32x4_t rawp[ElemTraits<DTP>::NVC];
    load_chunk_raw<DTP>(prow, e_base, V, lane, rawp);
    float y[64];
    // (both chunks' loads are under way before the first is used)
    if constexpr (DTQ != kNoProposal) chunk_scaled<DTQ>(row_ptr<DTQ>(a.q, row, a.ld_q), e_base, V, lane, a.scale, y);
    {
      float x[64];
#pragma unroll
      for (int i = 0; i < ElemTraits<DTP>::NVC; ++i) unpack_vec<DTP>(rawp[i], &x[i * EPVP]);
      Np = exp_n(wave_max(lane_max64(x)));
      if (Np != kNegInf) Sp = wave_fix_sum(lane_sum64<EPVP>(x, Np));
      if constexpr (DTQ == kNoProposal) {
#pragma unroll
        for (int j = 0; j < 64; ++j) y[j] = x[j] * a.scale;  // (times 1.0f: the same bits)
      }
    }
    switch (a.mask_kind) {  // (wave-uniform)
      case GLB_MASK_NONE: chunk_sums<DTY, GLB_MASK_NONE>(y, true, a.mask, mid, a.mask_ld, e_base, V, lane, Ny, Sy, Nz, Sz); break;
      case GLB_MASK_BITS: chunk_sums<DTY, GLB_MASK_BITS>(y, true, a.mask, mid, a.mask_ld, e_base, V, lane, Ny, Sy, Nz, Sz); break;
      default: chunk_sums<DTY, GLB_MASK_F32>(y, true, a.mask, mid, a.mask_ld, e_base, V, lane, Ny, Sy, Nz, Sz); break;
    }
  }
  if (lane == 0) {
    typedef uint32_t v4 __attribute__((ext_vector_type(4)));
    v4 *o = reinterpret_cast<v4 *>(rec);
    o[0] = v4{__float_as_uint(Np), __float_as_uint(Ny), __float_as_uint(Nz), 0u};
    o[1] = v4{(uint32_t)Sp, (uint32_t)(Sp >> 32), (uint32_t)Sy, (uint32_t)(Sy >> 32)};
    o[2] = v4{(uint32_t)Sz, (uint32_t)(Sz >> 32), 0u, 0u};
  }
}

// inclusive prefix sums of a double over the 64 lanes, lane order
__device__ __forceinline__ double wave_scan_f64(double v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

template <int DT>
__device__ __forceinline__ float load_elem(const char *rowp, int j) {
  if constexpr (DT == kDtF32) return *reinterpret_cast<const float *>(rowp + (int64_t)j * 4);
  const uint32_t h = *reinterpret_cast<const uint16_t *>(rowp + (int64_t)j * 2);
  if constexpr (DT == kDtBf16) return __uint_as_float(h << 16);
  return (float)__builtin_bit_cast(_Float16, (uint16_t)h);
}

template <int DTP, int DTQ>
__global__ __launch_bounds__(64) void imp_finish_kernel(const ImpParams a) {
  constexpr int DTY = DTQ == kNoProposal ? DTP : DTQ;
  constexpr int EPVY = ElemTraits<DTY>::EPV, NVY = ElemTraits<DTY>::NVC;
  const int lane = threadIdx.x, pidx = blockIdx.x, V = a.V, nch = a.nch;
  int u = pidx, row = -1, mid = 0;
  bool ok = true;
  if (a.by_row) {
    u = a.row_of ? a.row_of[pidx] : pidx;
    ok = u >= 0 && u < a.n_units;
  }
  ok = ok && unit_rows(a, u, row, mid);  // (wave-uniform)
  int32_t token = -1;
  float dlogw = kNegInf, lse_t = kNegInf, logZq = kNegInf;
  if (ok) {
    const ImpRec *recs = a.recs + (int64_t)u * nch;
    const int B = (nch + 63) >> 6, c0 = lane * B, c1 = min(c0 + B, nch);
    // the unit's scales: the largest scale of a chunk that holds anything
    float Mp = kNegInf, My = kNegInf, Mz = kNegInf;
    for (int c = c0; c < c1; ++c) {
      const ImpRec r = recs[c];
      Mp = fmaxf(Mp, r.Sp ? r.Np : kNegInf);
      My = fmaxf(My, r.Sy ? r.Ny : kNegInf);
      Mz = fmaxf(Mz, r.Sz ? r.Nz : kNegInf);
    }
    Mp = wave_max(Mp);
    My = wave_max(My);
    Mz = wave_max(Mz);
    double wp = 0.0, wy = 0.0, wz = 0.0;  // the lane's chunks, in chunk order
    for (int c = c0; c < c1; ++c) {
      const ImpRec r = recs[c];
      wp += rec_mass(r.Sp, r.Np, Mp);
      wy += rec_mass(r.Sy, r.Ny, My);
      wz += rec_mass(r.Sz, r.Nz, Mz);
    }
    const double Wp = __shfl(wave_scan_f64(wp, lane), 63), Wy = __shfl(wave_scan_f64(wy, lane), 63);
    const double cz = wave_scan_f64(wz, lane), Wz = __shfl(cz, 63);
    const double lse_p = lse_of(Wp, Mp), lse_y = lse_of(Wy, My), lse_z = lse_of(Wz, Mz);
    lse_t = (float)lse_p;
    if (Wz > 0.0) {
      logZq = (float)(lse_z - lse_y);
      const uint64_t gp = (uint64_t)(a.particle_base + pidx);
      const uint32_t ctr[4] = {(uint32_t)gp, (uint32_t)(gp >> 32), (uint32_t)a.offset, (uint32_t)(a.offset >> 32)};
      const uint32_t key[2] = {(uint32_t)a.seed, (uint32_t)(a.seed >> 32)};
      uint32_t rnd[4];
      philox4x32_10(ctr, key, rnd);
      const uint64_t R1 = ((uint64_t)rnd[1] << 32) | rnd[0], R2 = ((uint64_t)rnd[3] << 32) | rnd[2];
      // ---- the chunk: inverse CDF over the chunks' masses of y + m, chunk order ----
      const double t1 = (double)R1 * kTwoM64 * Wz;
      int pick = -1, last = -1;
      {
        double cum = cz - wz;
        for (int c = c0; c < c1; ++c) {
          const ImpRec r = recs[c];
          const double w = rec_mass(r.Sz, r.Nz, Mz);
          if (w > 0.0) {
            cum += w;
            last = c;
            if (pick < 0 && cum > t1) pick = c;
          }
        }
        if (pick < 0) pick = last;
      }
      uint64_t hit = __ballot(wz > 0.0 && cz > t1);
      int L = hit ? (int)__ffsll((unsigned long long)hit) - 1 : 63 - (int)__clzll((unsigned long long)__ballot(wz > 0.0));
      const int cstar = __shfl(pick, L);
      // ---- the element: the chunk again, lane l its elements [64 l, 64 l + 64) ----
      const int e_base = cstar * kChunk, e0 = e_base + lane * 64;
      const char *yrow = DTQ == kNoProposal ? row_ptr<DTP>(a.p, row, a.ld_p) : row_ptr<DTY>(a.q, row, a.ld_q);
      float y[64], z[64];
#pragma unroll
      for (int i = 0; i < NVY; ++i) unpack_scaled<DTY, true>(load_vec_guarded<DTY>(yrow, e0 + i * EPVY, V), a.scale, &y[i * EPVY]);
      if (a.mask_kind == GLB_MASK_BITS) {
        const uint32_t *mrow = reinterpret_cast<const uint32_t *>(a.mask) + (int64_t)mid * a.mask_ld;
        const int nw = (V + 31) >> 5, wi = e0 >> 5;
        const uint32_t m0 = wi < nw ? mrow[wi] : 0u, m1 = wi + 1 < nw ? mrow[wi + 1] : 0u;
#pragma unroll
        for (int j = 0; j < 64; ++j) z[j] = (((j < 32 ? m0 : m1) >> (j & 31)) & 1u) ? y[j] : kNegInf;
      } else if (a.mask_kind == GLB_MASK_F32) {
        const char *mrow = reinterpret_cast<const char *>(reinterpret_cast<const float *>(a.mask) + (int64_t)mid * a.mask_ld);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          float m[4];
          unpack_vec<kDtF32>(load_vec_guarded<kDtF32>(mrow, e0 + 4 * i, V), m);
#pragma unroll
          for (int k = 0; k < 4; ++k) z[4 * i + k] = y[4 * i + k] + m[k];
        }
      } else {
#pragma unroll
        for (int j = 0; j < 64; ++j) z[j] = y[j];
      }
      const float bias = term_bias<kExpHw>(exp_n(wave_max(lane_max64(z))));
      double ls = 0.0;
#pragma unroll
      for (int j = 0; j < 64; ++j) {
        z[j] = chunk_term<kExpHw>(z[j], bias);  // (from here z holds the terms)
        ls += (double)z[j];
      }
      const double ce = wave_scan_f64(ls, lane), T = __shfl(ce, 63);
      const double t2 = (double)R2 * kTwoM64 * T;
      int jp = -1, jl = -1;
      float yp = 0.0f, yl = 0.0f;
      {
        double cum = ce - ls;
#pragma unroll
        for (int j = 0; j < 64; ++j) {
          const bool pos = z[j] > 0.0f;
          cum += (double)z[j];
          const bool take = pos && jp < 0 && cum > t2;
          jp = take ? j : jp;
          yp = take ? y[j] : yp;
          jl = pos ? j : jl;
          yl = pos ? y[j] : yl;
        }
        if (jp < 0) {
          jp = jl;
          yp = yl;
        }
      }
      hit = __ballot(ls > 0.0 && ce > t2);
      const uint64_t any = __ballot(ls > 0.0);
      if (any) {  // (always: the chunk's record said so)
        L = hit ? (int)__ffsll((unsigned long long)hit) - 1 : 63 - (int)__clzll((unsigned long long)any);
        token = e_base + L * 64 + __shfl(jp, L);
        const float y_tok = __shfl(yp, L);
        const float p_tok = load_elem<DTP>(row_ptr<DTP>(a.p, row, a.ld_p), token);
        dlogw = p_tok == kNegInf ? kNegInf : (float)(((double)p_tok - lse_p) - ((double)y_tok - lse_z));
      }
    }
  }
  if (lane == 0) {
    if (a.out_token) a.out_token[pidx] = token;
    if (a.out_dlogw) a.out_dlogw[pidx] = dlogw;
    if (a.out_lse) a.out_lse[pidx] = lse_t;
    if (a.out_logZq) a.out_logZq[pidx] = logZq;
  }
}

template <int DTP, int DTQ>
void launch_pair(const ImpParams &a, hipStream_t s) {
  hipLaunchKernelGGL((imp_stats_kernel<DTP, DTQ>), dim3((unsigned)((int64_t)a.n_units * a.nch)), dim3(64), 0, s, a);
  hipLaunchKernelGGL((imp_finish_kernel<DTP, DTQ>), dim3((unsigned)a.n_particles), dim3(64), 0, s, a);
}

template <int DTP>
void launch_q(int dtq, const ImpParams &a, hipStream_t s) {
  switch (dtq) {
    case kNoProposal: return launch_pair<DTP, kNoProposal>(a, s);
    case GLB_F32: return launch_pair<DTP, kDtF32>(a, s);
    case GLB_BF16: return launch_pair<DTP, kDtBf16>(a, s);
    default: return launch_pair<DTP, kDtF16>(a, s);
  }
}

int64_t n_chunks(int64_t vocab) { return (vocab + kChunk - 1) / kChunk; }

}  // namespace

extern "C" {

size_t glb_importance_workspace_bytes(int64_t n_particles, int64_t n_rows, int64_t vocab) {
  if (n_particles <= 0 || n_rows <= 0 || vocab <= 0) return 0;
  const int64_t units = n_particles > n_rows ? n_particles : n_rows;
  return (size_t)units * (size_t)n_chunks(vocab) * sizeof(ImpRec);
}

int glb_importance_step(const glb_importance_args *a, void *stream) {
  const char *const what = "glb_importance_step";
  if (const int rc = glb::block_ok(a, what, "glb_importance_args")) return rc;
  if (!a->target) return api_fail(GLB_EINVAL, "%s: target is null", what);
  if (a->target_dtype < GLB_F32 || a->target_dtype > GLB_F16)
    return api_fail(GLB_EINVAL, "%s: bad target_dtype %d", what, a->target_dtype);
  if (a->proposal && (a->proposal_dtype < GLB_F32 || a->proposal_dtype > GLB_F16))
    return api_fail(GLB_EINVAL, "%s: bad proposal_dtype %d", what, a->proposal_dtype);
  if (a->n_rows <= 0 || a->vocab <= 0 || a->n_particles <= 0)
    return api_fail(GLB_EINVAL, "%s: n_rows=%lld vocab=%lld n_particles=%lld must be positive", what, (long long)a->n_rows,
                    (long long)a->vocab, (long long)a->n_particles);
  if (a->vocab > 0x7fffff00ll || a->n_particles > 0x7fffffffll || a->n_rows > 0x7fffffffll)
    return api_fail(GLB_EINVAL, "%s: vocab / n_particles / n_rows exceed 31 bits", what);
  if (a->ld_p < a->vocab) return api_fail(GLB_EINVAL, "%s: ld_p %lld < vocab %lld", what, (long long)a->ld_p, (long long)a->vocab);
  if (a->proposal && a->ld_q < a->vocab)
    return api_fail(GLB_EINVAL, "%s: ld_q %lld < vocab %lld", what, (long long)a->ld_q, (long long)a->vocab);
  if (((uintptr_t)a->target) % (a->target_dtype == GLB_F32 ? 4 : 2) ||
      (a->proposal && ((uintptr_t)a->proposal) % (a->proposal_dtype == GLB_F32 ? 4 : 2)))
    return api_fail(GLB_EINVAL, "%s: logits pointer not element aligned", what);
  if (!(a->proposal_scale == a->proposal_scale)) return api_fail(GLB_EINVAL, "%s: proposal_scale is NaN", what);
  if (!a->row_of && a->n_particles != a->n_rows)
    return api_fail(GLB_EINVAL, "%s: row_of is null but n_particles != n_rows", what);
  if (a->mask_kind == GLB_MASK_PREPARED)
    return api_fail(GLB_EINVAL, "%s: GLB_MASK_PREPARED is the fused step's layout; give the bit rows (GLB_MASK_BITS)", what);
  if (a->mask_kind < GLB_MASK_NONE || a->mask_kind > GLB_MASK_F32)
    return api_fail(GLB_EINVAL, "%s: bad mask_kind %d", what, a->mask_kind);
  const bool by_row = a->mask_kind == GLB_MASK_NONE || a->row_mask_id != nullptr;
  const int64_t n_units = by_row ? a->n_rows : a->n_particles;
  if (a->mask_kind != GLB_MASK_NONE) {
    if (!a->mask || a->n_masks <= 0) return api_fail(GLB_EINVAL, "%s: mask table missing", what);
    const int64_t need = a->mask_kind == GLB_MASK_BITS ? (a->vocab + 31) / 32 : a->vocab;
    if (a->mask_ld < need) return api_fail(GLB_EINVAL, "%s: mask_ld %lld < %lld", what, (long long)a->mask_ld, (long long)need);
    if (a->row_mask_id && a->mask_id)
      return api_fail(GLB_EINVAL, "%s: give mask_id (per particle) or row_mask_id (per row), not both", what);
    if (!a->row_mask_id && !a->mask_id && a->n_masks != 1 && a->n_masks != n_units)
      return api_fail(GLB_EINVAL, "%s: no mask ids given but n_masks is neither 1 nor the number of %s", what,
                      by_row ? "rows" : "particles");
    if (((uintptr_t)a->mask) % 4) return api_fail(GLB_EINVAL, "%s: mask pointer misaligned", what);
    if (a->n_masks > 0x7fffffffll) return api_fail(GLB_EINVAL, "%s: n_masks exceeds 31 bits", what);
  }
  const int64_t nch = n_chunks(a->vocab);
  // (a grid holds fewer than 2^32 threads, 64 a wave)
  if (n_units * nch > 0x3ffffffll || a->n_particles > 0x3ffffffll)
    return api_fail(GLB_EUNSUPPORTED, "%s: %lld (unit, chunk) items / %lld particles exceed one grid of 2^26 waves", what,
                    (long long)(n_units * nch), (long long)a->n_particles);
  if (!a->workspace) return api_fail(GLB_EINVAL, "%s: workspace is null (glb_importance_workspace_bytes)", what);
  if (((uintptr_t)a->workspace) % 16) return api_fail(GLB_EINVAL, "%s: workspace not 16-byte aligned", what);
  const size_t need_ws = (size_t)n_units * (size_t)nch * sizeof(ImpRec);
  if (a->workspace_bytes < need_ws) return api_fail(GLB_ENOSPC, "%s: workspace %zu < %zu bytes", what, a->workspace_bytes, need_ws);

  ImpParams p{};
  p.p = a->target;
  p.q = a->proposal;
  p.ld_p = a->ld_p;
  p.ld_q = a->ld_q;
  p.V = (int32_t)a->vocab;
  p.nch = (int32_t)nch;
  p.scale = a->proposal_scale;
  p.n_rows = (int32_t)a->n_rows;
  p.n_particles = (int32_t)a->n_particles;
  p.n_units = (int32_t)n_units;
  p.n_masks = (int32_t)a->n_masks;
  p.by_row = by_row ? 1 : 0;
  p.mask_kind = a->mask_kind;
  p.row_of = a->row_of;
  p.unit_mask = a->mask_kind == GLB_MASK_NONE ? nullptr : (by_row ? a->row_mask_id : a->mask_id);
  p.mask = a->mask;
  p.mask_ld = a->mask_ld;
  p.seed = a->seed;
  p.offset = a->offset;
  p.particle_base = a->particle_base;
  p.out_token = a->out_token;
  p.out_dlogw = a->out_dlogw;
  p.out_lse = a->out_lse_target;
  p.out_logZq = a->out_logZ_proposal;
  p.recs = reinterpret_cast<ImpRec *>(a->workspace);
  const int dtq = a->proposal ? a->proposal_dtype : kNoProposal;
  hipStream_t s = (hipStream_t)stream;
  switch (a->target_dtype) {
    case GLB_F32: launch_q<kDtF32>(dtq, p, s); break;
    case GLB_BF16: launch_q<kDtBf16>(dtq, p, s); break;
    default: launch_q<kDtF16>(dtq, p, s); break;
  }
  return glb::launched(what);
}

}  // extern "C"
