// glb_truncate.hip - the keep set of top-k, top-p (nucleus) and min-p truncation as one bit row per logits row (include/glb.h:
// glb_truncate_rows).
//
// Per logits row, with y = fl32(x * scale), m its mask row, key = fl32(y + m) (glb_rowlse.hpp's keys) and u = key_mono(key), the
// keys' order as unsigned order: the row's threshold is the largest of
//   tau_k   the top_k-th largest key             an exact radix select over u by integer counts
//   tau_p   the nucleus boundary inside key >= tau_k   the same select weighted by integer masses
//   tau_m   fl32(key_max + log_min_p)
// and the keep set {key > -inf, key >= tau} is written as raw GLB_MASK_BITS words.
// truncate_rows_kernel  one workgroup of four waves per row: wave w streams the row's 4096-token chunks w, w + 4, ...
//                       (glb_rowlse.hpp's reader), once per pass:
//                         1  the largest key and the number of finite keys
//                         2  a select, digit by digit (11, 11 and 10 bits of u, most significant first): every key whose higher
//                            digits equal the chosen prefix adds 1 and its mass to its digit's bin in LDS, wave 0 sums the bins
//                            from the top and picks the bin in which the target (a count or a mass) is reached.  tau_k first
//                            (three passes), which also yields Z_k, the mass of key >= tau_k; then tau_p with the target
//                            ceil(top_p * Z_k) formed once in double - its first digit reuses the first pass's masses, so two
//                            more passes.  A select that is off (top_k = 0 or no more than top_k finite keys; top_p = 1) costs
//                            no pass.
//                         3  the emit pass: the lanes that share a word OR their bits together, one of them stores it; the kept
//                            count, and for out_logmass the kept and the total mass, are integer sums.
// The construction that makes a row's outputs independent of every order: a key's mass is round(2^(fl32(key - key_max) * log2 e)
// * 2^40) (v_exp_f32, at most 2^40 - 1) - a function of the key and the row's maximum alone - and every sum of counts and masses
// is an integer sum (LDS integer atomics, DPP integer sums), so neither which wave holds which chunk nor the order in which
// atomics land can change a bit.  A row's total stays below 2^64 for vocab <= 2^24.  The mass error against exact arithmetic is a
// few 1e-6 relative from the exponential and vocab * 2^-41 from the rounding, far inside the 1e-4 of the contract.
// Nothing waits on another workgroup; no workspace.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/glb.h"
#include "glb_chunk.hpp"
#include "glb_common.hpp"
#include "glb_rowlse.hpp"
#include "glb_topk.hpp"

namespace {
using namespace glb;

constexpr int kWaves = 4;
constexpr int kBins = 2048;                       // bins of the widest digit
constexpr int kLevels = 3;                        // digits of key_mono: bits 31..21, 20..10, 9..0
constexpr uint64_t kMassCap = (1ull << 40) - 1;   // a key's mass: at most this, so 2^24 of them stay below 2^64
constexpr int64_t kVocabMax = 1ll << 24;

__host__ __device__ constexpr int level_shift(int l) { return l == 0 ? 21 : (l == 1 ? 10 : 0); }
__host__ __device__ constexpr int level_bits(int l) { return l == 2 ? 10 : 11; }

struct TruncParams : RowsParams {
  int32_t top_k;  // 0 = off (the host caps it above any vocab)
  float top_p, log_min_p;
  uint32_t *out_bits;
  int64_t out_ld;
  float *out_threshold, *out_logmass;
  int32_t *out_kept;
};

struct Sel {  // what a scan of the bins found
  uint64_t mass_excl, mass_bin, mass_total;
  uint32_t bin, cnt_excl;
};

// round(exp(key - kmax) * 2^40), capped: a function of (key, kmax) alone
__device__ __forceinline__ uint64_t mass_fix(float key, float kmax) {
  const float e = __builtin_amdgcn_exp2f((key - kmax) * kLog2e);
  const uint64_t f = (uint64_t)__builtin_rint((double)e * kFixOne);
  return f < kMassCap ? f : kMassCap;
}

// Wave 0, all lanes: the bins summed from the top (bin nbins - 1 first) until `target` - a count, or with by_mass a mass - is
// reached; what lies strictly above the bin found, and the bin's own mass.  A target above the total is the total.
__device__ __forceinline__ void scan_select(const uint32_t *cnt, const uint64_t *mass, int nbins, bool by_mass, uint64_t target, int lane,
                                            Sel *out) {
  const int per = nbins >> 6;  // bins a lane: lane l holds bins nbins - 1 - l * per - i, i = 0 .. per - 1
  uint64_t c = 0, m = 0;
  for (int i = 0; i < per; ++i) {
    const int b = nbins - 1 - (lane * per + ((i + lane) & (per - 1)));  // (rotated by the lane: the lanes read different banks)
    c += cnt[b];
    m += mass[b];
  }
  const uint64_t ci = wave_scan_u64(c), mi = wave_scan_u64(m);
  const uint64_t vi = by_mass ? mi : ci;
  const uint64_t total = readlane_u64(vi, 63), mass_total = readlane_u64(mi, 63);
  target = target < total ? target : total;
  const int pick = __ffsll((long long)__ballot(vi >= target)) - 1;  // (lane 63 reaches the total)
  if (lane == pick) {
    uint64_t rc = ci - c, rm = mi - m;
    for (int i = 0; i < per; ++i) {
      const int b = nbins - 1 - (lane * per + i);
      const uint64_t cb = cnt[b], mb = mass[b];
      if ((by_mass ? rm + mb : rc + cb) >= target || i == per - 1) {
        out->bin = (uint32_t)b;
        out->cnt_excl = (uint32_t)rc;
        out->mass_excl = rm;
        out->mass_bin = mb;
        out->mass_total = mass_total;
        break;
      }
      rc += cb;
      rm += mb;
    }
  }
}

template <int DT, int MASK>
__global__ __launch_bounds__(64 * kWaves) void truncate_rows_kernel(const TruncParams a) {
  constexpr int EPV = ElemTraits<DT>::EPV, NVC = ElemTraits<DT>::NVC, LPW = 32 / EPV;  // LPW: lanes that share a word of bits
  __shared__ uint32_t h_cnt[kBins];
  __shared__ uint64_t h_mass[kBins];   // the masses of a pass's bins
  __shared__ uint64_t h_mass1[kBins];  // the first digit's, kept for the nucleus while tau_k takes its later digits
  __shared__ uint64_t s_red[kWaves][3];
  __shared__ Sel s_sel;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, V = a.V, nw = (V + 31) >> 5;
  for (int64_t row = blockIdx.x; row < a.n_rows; row += gridDim.x) {  // (the same trip count for the whole workgroup)
    int mid;
    const bool mask_ok = row_mask_of<MASK>(a, row, mid);
    const char *xrow = row_ptr<DT>(a.x, row, a.ld);
    uint32_t *orow = a.out_bits + row * a.out_ld;
    auto keys_of = [&](int e_base, float(&y)[64]) {
      chunk_scaled<DT>(xrow, e_base, V, lane, a.scale, y);
      chunk_add_mask<DT, MASK>(y, mask_ok, a.mask, mid, a.mask_ld, e_base, V, lane);
    };
    // three integer sums (v0: a maximum instead) over the workgroup, the same in every thread
    auto reduce3 = [&](bool v0_is_max, uint64_t &v0, uint64_t &v1, uint64_t &v2) {
      v0 = v0_is_max ? wave_max_u64(v0) : wave_sum_u64(v0);
      v1 = wave_sum_u64(v1);
      v2 = wave_sum_u64(v2);
      if (lane == 0) {
        s_red[wave][0] = v0;
        s_red[wave][1] = v1;
        s_red[wave][2] = v2;
      }
      __syncthreads();
      uint64_t r0 = 0, r1 = 0, r2 = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        r0 = v0_is_max ? (s_red[w][0] > r0 ? s_red[w][0] : r0) : r0 + s_red[w][0];
        r1 += s_red[w][1];
        r2 += s_red[w][2];
      }
      __syncthreads();  // (s_red is written again)
      v0 = r0;
      v1 = r1;
      v2 = r2;
    };

    // ---- pass 1: the largest key, the number of finite keys
    uint64_t top_mono = 0, n_finite = 0, unused = 0;
    for (int c = wave; c < a.nch; c += kWaves) {
      float y[64];
      keys_of(c * kChunk, y);
      uint32_t mx = 0, nf = 0;
#pragma unroll
      for (int j = 0; j < 64; ++j) {
        const bool fin = y[j] > kNegInf;
        const uint32_t u = key_mono(y[j]);
        mx = fin && u > mx ? u : mx;
        nf += fin ? 1u : 0u;
      }
      top_mono = mx > top_mono ? mx : top_mono;
      n_finite += nf;
    }
    reduce3(true, top_mono, n_finite, unused);
    if (n_finite == 0) {  // (workgroup-uniform) nothing to keep
      for (int w = threadIdx.x; w < nw; w += 64 * kWaves) orow[w] = 0u;
      if (threadIdx.x == 0) {
        if (a.out_threshold) a.out_threshold[row] = __builtin_huge_valf();
        if (a.out_kept) a.out_kept[row] = 0;
        if (a.out_logmass) a.out_logmass[row] = kNegInf;
      }
      continue;
    }
    const float kmax = mono_key((uint32_t)top_mono);
    const bool need_k = a.top_k > 0 && n_finite > (uint64_t)a.top_k, need_p = a.top_p < 1.0f;

    // one digit's histogram: every finite key whose digits above `level` equal `prefix`
    auto hist_pass = [&](int level, uint32_t prefix, bool want_cnt, bool want_mass, uint64_t *mass) {
      for (int i = threadIdx.x; i < kBins; i += 64 * kWaves) {
        h_cnt[i] = 0u;
        mass[i] = 0ull;
      }
      __syncthreads();
      const int sh = level_shift(level), psh = level == 0 ? 31 : level_shift(level - 1);
      const uint32_t bm = (1u << level_bits(level)) - 1u;
      for (int c = wave; c < a.nch; c += kWaves) {
        float y[64];
        keys_of(c * kChunk, y);
#pragma unroll
        for (int j = 0; j < 64; ++j) {
          const float v = y[j];
          const uint32_t u = key_mono(v);
          if (v > kNegInf && (level == 0 || (u >> psh) == prefix)) {
            const uint32_t b = (u >> sh) & bm;
            if (want_cnt) atomicAdd(&h_cnt[b], 1u);
            if (want_mass) {
              const uint64_t f = mass_fix(v, kmax);
              if (f) atomicAdd(reinterpret_cast<unsigned long long *>(&mass[b]), (unsigned long long)f);
            }
          }
        }
      }
      __syncthreads();
    };
    auto select = [&](const uint64_t *mass, int level, bool by_mass, uint64_t target) {
      if (wave == 0) scan_select(h_cnt, mass, 1 << level_bits(level), by_mass, target, lane, &s_sel);
      __syncthreads();
      const Sel s = s_sel;
      __syncthreads();  // (the next select may follow at once)
      return s;
    };

    // ---- tau_k, and Z_k: the mass of key >= tau_k
    uint32_t tk_mono = 0, tp_mono = 0;
    uint64_t Zk = 0;
    if (need_k) {
      uint64_t rem = (uint64_t)a.top_k, above = 0;
      for (int level = 0; level < kLevels; ++level) {
        uint64_t *mass = level == 0 ? h_mass1 : h_mass;
        hist_pass(level, tk_mono, true, need_p, mass);
        const Sel s = select(mass, level, false, rem);
        tk_mono = (tk_mono << level_bits(level)) | s.bin;
        rem -= s.cnt_excl;
        above += s.mass_excl;
        Zk = above + s.mass_bin;
      }
    }
    // ---- tau_p: the largest key t with mass(key >= t) >= top_p * Z_k
    if (need_p) {
      if (!need_k) {
        hist_pass(0, 0u, false, true, h_mass1);
        Zk = select(h_mass1, 0, true, ~0ull).mass_total;
      }
      const double t = __builtin_ceil((double)a.top_p * (double)Zk);
      uint64_t T = t >= (double)Zk ? Zk : (uint64_t)t;
      T = T < 1 ? 1 : T;
      for (int level = 0; level < kLevels; ++level) {
        const uint64_t *mass = level == 0 ? h_mass1 : h_mass;
        if (level > 0) hist_pass(level, tp_mono, false, true, h_mass);
        const Sel s = select(mass, level, true, T);
        tp_mono = (tp_mono << level_bits(level)) | s.bin;
        T -= s.mass_excl;
      }
    }
    const float tau_k = need_k ? mono_key(tk_mono) : kNegInf, tau_p = need_p ? mono_key(tp_mono) : kNegInf;
    const float tau = fmaxf(fmaxf(tau_k, tau_p), kmax + a.log_min_p);

    // ---- the emit pass
    const bool want_mass = a.out_logmass != nullptr;
    uint64_t kept = 0, m_kept = 0, m_all = 0;
    for (int c = wave; c < a.nch; c += kWaves) {
      const int e_base = c * kChunk;
      float y[64];
      keys_of(e_base, y);
#pragma unroll
      for (int i = 0; i < NVC; ++i) {
        uint32_t bits = 0;
#pragma unroll
        for (int q = 0; q < EPV; ++q) {
          const float v = y[i * EPV + q];
          const bool keep = v > kNegInf && v >= tau;
          bits |= (keep ? 1u : 0u) << q;
          if (want_mass && v > kNegInf) {
            const uint64_t f = mass_fix(v, kmax);
            m_all += f;
            m_kept += keep ? f : 0ull;
          }
        }
        kept += __popc(bits);
        uint32_t word = bits << ((lane & (LPW - 1)) * EPV);
#pragma unroll
        for (int d = 1; d < LPW; d <<= 1) word |= (uint32_t)__shfl_xor((int)word, d);
        const int wi = (e_base >> 5) + i * (64 * EPV / 32) + lane / LPW;
        if ((lane & (LPW - 1)) == 0 && wi < nw) orow[wi] = word;  // (bits beyond the row are 0: those keys read as -inf)
      }
    }
    reduce3(false, kept, m_kept, m_all);
    if (threadIdx.x == 0) {
      if (a.out_threshold) a.out_threshold[row] = tau;
      if (a.out_kept) a.out_kept[row] = (int32_t)kept;
      if (a.out_logmass) a.out_logmass[row] = (float)(log((double)m_kept) - log((double)m_all));
    }
  }
}

}  // namespace

extern "C" {

int glb_truncate_rows(const glb_truncate_args *a, void *stream) {
  const char *const what = "glb_truncate_rows";
  if (const int rc = glb::block_ok(a, what, "glb_truncate_args")) return rc;
  if (!a->logits) return api_fail(GLB_EINVAL, "%s: logits is null", what);
  if (!a->out_bits) return api_fail(GLB_EINVAL, "%s: out_bits is null", what);
  if (((uintptr_t)a->out_bits) % 4) return api_fail(GLB_EINVAL, "%s: out_bits pointer misaligned", what);
  if (a->top_k < 0) return api_fail(GLB_EINVAL, "%s: top_k %lld is negative", what, (long long)a->top_k);
  if (!(a->top_p > 0.0f) || a->top_p > 1.0f) return api_fail(GLB_EINVAL, "%s: top_p %g outside (0, 1]", what, (double)a->top_p);
  if (!(a->log_min_p <= 0.0f)) return api_fail(GLB_EINVAL, "%s: log_min_p %g must be at most 0", what, (double)a->log_min_p);
  if (a->vocab > kVocabMax) return api_fail(GLB_EINVAL, "%s: vocab %lld above 2^24 (a row's masses are summed in 64 bits)", what, (long long)a->vocab);
  if (a->n_rows > 0x7fffffffll) return api_fail(GLB_EINVAL, "%s: n_rows exceeds 31 bits", what);
  const RowsView v = rows_view(a);
  if (const int rc = rows_args_ok(what, v)) return rc;
  if (a->out_ld < (a->vocab + 31) / 32)
    return api_fail(GLB_EINVAL, "%s: out_ld %lld < %lld words", what, (long long)a->out_ld, (long long)((a->vocab + 31) / 32));

  const int32_t top_k = (int32_t)(a->top_k < 2 * kVocabMax ? a->top_k : 2 * kVocabMax);  // (at or above the vocabulary: off for every row)
  const TruncParams p{rows_params(v), top_k, a->top_p, a->log_min_p, a->out_bits, a->out_ld, a->out_threshold, a->out_logmass, a->out_kept};
  launch_rows(v, [&](auto dt, auto mk) {
    hipLaunchKernelGGL((truncate_rows_kernel<decltype(dt)::value, decltype(mk)::value>), rows_grid(p.n_rows), dim3(64 * kWaves), 0,
                       (hipStream_t)stream, p);
  });
  return glb::launched(what);
}

}  // extern "C"
