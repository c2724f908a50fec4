// glb_bytelm.hip - a byte-level beam over tokenisations (include/glb.h: glb_bytelm_children, glb_bytelm_extend,
// glb_bytelm_next).
//
// Candidates live in slots that never move: group g owns slots g * width .. g * width + width - 1 of node / u / w / alive.
//   bytelm_children_kernel  one wave per slot: the slot's node's out-edges (the trie's CSR with the edge symbols) scattered into
//                           a row of 260 node ids in LDS - columns 0..255 the byte children, 256..259 the leaf children - and
//                           written out in one piece.
//   bytelm_extend_kernel    one wave per group: the at most 64 existing weights (indices 0..63) and 64 * 4 offers (index
//                           64 + slot * 4 + leaf) are one chunk of glb_topk.hpp's selection core, so equal weights order by
//                           existing before spawned, lower slot, lower leaf.  Kept candidates stay where they are; the r-th
//                           best spawned survivor takes the r-th lowest slot no kept candidate holds.
//   bytelm_compact_kernel   one wave: the slots that hold a spawned candidate, ascending, and their number.
//   bytelm_next_kernel      one wave per group: column c of the next-byte row on lane c % 64; the group's largest u first,
//                           then every column's sum over the slots in slot order; with `byte`, the advance.
//   bytelm_step_kernel      one wave per group (glb_bytelm_step): next's row (the same device function), the row
//                           of a byte automaton at the group's state, the constrained mass, the byte - given, or the first
//                           column past a uniform by a scan per register and the registers' carried totals - and the advance.
// A group's outputs depend on that group's inputs alone; every fold has a fixed order.  Nothing waits on another workgroup.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/glb.h"
#include "glb_common.hpp"
#include "glb_math.hpp"
#include "glb_topk.hpp"

namespace {
using namespace glb;

constexpr int kSel = GLB_BYTELM_SEL;        // columns of a selection / mass row
constexpr int kRow = GLB_BYTELM_ROW;        // columns of a next-byte row: 256 bytes and EOS
constexpr int kLeaves = GLB_BYTELM_LEAVES;  // leaf children a node may have

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < __builtin_huge_valf(); }  // (false for NaN)
__device__ __forceinline__ float mass_or_zero(float m) { return m > 0.0f ? m : 0.0f; }           // (a NaN mass counts as none)

__global__ __launch_bounds__(64) void bytelm_children_kernel(const glb_bytelm_args a) {
  __shared__ int32_t row[kSel];
  const int lane = threadIdx.x;
  const int64_t n_slots = a.n_groups * a.width;
  for (int64_t s = blockIdx.x; s < n_slots; s += gridDim.x) {
    for (int c = lane; c < kSel; c += 64) row[c] = -1;
    __syncthreads();
    const int n = a.node[s];
    if (a.alive[s] != 0 && n >= 0 && n < a.n_nodes) {
      const int lo = a.child_ptr[n], hi = a.child_ptr[n + 1];
      for (int i = lo + lane; i < hi; i += 64) {
        const int sym = a.child_sym[i];
        if (sym >= 0 && sym < kSel) row[sym] = a.child_idx[i];  // (a symbol occurs once among a node's edges)
      }
    }
    __syncthreads();
    for (int c = lane; c < kSel; c += 64) a.sel[s * kSel + c] = row[c];
    __syncthreads();  // (the row is filled again for the workgroup's next slot)
  }
}

__global__ __launch_bounds__(64) void bytelm_extend_kernel(const glb_bytelm_args a) {
  __shared__ int32_t s_parent[64], s_token[64];
  __shared__ float s_u[64];
  const int lane = threadIdx.x, B = a.width;
  for (int64_t g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
    const int64_t b0 = g * B;
    const bool fresh = a.fresh == nullptr || a.fresh[g] != 0;  // (a group that has not moved since its last extension offers nothing)
    float z[64];
#pragma unroll
    for (int j = 0; j < 64; ++j) {  // candidate s = j * 64 + lane: 0..63 the existing slots, 64 + slot * 4 + leaf the offers
      float v = kNegInf;
      if (j == 0) {
        if (lane < B && a.alive[b0 + lane] != 0) {
          const float w = a.w[b0 + lane];
          if (finite_f(w) && finite_f(a.u[b0 + lane])) v = w;
        }
      } else if (j <= kLeaves) {
        const int o = (j - 1) * 64 + lane, b = o >> 2, l = o & 3;
        if (fresh && b < B && a.alive[b0 + b] != 0 && a.node[b0 + b] != a.root) {
          const int leaf = a.sel[(b0 + b) * kSel + 256 + l];
          const float m = a.mass[(b0 + b) * kSel + 256 + l], u = a.u[b0 + b];
          if (leaf >= 0 && leaf < a.n_nodes && m > 0.0f && finite_f(u) && a.leaf_token[leaf] >= 0) {
            const float t = u + logf(m);
            if (finite_f(t)) v = t;
          }
        }
      }
      z[j] = v;
    }
    uint64_t L = 0;
    select_chunk<1>(z, 0, lane, B, L);
    const bool has = lane < B && L != 0ull;
    const int idx = has ? entry_index(L) : -1;
    const bool is_old = has && idx < 64, is_new = has && idx >= 64;
    s_parent[lane] = -1;
    s_token[lane] = -1;
    s_u[lane] = kNegInf;
    __syncthreads();
    if (is_old) s_parent[idx] = idx;
    __syncthreads();
    const uint64_t all = B == 64 ? ~0ull : ((1ull << B) - 1ull);
    uint64_t free_slots = ~__ballot(s_parent[lane] >= 0) & all;
    const int rank = __popcll(__ballot(is_new) & ((1ull << lane) - 1ull));  // (the list is sorted: lane order is weight order)
    __syncthreads();  // (every lane has read the kept slots before a spawned candidate is written among them)
    if (is_new) {  // kept + spawned <= B, so there is a free slot for every rank
      for (int i = 0; i < rank; ++i) free_slots &= free_slots - 1ull;
      const int to = __builtin_ctzll(free_slots), o = idx - 64, b = o >> 2;
      s_parent[to] = b;
      s_token[to] = a.leaf_token[a.sel[(b0 + b) * kSel + 256 + (o & 3)]];
      s_u[to] = entry_key(L);
    }
    __syncthreads();
    if (lane < B) {
      const int p = s_parent[lane], t = s_token[lane];
      const int64_t s = b0 + lane;
      const bool kept = p >= 0 && t < 0, spawned = p >= 0 && t >= 0;
      a.out_parent[s] = p >= 0 ? (int32_t)(b0 + p) : -1;
      a.out_token[s] = spawned ? t : -1;
      a.out_alive[s] = p >= 0 ? 1 : 0;
      a.out_node[s] = kept ? a.node[s] : a.root;
      a.out_u[s] = kept ? a.u[s] : s_u[lane];
      a.out_w[s] = kept ? a.w[s] : s_u[lane];  // (a spawned candidate stands at the root, whose mass is 1: w = u)
    }
    if (lane == 0 && a.fresh != nullptr) a.fresh[g] = 0;
    __syncthreads();  // (the shared arrays are written again for the workgroup's next group)
  }
}

__global__ __launch_bounds__(64) void bytelm_compact_kernel(const glb_bytelm_args a) {
  const int lane = threadIdx.x;
  const int64_t n_slots = a.n_groups * a.width;
  int64_t base = 0;
  for (int64_t i0 = 0; i0 < n_slots; i0 += 64) {
    const int64_t i = i0 + lane;
    const bool f = i < n_slots && a.out_token[i] >= 0;
    const uint64_t m = __ballot(f);
    if (f) a.out_spawned[base + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)i;
    base += __popcll(m);
  }
  for (int64_t i = base + lane; i < n_slots; i += 64) a.out_spawned[i] = -1;
  if (lane == 0) a.out_n_spawned[0] = (int32_t)base;
}

__device__ __forceinline__ float wave_all_max(float v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v = fmaxf(v, __shfl_xor(v, d));
  return v;
}
__device__ __forceinline__ float wave_all_sum(float v) {  // (a + b == b + a bit for bit: every lane ends with the same sum)
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
  return v;
}

// The unconstrained next-byte row of the group whose first slot is b0 (glb_bytelm_next's contract): out[q] is column q * 64 + lane
// for q < 4, out[4] on lane 0 is EOS (-inf on the other lanes); uu the lane's own slot's u (-inf: no live candidate there);
// logZ as out_logZ.  Shared by bytelm_next_kernel and bytelm_step_kernel: one sequence of float32 operations.
__device__ __forceinline__ void bytelm_row(const glb_bytelm_args &a, int64_t b0, int lane, float &uu, float (&out)[5], float &logZ) {
  const int B = a.width;
  uu = kNegInf;
  int at_root = 0;  // (a lane reads its own slot's state only: the advance writes it)
  if (lane < B && a.alive[b0 + lane] != 0) {
    const float t = a.u[b0 + lane];
    if (finite_f(t)) uu = t;
    at_root = a.node[b0 + lane] == a.root ? 1 : 0;
  }
  const float top = wave_all_max(uu);
  float num[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // columns lane, 64 + lane, 128 + lane, 192 + lane; lane 0: EOS
  for (int s = 0; s < B; ++s) {                   // slot order
    const float us = __shfl(uu, s);
    if (!(us > kNegInf)) continue;  // (wave-uniform)
    const float e = expf(us - top);
    const float *mrow = a.mass + (b0 + s) * kSel;
#pragma unroll
    for (int q = 0; q < 4; ++q) num[q] += e * mass_or_zero(mrow[q * 64 + lane]);
    if (__shfl(at_root, s) != 0 && lane == 0) {  // a candidate between two tokens may end: the root's leaves are the EOS tokens
      float t = 0.0f;
#pragma unroll
      for (int l = 0; l < kLeaves; ++l) t += mass_or_zero(mrow[256 + l]);
      num[4] += e * t;
    }
  }
  const float total = wave_all_sum(((num[0] + num[1]) + (num[2] + num[3])) + num[4]);
  const bool any = top > kNegInf && total > 0.0f;
  const float log_total = any ? logf(total) : 0.0f;
#pragma unroll
  for (int q = 0; q < 5; ++q) out[q] = (any && num[q] > 0.0f) ? logf(num[q]) - log_total : kNegInf;
  logZ = any ? top + log_total : kNegInf;
}

// register q's entry for column c = q * 64 + lane (EOS: q = 4, lane 0), broadcast from the lane that holds it
__device__ __forceinline__ float row_entry(const float (&v)[5], int c) {
  const int q = c >> 6;
  const float mine = q == 0 ? v[0] : q == 1 ? v[1] : q == 2 ? v[2] : q == 3 ? v[3] : v[4];
  return __shfl(mine, c & 63);
}

// The advance of group g by `byte` (0 .. 256; wave-uniform): the unconstrained row's entry joins the group's logp, every
// candidate moves to its child or dies.  kill: every candidate dies whatever the byte (a byte < 0 then adds nothing to logp).
__device__ __forceinline__ void bytelm_advance(const glb_bytelm_args &a, int64_t g, int lane, float uu, const float (&out)[5], int byte,
                                               bool kill) {
  const int B = a.width;
  const int64_t b0 = g * B;
  const float step = byte >= 0 ? row_entry(out, byte) : 0.0f;
  if (lane < B) {
    const int64_t s = b0 + lane;
    if (a.alive[s] != 0) {
      int child = -1;
      float m = 0.0f;
      if (byte >= 0 && byte < 256 && !kill) {
        child = a.sel[s * kSel + byte];
        m = a.mass[s * kSel + byte];
      }
      if (child >= 0 && child < a.n_nodes && m > 0.0f && uu > kNegInf) {
        a.node[s] = child;
        a.w[s] = uu + logf(m);
      } else {
        a.alive[s] = 0;
        a.w[s] = kNegInf;
      }
    }
  }
  if (lane == 0) {
    if (byte >= 0) a.logp[g] += step;
    if (a.fresh != nullptr) a.fresh[g] = 1;
  }
}

__global__ __launch_bounds__(64) void bytelm_next_kernel(const glb_bytelm_args a) {
  const int lane = threadIdx.x;
  for (int64_t g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
    int byte = 0;
    if (a.byte != nullptr) {
      byte = a.byte[g];
      if (byte < 0 || byte >= kRow) continue;  // (wave-uniform) -1: the group is left alone
    }
    float uu, out[5], logZ;
    bytelm_row(a, g * a.width, lane, uu, out, logZ);
    if (a.byte == nullptr) {
#pragma unroll
      for (int q = 0; q < 4; ++q) a.out_next[g * kRow + q * 64 + lane] = out[q];
      if (lane == 0) {
        a.out_next[g * kRow + 256] = out[4];
        a.out_logZ[g] = logZ;
      }
      continue;
    }
    bytelm_advance(a, g, lane, uu, out, byte, false);
  }
}

// inclusive prefix sum over the lanes in a fixed order (lane 63: the wave's total)
__device__ __forceinline__ float wave_scan_f32(float v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float t = __shfl_up(v, d);
    if (lane >= d) v += t;
  }
  return v;
}

// One byte step under a byte automaton (include/glb.h glb_bytelm_step): the row, the automaton's row at the group's state, the
// constrained mass, the byte (given, from a given uniform, or from Philox) and the advance, one wave per group.
__global__ __launch_bounds__(64) void bytelm_step_kernel(const glb_bytelm_step_args p) {
  const glb_bytelm_args &a = p.beam;
  const int lane = threadIdx.x;
  const int64_t S = p.n_states;
  const bool given = a.byte != nullptr, peek = p.peek != 0;
  for (int64_t g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
    int byte = -1;
    if (p.ended[g] != 0 || (given && !peek && ((byte = a.byte[g]) < 0 || byte >= kRow))) {  // (wave-uniform) left alone
      if (p.out_row != nullptr) {  // the outputs say so: no next byte was looked at
#pragma unroll
        for (int q = 0; q < 4; ++q) p.out_row[g * kRow + q * 64 + lane] = kNegInf;
        if (lane == 0) p.out_row[g * kRow + 256] = kNegInf;
      }
      if (lane == 0) {
        p.out_logZc[g] = kNegInf;
        if (!given && !peek) p.out_byte[g] = -1;
      }
      continue;
    }
    float uu, out[5], logZ;
    bytelm_row(a, g * a.width, lane, uu, out, logZ);
    // ---- the automaton's row at s
    const int64_t s = p.state[g];
    const bool in = s >= 0 && s < S;
    int32_t to[4];
    float lc[5], aw[5];  // aw: the automaton's own weight of the column (0 without weights)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = q * 64 + lane;
      const int32_t t = in ? p.delta[s * 256 + c] : -1;
      const bool ok = t >= 0 && t < S && p.live[t] != 0;
      aw[q] = ok && p.arc_logw != nullptr ? p.arc_logw[s * 256 + c] : 0.0f;
      const float v = ok ? out[q] + aw[q] : kNegInf;
      to[q] = ok ? t : -1;
      lc[q] = finite_f(v) ? v : kNegInf;  // (a weight of -inf, NaN or +inf forbids)
    }
    lc[4] = kNegInf;
    aw[4] = 0.0f;
    if (lane == 0 && in && p.accepting[s] != 0) {
      if (p.final_logw != nullptr) aw[4] = p.final_logw[s];
      const float v = out[4] + aw[4];
      lc[4] = finite_f(v) ? v : kNegInf;
    }
    // ---- the constrained mass: the maximum first, then the sum in row's order
    const float m = wave_all_max(fmaxf(fmaxf(fmaxf(lc[0], lc[1]), fmaxf(lc[2], lc[3])), lc[4]));
    const bool some = m > kNegInf;
    float e[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) e[q] = (some && lc[q] > kNegInf) ? expf(lc[q] - m) : 0.0f;
    const float total = wave_all_sum(((e[0] + e[1]) + (e[2] + e[3])) + e[4]);  // (>= 1 where `some`: the maximum's term)
    const float logZc = some ? m + logf(total) : kNegInf;
    float row[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) row[q] = (some && lc[q] > kNegInf) ? lc[q] - logZc : kNegInf;
    if (p.out_row != nullptr) {
#pragma unroll
      for (int q = 0; q < 4; ++q) p.out_row[g * kRow + q * 64 + lane] = row[q];
      if (lane == 0) p.out_row[g * kRow + 256] = row[4];
    }
    if (lane == 0) p.out_logZc[g] = logZc;
    if (peek) continue;
    // ---- the byte
    bool dead = !some;
    if (!given && some) {
      float uni;
      if (p.uniform != nullptr) {
        uni = p.uniform[g];
      } else {
        const uint32_t ctr[4] = {(uint32_t)g, (uint32_t)((uint64_t)g >> 32), (uint32_t)p.offset, (uint32_t)(p.offset >> 32)};
        const uint32_t key[2] = {(uint32_t)p.seed, (uint32_t)(p.seed >> 32)};
        uint32_t rnd[4];
        philox4x32_10(ctr, key, rnd);
        uni = (float)(rnd[0] >> 8) * 0x1p-24f;
      }
      // the first column in the order 0 .. 256 whose cumulative probability exceeds uni: a scan per register, the registers'
      // totals carried; the last allowed column where rounding leaves none
      float base = 0.0f;
      int last = -1;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool allowed = row[q] > kNegInf;
        const float cum = base + wave_scan_f32(allowed ? expf(row[q]) : 0.0f, lane);
        const uint64_t open = __ballot(allowed);
        if (byte < 0) {
          const uint64_t hit = __ballot(allowed && cum > uni);
          if (hit != 0ull) byte = q * 64 + (int)__ffsll((unsigned long long)hit) - 1;
        }
        if (open != 0ull) last = q * 64 + 63 - (int)__clzll((unsigned long long)open);
        base = __shfl(cum, 63);
      }
      const float r4 = __shfl(row[4], 0);
      if (r4 > kNegInf) {
        if (byte < 0 && base + expf(r4) > uni) byte = 256;
        last = 256;
      }
      if (byte < 0) byte = last;
    }
    // a given byte: dead where it is forbidden or without mass, else its weight is the automaton's own
    if (given && some && !(row_entry(lc, byte) > kNegInf)) dead = true;
    const float mine = given && !dead ? row_entry(aw, byte) : 0.0f;
    const int32_t q_to = byte >= 0 && byte < 256 ? byte >> 6 : 0;
    const int32_t next = __shfl(q_to == 0 ? to[0] : q_to == 1 ? to[1] : q_to == 2 ? to[2] : to[3], byte >= 0 ? byte & 63 : 0);
    // ---- the advance
    bytelm_advance(a, g, lane, uu, out, byte, dead);
    if (lane == 0) {
      if (dead) {
        p.state[g] = -1;
        p.log_weight[g] = kNegInf;
        if (!given) byte = -1;
      } else {
        p.state[g] = byte < 256 ? next : -1;
        if (byte == 256) p.ended[g] = 1;
        p.log_weight[g] += given ? mine : logZc;
      }
      if (p.out_byte != nullptr) p.out_byte[g] = byte;
    }
  }
}

int common_checks(const glb_bytelm_args *a, const char *what) {
  if (const int rc = glb::block_ok(a, what, "glb_bytelm_args")) return rc;
  if (a->width < 1 || a->width > kTopkMax) return api_fail(GLB_EINVAL, "%s: width %d outside 1..%d", what, a->width, kTopkMax);
  if (a->n_groups <= 0 || a->n_nodes <= 0)
    return api_fail(GLB_EINVAL, "%s: n_groups=%lld n_nodes=%lld must be positive", what, (long long)a->n_groups, (long long)a->n_nodes);
  if (a->n_groups > 0x7fffffffll / a->width || a->n_nodes > 0x7fffffffll)
    return api_fail(GLB_EINVAL, "%s: n_groups * width or n_nodes exceed 31 bits", what);
  if (a->root < 0 || a->root >= a->n_nodes) return api_fail(GLB_EINVAL, "%s: root %d outside the trie", what, a->root);
  if (!a->node || !a->alive || !a->sel) return api_fail(GLB_EINVAL, "%s: null node, alive or sel", what);
  return GLB_OK;
}

unsigned grid_for(int64_t n) { return (unsigned)(n < (1 << 20) ? n : (1 << 20)); }

}  // namespace

extern "C" {

int glb_bytelm_children(const glb_bytelm_args *a, void *stream) {
  const char *const what = "glb_bytelm_children";
  if (const int rc = common_checks(a, what)) return rc;
  if (!a->child_ptr || !a->child_idx || !a->child_sym) return api_fail(GLB_EINVAL, "%s: null child_ptr, child_idx or child_sym", what);
  hipLaunchKernelGGL(bytelm_children_kernel, dim3(grid_for(a->n_groups * a->width)), dim3(64), 0, (hipStream_t)stream, *a);
  return glb::launched(what);
}

int glb_bytelm_extend(const glb_bytelm_args *a, void *stream) {
  const char *const what = "glb_bytelm_extend";
  if (const int rc = common_checks(a, what)) return rc;
  if (!a->u || !a->w || !a->mass || !a->leaf_token) return api_fail(GLB_EINVAL, "%s: null u, w, mass or leaf_token", what);
  if (!a->out_parent || !a->out_token || !a->out_node || !a->out_alive || !a->out_u || !a->out_w)
    return api_fail(GLB_EINVAL, "%s: null out_parent, out_token, out_node, out_alive, out_u or out_w", what);
  if (!a->out_spawned || !a->out_n_spawned) return api_fail(GLB_EINVAL, "%s: null out_spawned or out_n_spawned", what);
  if (a->out_node == a->node || a->out_alive == a->alive || a->out_u == a->u || a->out_w == a->w)
    return api_fail(GLB_EINVAL, "%s: the new state may not lie over the old one", what);
  hipLaunchKernelGGL(bytelm_extend_kernel, dim3(grid_for(a->n_groups)), dim3(64), 0, (hipStream_t)stream, *a);
  hipLaunchKernelGGL(bytelm_compact_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *a);
  return glb::launched(what);
}

int glb_bytelm_next(const glb_bytelm_args *a, void *stream) {
  const char *const what = "glb_bytelm_next";
  if (const int rc = common_checks(a, what)) return rc;
  if (!a->u || !a->w || !a->mass) return api_fail(GLB_EINVAL, "%s: null u, w or mass", what);
  if (a->byte == nullptr && (!a->out_next || !a->out_logZ)) return api_fail(GLB_EINVAL, "%s: null out_next or out_logZ", what);
  if (a->byte != nullptr && !a->logp) return api_fail(GLB_EINVAL, "%s: byte given without logp", what);
  hipLaunchKernelGGL(bytelm_next_kernel, dim3(grid_for(a->n_groups)), dim3(64), 0, (hipStream_t)stream, *a);
  return glb::launched(what);
}

int glb_bytelm_step(const glb_bytelm_step_args *p, void *stream) {
  const char *const what = "glb_bytelm_step";
  if (const int rc = glb::block_ok(p, what, "glb_bytelm_step_args")) return rc;
  const glb_bytelm_args *a = &p->beam;
  if (const int rc = common_checks(a, what)) return rc;
  if (!a->u || !a->w || !a->mass) return api_fail(GLB_EINVAL, "%s: null u, w or mass", what);
  if (p->n_states <= 0 || p->n_states > 0x7fffffffll / 256)
    return api_fail(GLB_EINVAL, "%s: n_states=%lld must be positive and n_states * 256 within 31 bits", what, (long long)p->n_states);
  if (!p->delta || !p->accepting || !p->live) return api_fail(GLB_EINVAL, "%s: null delta, accepting or live", what);
  if ((p->arc_logw == nullptr) != (p->final_logw == nullptr))
    return api_fail(GLB_EINVAL, "%s: arc_logw and final_logw come together or not at all", what);
  if (!p->state || !p->ended || !p->out_logZc) return api_fail(GLB_EINVAL, "%s: null state, ended or out_logZc", what);
  if (!p->peek) {
    if (!a->logp || !p->log_weight) return api_fail(GLB_EINVAL, "%s: an advance needs logp and log_weight", what);
    if (a->byte == nullptr && !p->out_byte) return api_fail(GLB_EINVAL, "%s: a drawn byte needs out_byte", what);
  }
  hipLaunchKernelGGL(bytelm_step_kernel, dim3(grid_for(a->n_groups)), dim3(64), 0, (hipStream_t)stream, *p);
  return glb::launched(what);
}

}  // extern "C"
