/*
 * glb.h — C ABI of libglb_hip.so, the MI355X (gfx950) implementation of genlm-backend's
 * autobatched next_token_logprobs hot path.
 *
 * Every entry point is `extern "C"`, takes plain device/host pointers and sizes, returns an
 * int status (GLB_OK == 0) and never throws.  On failure a thread-local message is available
 * through glb_last_error().  The library never allocates or frees caller memory: all buffers,
 * including scratch, are caller-owned (torch-allocated in the Python host) and must stay valid
 * until the passed HIP stream has reached the end of the call.  Kernels are enqueued on the
 * caller's stream; no entry point synchronises the device unless its comment says so.
 *
 * Each entry point cites the reference (genlm/genlm-backend) code it replaces; paths are
 * relative to the reference checkout.
 *
 * Arithmetic contract ("GLB math"): a logits row is a sequence of 4096-element chunks, each
 * with its own binary scale; the terms of a correctly-rounded-FMA polynomial exp are added in float32 in a fixed
 * order inside each of a chunk's 256 (lane, class) groups of 16 elements and as integers (floor(P * 2^36)) above
 * that, so logZ / lse / sampled token are bit-identical for any launch geometry, GPU count or particle split,
 * and are restated bit-for-bit by oracle/glb_oracle.c.
 */
#ifndef GLB_H
#define GLB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLB_ABI_VERSION 9

/* status codes */
enum {
  GLB_OK = 0,
  GLB_EINVAL = 1,      /* bad argument (null pointer, zero size, bad enum, misaligned ld) */
  GLB_EUNSUPPORTED = 2,/* valid request the build cannot serve (e.g. vocab too large for scratch) */
  GLB_EHIP = 3,        /* HIP runtime error (message carries hipGetErrorString) */
  GLB_ENOSPC = 4       /* caller-provided workspace too small */
};

/* element types of a logits matrix */
enum { GLB_F32 = 0, GLB_BF16 = 1, GLB_F16 = 2 };

/* mask kinds (README.md:57-70 builds two shared {0,-inf} masks; real grammars give per-row masks) */
enum {
  GLB_MASK_NONE = 0, /* no mask: logZ == 0 up to rounding, sample from the full distribution      */
  GLB_MASK_BITS = 1, /* table [n_masks, mask_ld] of uint32 words, bit j%32 of word j/32 == 1 ⇔
                        token j allowed (log-mask 0), 0 ⇔ forbidden (log-mask -inf).  The one-launch step
                        reads these rows as they are (every lane the words that hold its elements' bits:
                        what a grammar that changes every particle's mask every step hands over); the
                        two-launch forms bring them into GLB_MASK_PREPARED's layout in the workspace first */
  GLB_MASK_F32 = 2,  /* table [n_masks, mask_ld] of float additive log-masks (any value, -inf ok) */
  GLB_MASK_PREPARED = 3 /* bit masks already brought into the kernels' layout by glb_mask_prepare (same
                        meaning as GLB_MASK_BITS; saves one small launch per call for masks that are
                        built once, like the two README masks)                                     */
};

/* glb_step_args.flags.
 * GLB_STEP_HW_EXP: the second arithmetic contract of the step - a term is the hardware's 2^y,
 * t = v_exp_f32(fma(x, log2 e, -(N_c + 1))), instead of the polynomial.  Same chunks, same
 * (lane, class) float32 sums in load order, same integer sums, records and draws, so results are still deterministic and
 * independent of launch geometry and particle sharding ON gfx950; v_exp_f32 is within one ulp of 2^y (the polynomial:
 * 2.7e-6) but not correctly rounded, so oracle/glb_oracle.c restates this contract with exp2f and the comparison is by
 * tolerance: logZ / lse within 1e-4 of the reference (observed 1e-6), parity-mode tokens identical on every golden,
 * Philox tokens equal to the oracle's except where a draw lands within 2^-20 of a boundary of the inverse CDF
 * (tests/test_step_gpu.py counts them).  What it buys: the exponential is 9 of the 13 vector instructions per element of
 * the polynomial contract and 16-bit rows are bound by instruction issue (512 x 128256 bf16 31.5 ->
 * 27 us); cache.py:96 keeps the logits' dtype, so 16-bit rows are every Llama-class checkpoint's case.  float32 rows are
 * bound by memory and gain less (1024 x 50257: 38.0 -> 36.6 us): the Python host sets the flag for 16-bit rows by default
 * ("auto") and for float32 rows only when asked ("hw"), so that float32 results stay the oracle's bit for bit. */
enum { GLB_STEP_HW_EXP = 1 };

/* RNG modes of the categorical draw */
enum {
  GLB_RNG_NONE = 0,   /* no draw (out_token untouched)                                            */
  GLB_RNG_PHILOX = 1, /* in-kernel Philox4x32-10, two 64-bit uniforms per particle: exact integer inverse
                         CDF over the row's 4096-token chunks, then down the chunk's summation tree: lane,
                         class, element                                              */
  GLB_RNG_NOISE = 2   /* parity mode: caller supplies Exp(1) noise E[n_particles, noise_ld] drawn
                         the way torch.multinomial draws it on CPU; token = first argmax p_j/E_j
                         (README.md:87, base.py:137-141)                                          */
};

const char *glb_version(void);
int glb_abi_version(void);
/* copies the calling thread's last error message (NUL-terminated, truncated to n) */
int glb_last_error(char *buf, size_t n);
/* number of visible HIP devices, or -1 when the runtime cannot initialise (no GPU) */
int glb_device_count(void);

/*
 * Fused particle step.  Replaces, per particle,
 *     logps  = log_softmax(logits_row)                      cache.py:96
 *     masked = logps + mask                                 README.md:84
 *     logZ   = masked.logsumexp(-1)                         README.md:85
 *     token  = multinomial((masked - logZ).exp(), 1)        README.md:87   (base.py:136-141 with
 *                                                           logit_scale = 1/temperature)
 * in one pass over the logits row.  Particle i reads row row_of[i] (dedup fan-out of
 * hf.py:214-220,285-288) and mask row mask_id[i].  When the mask is a function of the context - as in
 * the README, where it depends on len(context) only - pass the ids per logits ROW (row_mask_id) instead:
 * a row shared by several particles is then reduced once and only the draw is done per particle (any number of
 * particles per row: the reduction leaves what every draw needs, whoever makes it).
 */
typedef struct glb_step_args {
  uint32_t struct_size; /* sizeof(glb_step_args) — ABI guard */
  /* logits of the unique contexts */
  const void *logits; /* [n_rows, ld] device */
  int32_t dtype;      /* GLB_F32 / GLB_BF16 / GLB_F16 */
  int64_t n_rows;
  int64_t vocab; /* V */
  int64_t ld;    /* row pitch in elements, >= vocab */
  float logit_scale; /* x' = fl(x * logit_scale) when != 1 (1/temperature of base.py:136) */
  /* particles */
  int64_t n_particles;
  const int32_t *row_of; /* [n_particles] device, nullable ⇒ identity (needs n_particles == n_rows) */
  /* mask */
  int32_t mask_kind;
  const void *mask;  /* [n_masks, mask_ld] device (uint32 words or float) */
  int64_t mask_ld;   /* pitch in words (BITS, >= ceil(V/32)) or floats (F32, >= V) */
  int64_t n_masks;
  const int32_t *mask_id; /* [n_particles] device, nullable ⇒ identity (needs n_masks == n_particles)
                             or, when n_masks == 1, everybody uses mask 0 */
  const int32_t *row_mask_id; /* [n_rows] device, nullable: mask ids per logits row instead of per particle
                             (exclusive with mask_id); null ids ⇒ identity over rows / mask 0 as above */
  /* rng */
  int32_t rng_mode;
  const float *noise; /* GLB_RNG_NOISE: [n_particles, noise_ld] device */
  int64_t noise_ld;   /* >= vocab, or 0: ONE row shared by every particle (base.py:148-179 seeds every sequence of a
                         batch_sample call alike) */
  uint64_t seed;          /* GLB_RNG_PHILOX key */
  uint64_t offset;        /* GLB_RNG_PHILOX counter word (e.g. SIS step number) */
  int64_t particle_base;  /* global index of particle 0 of this call (multi-GPU shards) */
  /* outputs, each nullable */
  float *out_logZ;   /* [n_particles] logsumexp(log_softmax(x)+mask) */
  float *out_lse;    /* [n_particles] logsumexp(x) of the particle's row */
  int32_t *out_token;/* [n_particles] sampled id, -1 when every token is masked out (-2, with NaN logZ / lse: a
                        finishing wave gave up waiting for its row's records - a failed launch, never a result) */
  float *out_margin; /* [n_particles] GLB_RNG_NOISE only: (winner - runner-up) / winner of the race e_j / E_j, i.e. how
                        far the draw is from a tie that float rounding could flip (1 if there is no runner-up) */
  int32_t flags;     /* 0 or GLB_STEP_HW_EXP; any other bit: GLB_EINVAL */
  /* device scratch of >= glb_step_workspace_bytes(...) bytes, 32-byte aligned: the per-chunk records (64 bytes per
     row and 4096-token chunk) the reducing waves hand to the per-particle waves (and, for GLB_MASK_BITS, the prepared
     masks).  See glb_workspace_init. */
  void *workspace;
  size_t workspace_bytes;
} glb_step_args;

size_t glb_step_workspace_bytes(int64_t n_particles, int64_t n_rows, int64_t vocab, int64_t n_masks);
int glb_logprob_mask_sample(const glb_step_args *args, void *hip_stream);
/*
 * The same call with two HIP events (hipEvent_t, created by the caller with timing enabled; either may be null) that
 * the step's first launch carries as its start stamp and its last launch as its stop stamp (hipExtLaunchKernel):
 * hipEventElapsedTime(start, stop) is then the duration of the step's launch(es) on the device - what a profiler
 * reports for them - without the marker packets of hipEventRecord around the call.  For measurement (bench.py).
 */
int glb_logprob_mask_sample_timed(const glb_step_args *args, void *hip_stream, void *start_event, void *stop_event);

/*
 * A step workspace that was zeroed and registered with glb_workspace_init is served in ONE launch: the waves that
 * reduce the rows tag every record with the call's epoch (counted per workspace by the library) and the waves that
 * finish the particles, dealt at the end of the same grid, sweep the records of their row until all tags are fresh.
 * Call it once after allocating the buffer (enqueues one memset on the stream), and glb_workspace_release before
 * freeing it or handing the memory to anything else.  Workspaces nobody initialised, calls made while the stream is
 * being captured into a graph, and GLB_RNG_NOISE calls take two launches - same results, bit for bit.  A workspace
 * serves one call at a time (as before: it is scratch).
 */
int glb_workspace_init(void *workspace, size_t workspace_bytes, void *hip_stream);
int glb_workspace_release(void *workspace);
/*
 * The one-launch forms (fused step, log-softmax rows) have waves that wait, inside the launch, for records other waves
 * of the same launch write.  HIP promises no dispatch order, so every such wait is bounded by a watchdog (2 s by
 * default; glb_set_spin_limit, 0 = default): a wave that gives up writes token -2 and NaN logZ / lse (NaN rows for
 * glb_log_softmax_rows) and adds 1 to the error word in the last 64 bytes of the registered workspace - which is why a
 * registered workspace serves the calls of ONE stream at a time, and why its size should come from the *_workspace_bytes
 * functions (they leave that room).  The calls themselves return GLB_OK: they do not synchronise.
 *   glb_workspace_check       synchronises `hip_stream`, returns GLB_EHIP (and clears the word) if any wave gave up since
 *                             the last check - the results of those calls must not be used -, GLB_OK otherwise
 *   glb_workspace_error_word  the word's device address, for hosts that already copy results back and want it to ride
 *                             along (null for a workspace that is not registered); nonzero = failed, as above
 * The reference's counterpart of "nobody is left with a silent wrong answer" is vllm.py:396-400.
 */
int glb_workspace_check(void *workspace, void *hip_stream);
const uint32_t *glb_workspace_error_word(void *workspace);
#define GLB_SPIN_NONE UINT64_MAX /* give up at the first poll that finds a record missing: forces the failure path (tests) */
int glb_set_spin_limit(uint64_t microseconds);

/*
 * Bring GLB_MASK_BITS rows into the layout the kernels read ([mask][chunk][vector][component] 64-bit lane
 * words) once, for masks that do not change between steps (the two README masks, README.md:57-70).  `dtype` is the element type of the
 * logits the masks will be used with (the lane layout differs between 4- and 2-byte elements).  Pass the
 * result as `mask` with mask_kind = GLB_MASK_PREPARED and the same n_masks / vocab.
 */
size_t glb_mask_prepared_bytes(int64_t n_masks, int64_t vocab);
int glb_mask_prepare(const uint32_t *mask_bits, int64_t n_masks, int64_t vocab, int64_t mask_ld, int32_t dtype,
                     void *out_prepared, size_t out_bytes, void *hip_stream);
/*
 * Masks that change a few at a time (a grammar moves one particle's mask per token, README.md:57-70 generalised): re-prepare
 * ONLY the masks rows[0 .. n_rows) (device int32; entries outside [0, n_masks) are skipped) of a buffer glb_mask_prepare
 * filled before - the other masks' lane words stay as they are, so a steady-state call pays for what changed, not for
 * n_masks x ceil(V / 8) bytes in and out.
 */
int glb_mask_prepare_rows(const uint32_t *mask_bits, int64_t n_masks, int64_t vocab, int64_t mask_ld, int32_t dtype,
                          const int32_t *rows, int64_t n_rows, void *prepared, size_t prepared_bytes, void *hip_stream);

/*
 * Materialise log-probabilities: out[r, j] = x[r, j] - logsumexp(x[r, :]).  Replaces the
 * per-position torch.log_softmax of TokenTrie.extend_cache (cache.py:93-98) and
 * next_token_logprobs_uncached (hf.py:422).  out_lse is optional.  workspace: device scratch of at least
 * glb_log_softmax_workspace_bytes(n_rows, vocab) bytes, 32-byte aligned.  On a workspace glb_workspace_init has seen
 * (and outside stream capture, rows of at most 262144 elements) the call is one launch that reads every logit once
 * and keeps it on the chip until its log-probability is written; otherwise three launches.  Same bits either way.
 * out_dtype: GLB_F32, or the logits' own dtype - the reference returns log-probabilities in the model's dtype
 * (cache.py:96 keeps it): the float32 result rounded to nearest even, out_ld in elements of that type; for 16-bit
 * models that is a third fewer bytes per call (512 x 128256 bf16: 263 MB instead of 394 MB).
 */
size_t glb_log_softmax_workspace_bytes(int64_t n_rows, int64_t vocab);
int glb_log_softmax_rows(const void *logits, int32_t dtype, int64_t n_rows, int64_t vocab,
                         int64_t ld, float logit_scale, void *out_logprobs, int32_t out_dtype, int64_t out_ld,
                         float *out_lse, void *workspace, size_t workspace_bytes, void *hip_stream);

/*
 * Convert {0,-inf}-style float log-masks (README.md:60-66, `.log()` of a 0/1 tensor) to the
 * packed GLB_MASK_BITS form: bit = (mask[j] == 0).  Values other than 0 / -inf set *out_nonbinary
 * (device int32, optional) to 1 so the caller can fall back to GLB_MASK_F32.
 */
int glb_mask_f32_to_bits(const float *mask, int64_t n_masks, int64_t vocab, int64_t mask_ld,
                         uint32_t *out_bits, int64_t bits_ld, int32_t *out_nonbinary,
                         void *hip_stream);

/*
 * Ragged contexts are passed as (tokens, starts, lengths): context i is
 * tokens[starts[i] .. starts[i] + lengths[i]), int32 token ids, int64 starts, int32 lengths, all on
 * the device.  This covers both a CSR buffer and the rows of a padded [n, cap] particle matrix.
 *
 * Context grouping: exact dedup of ragged token contexts, first-appearance order.  Replaces the
 * dict keyed by tuple(prompt) of batch_evaluate_queries (hf.py:214-220).
 *   out_group_of [n]   group id of every context (ids numbered by first appearance)
 *   out_rep      [n]   out_rep[g] = smallest context index in group g (only [0, n_groups) valid)
 *   out_n_groups [1]   device int32
 * workspace: device scratch of at least glb_group_contexts_workspace(n) bytes.
 * ctx_hashes (nullable, [n] device): the contexts' hashes as glb_hash_contexts makes them and glb_particles_advance
 * keeps them up to date - a context's hash extends token by token, so a loop that only appends never reads its
 * contexts again to group them (the grouping itself is by exact comparison: hashes only place the slots).
 */
size_t glb_group_contexts_workspace(int64_t n);
int glb_group_contexts(const int32_t *tokens, const int64_t *starts, const int32_t *lengths,
                       int64_t n, const uint64_t *ctx_hashes, int32_t *out_group_of, int32_t *out_rep,
                       int32_t *out_n_groups, void *workspace, size_t workspace_bytes, void *hip_stream);
int glb_hash_contexts(const int32_t *tokens, const int64_t *starts, const int32_t *lengths, int64_t n,
                      uint64_t *out_hashes, void *hip_stream);

/*
 * Cached-prefix match ("trie grouping"): for every context pick the longest cached prefix that
 * is a proper prefix of it — the deepest KV-bearing trie node walk_cache returns (hf.py:314-344).
 *   cached prefixes in the same (tokens, starts, lengths) form
 *   out_prefix [n] int32 index of the chosen cached prefix or -1; out_base [n] int32 its length
 *   (0 when none).  Ties on length resolve to the lowest prefix index.
 */
int glb_match_prefixes(const int32_t *tokens, const int64_t *starts, const int32_t *lengths,
                       int64_t n, const int32_t *prefix_tokens, const int64_t *prefix_starts,
                       const int32_t *prefix_lengths, int64_t n_prefixes, int32_t *out_prefix,
                       int32_t *out_base, void *hip_stream);

/*
 * Ragged -> padded gather for the batched prefill.  Replaces Query.prompt_padded /
 * attention_mask / position_ids and the three torch.tensor(...) builds of hf.py:55-70,232-246.
 * For each selected context s = sel[u] (u < n_sel; sel nullable ⇒ identity) with cached-prefix
 * length base[s] (nullable ⇒ 0):
 *   input_ids[u, t]      = tokens[starts[s] + base + t]         t <  len          else pad_id
 *   position_ids[u, t]   = base + t                             t <  len          else 0
 *   attention_mask[u, p] = 1 for p < base; 0 for base <= p < p_max;
 *                          1 for p_max <= p < p_max + len; 0 afterwards           (hf.py:58-64)
 *   last_index[u]        = len - 1        (row of the next-token logits, optional output)
 * with len = lengths[s] - base.  Outputs are int64 [n_sel, l_max] /
 * [n_sel, p_max + l_max], matching what transformers expects.
 */
int glb_gather_padded(const int32_t *tokens, const int64_t *starts, const int32_t *lengths,
                      const int32_t *sel, int64_t n_sel, const int32_t *base, int64_t pad_id, int64_t p_max,
                      int64_t l_max, int64_t *out_input_ids, int64_t *out_attention_mask,
                      int64_t *out_position_ids, int32_t *out_last_index, void *hip_stream);

/*
 * Batched prefix-KV assembly.  Replaces Query.past_padded + the per-layer torch.cat of
 * hf.py:33-53,247-271: out[u, h, p, :] = slab_k[h, p, :] for p < plen_k, zero up to p_max,
 * where k = prefix_of[u] (k < 0 ⇒ all zeros).  `slabs` is a device array of n_prefixes device
 * pointers to [heads, plen_k, head_dim] tensors of elem_bytes-wide elements (contiguous).
 */
int glb_gather_kv_padded(const void *const *slabs, const int32_t *slab_len, int64_t n_prefixes,
                         const int32_t *prefix_of, int64_t n_rows, int64_t heads,
                         int64_t head_dim, int64_t p_max, int32_t elem_bytes, void *out,
                         void *hip_stream);

/*
 * Particle bookkeeping of the SIS loop (README.md:82-91): for every particle that is active,
 *   log_weight += logZ; if token == eos_id (or token < 0) active = 0
 *   else tokens[i, length[i]++] = token; and a context that reaches max_len is deactivated.
 * `contexts` is the padded [n, ctx_ld] int32 matrix the ragged views are cut from.  ctx_hashes (nullable, [n]): the
 * contexts' hashes (glb_hash_contexts), extended by the appended token.
 */
int glb_particles_advance(int32_t *contexts, int64_t ctx_ld, int32_t *lengths, int32_t *active,
                          float *log_weights, const float *logZ, const int32_t *token, int64_t n,
                          int32_t eos_id, int32_t max_len, uint64_t *ctx_hashes, void *hip_stream);

/*
 * Weight normalisation over the full particle population (README.md:108-110) on the all-gathered
 * log-weight vector: out_probs = exp(lw - logsumexp(lw)); out_stats = {logsumexp(lw), ESS}.
 * Deterministic (fixed-point sums), so every rank of a sharded run computes identical values.
 */
int glb_normalize_weights(const float *log_weights, int64_t n, float *out_probs, float *out_stats,
                          void *hip_stream);

/*
 * Device-resident particle state (SURVEY.md §8 f1 / e): per-particle KV in preallocated slabs
 * [n_rows, heads, cap, head_dim] (one per layer and K/V) instead of the reference's per-query tuples that are
 * zero-padded and concatenated every batch (hf.py:33-53,247-271) or per-token trie slices (cache.py:103-191).
 *
 * glb_kv_append:      slab[row_of[i], h, pos[i], :] = new_rows[i, h, :]   - the new token's K or V of every forward
 *                     row (row_of nullable: row i; with rows SHARED by particles of equal contexts it is the block
 *                     table's row of forward row i); new_rows is addressed by element strides (usually a transposed view).
 * glb_kv_gather_rows: dst[t][i, h, p, :] = src[t][src_row_of[i], h, p, :] for p < len_of[i], all n_tensors
 *                     (layer, K|V) slabs in one launch through device arrays of device pointers.  Fans the KV of
 *                     the distinct prompts out to the particles and gathers ancestors' KV after a resampling
 *                     step; src_row_of[i] < 0 leaves row i untouched.  src and dst must not alias.
 * glb_gather_rows_i32: dst[i, :width] = src[row_of[i], :width]   - the particles' token matrices.
 */
int glb_kv_append(void *slab, const void *new_rows, const int32_t *pos, const int32_t *row_of, int64_t n_rows,
                  int64_t heads, int64_t cap, int64_t head_dim, int64_t new_stride_row, int64_t new_stride_head,
                  int32_t elem_bytes, void *hip_stream);
int glb_kv_gather_rows(const void *const *src, void *const *dst, int64_t n_tensors, int64_t n_rows, int64_t heads,
                       int64_t head_dim, int64_t src_cap, int64_t dst_cap, const int32_t *src_row_of,
                       const int32_t *len_of, int32_t elem_bytes, void *hip_stream);
int glb_gather_rows_i32(const int32_t *src, int64_t src_ld, const int32_t *row_of, int64_t n, int64_t width,
                        int32_t *dst, int64_t dst_ld, void *hip_stream);

/*
 * KV rows shared between contexts, decided on the device.  The reference keeps per-token KV on trie
 * nodes (cache.py:103-191, mlx.py:177-318); here the prefixes sit in slab rows and a block table says which.
 *
 * glb_match_rows: for every dedup group g < *n_groups (its context = rep[g]), the table row that holds exactly the
 *   context, else the row that holds its first L - 1 tokens, else -1 (the smallest row index wins among equals).  The
 *   table is (row_tok [n_rows, cap] int32, row_len [n_rows] - 0: the row holds nothing -, row_hash [n_rows]: the hash of
 *   glb_hash_contexts); hashes only select candidates, every candidate's tokens are compared.  out_hash [n] (nullable): the
 *   groups' own hashes, for the table update of glb_kv_plan.  Contexts longer than cap match nothing.
 *
 * glb_kv_plan: the block table of one step, one small launch.  In: the dedup of the step's contexts (group_of [n], rep,
 *   n_groups: glb_group_contexts' outputs), the contexts' lengths, and where every group's prefix sits now - old_row[g]
 *   (old_row_by_context == 0: glb_match_rows' output) or old_row[rep[g]] (old_row_by_context != 0: the previous step's
 *   out_row_of_context: a population that only appends).  Decides: the first group (by id) of every live row KEEPS it and
 *   appends in place; the other groups that grew out of that row get a COPY of the prefix in a free row (copy-on-append),
 *   groups without a row whose context fits one get a free row to be filled from an ENCODING, in that order, for as long as
 *   free rows last - handed out by ascending row index, or longest unused first when row_stamps [n_rows] (int64, the call
 *   that used the row last; updated to call_no for every row in use) is given.  Out (int32, device):
 *     out_group_row [n]       the group's row from now on (-1: none)
 *     out_logits_row [n]      the forward row of the group: groups with a prefix in a row first, the ones to encode behind
 *     out_rows_a / out_ctx_a / out_pos_a [n]   per forward row k < head[1]: slab row, context index, position of the token fed
 *     out_ctx_b / out_rows_b [n]               per encoded row k < head[2]: context index, the row that keeps its KV (-1: none)
 *     out_copy_src / out_copy_len [n_rows]     row r takes out_copy_len[r] positions of row out_copy_src[r] (-1: nothing)
 *     out_ctx_of_row / out_pos_of_row [n_rows] for a forward that runs on ALL rows where they lie: the context that feeds
 *                                              row r and the position its token goes to (-1: the row is not in this
 *                                              forward; -2: it is being filled from an encoding)
 *     out_row_of_context [n]  (nullable) out_group_row[group_of[i]]: next step's old_row
 *     out_head [8]            n_groups, rows with a prefix, rows to encode, copies, encoded rows nobody keeps, the longest
 *                             context to encode, free rows before the call, 0 - all the host has to read
 *   With row_tok != null the table rows of every group that holds a row now are rewritten (tokens zero-padded to cap,
 *   length, group_hash[g]).  workspace: glb_kv_plan_workspace(n, n_rows) bytes, 4-byte aligned.
  *   A group whose context has outgrown a row (length > cap) holds no row from this step on, whatever old_row says: it is
 *   encoded from its tokens and not kept, and the row it sat in is free again.  A position outside [0, cap) handed to
 *   glb_slab_attention appends nothing and gives NaN outputs for that row.
 */
int glb_match_rows(const int32_t *tokens, const int64_t *starts, const int32_t *lengths, const int32_t *rep,
                   const int32_t *n_groups, int64_t n, const int32_t *row_tok, const int32_t *row_len,
                   const uint64_t *row_hash, int64_t n_rows, int64_t cap, int32_t *out_old_row, uint64_t *out_hash,
                   void *hip_stream);
typedef struct glb_kv_plan_args {
  uint32_t struct_size; /* sizeof(glb_kv_plan_args) - ABI guard */
  int64_t n, n_rows, cap;
  const int32_t *group_of, *rep, *n_groups;
  const int32_t *old_row;
  int32_t old_row_by_context;
  const int32_t *lengths;
  int64_t *row_stamps; /* nullable */
  int64_t call_no;
  /* the table of what the rows hold (all nullable together) */
  int32_t *row_tok, *row_len;
  uint64_t *row_hash;
  const uint64_t *group_hash;
  const int32_t *tokens;
  const int64_t *starts;
  /* outputs */
  int32_t *out_group_row, *out_logits_row, *out_rows_a, *out_ctx_a, *out_pos_a, *out_ctx_b, *out_rows_b, *out_copy_src,
      *out_copy_len, *out_ctx_of_row, *out_pos_of_row, *out_row_of_context, *out_head;
  void *workspace;
  size_t workspace_bytes;
} glb_kv_plan_args;
size_t glb_kv_plan_workspace(int64_t n, int64_t n_rows);
int glb_kv_plan(const glb_kv_plan_args *args, void *hip_stream);

/*
 * KV rows that serve ANY shared prefix (the reference's DynamicTokenTrie keeps per-token KV, cache.py:103-191:
 * a context finds the longest prefix it shares with anything cached).  Three additions; the entry points above keep their
 * outputs bit for bit.
 *
 * glb_match_prefix_rows: glb_match_rows' inputs plus max_new (1 .. GLB_KV_CHUNK_MAX).  For a group's context of L tokens and a
 *   row r with row_len[r] > 0, let c be the length of the common prefix of the row's tokens and the context's and
 *   keep = min(c, L - 1).  r is a candidate when keep >= 1, L - keep <= max_new and L <= cap.  out_old_row[g]: the candidate
 *   with the largest keep - among equals a row that holds exactly the context, then the smallest row index - or -1;
 *   out_keep[g]: its keep (0 without a row); out_hash[g] (nullable): the group's hash, as glb_match_rows gives it.  Tokens
 *   are always compared (row_hash is not consulted: rows of every length are candidates).
 *
 * glb_kv_plan_chunk: glb_kv_plan with a kept length per group, old_keep (indexed as old_row is).  A row with a prefix is
 *   fed the tokens at positions keep .. L - 1 in one forward: out_pos_a / out_pos_of_row give the FIRST new position,
 *   out_n_new_a [n] / out_n_new_of_row [n_rows] the number of tokens (0: the row is not fed), out_copy_len the group's own
 *   keep.  Forward rows: the ones fed one token first, the ones fed more behind them (head[8] of them), then the rows to
 *   encode; out_ctx_of_row is -3 for a row that is fed a chunk (it is not part of a one-token forward over all rows).
 *   The claim rule of glb_kv_plan with one addition: a group may keep its matched row in place only if that row holds at
 *   most keep + 1 tokens (the parent, the context itself, a sibling).  A longer row is never truncated in place - the
 *   group takes a copy of its keep tokens into a free row and the long row stays as it is, not free in this call (its stamp
 *   is renewed).  The first group (by id) that may keep a row in place keeps it.  A group whose keep is outside
 *   0 .. L - 1, or with more than GLB_KV_CHUNK_MAX tokens behind it, reads as a group without a row.  The row table (plan.row_tok ...) is required.  plan.out_head has TEN words:
 *   the eight of glb_kv_plan (head[1] counts every row with a prefix), head[8] the rows fed more than one token, head[9]
 *   the largest number of tokens fed to a row.  With old_keep[g] == L - 1 for every group and matched rows of L - 1 or L
 *   tokens every output shared with glb_kv_plan equals it (one kernel serves both entries).
 *
 * glb_slab_attention_chunk: attention of a forward with up to max_new <= GLB_KV_CHUNK_MAX new tokens per row over slab rows
 *   where they lie.  q [n_rows, heads, max_new, head_dim], k_new / v_new [n_rows, kv_heads, max_new, head_dim] by element
 *   strides {row, head, position}, unit inner stride; slabs [n_slab_rows, kv_heads, cap, head_dim] contiguous; forward row r
 *   lives in slab row row_of[r] (null: r; the rows of one call are distinct); pos[r]: its first new position, n_new[r] in
 *   1 .. max_new.  Query t < n_new[r] attends positions 0 .. pos[r] + t: below pos[r] from the slab, from pos[r] on from
 *   k_new / v_new, never from what the slab held there; the n_new[r] new K / V are written to slab positions pos[r] ..
 *   once per (row, KV head).  out [n_rows, max_new, heads, head_dim] contiguous; outputs of t >= n_new[r] are zeros.  A
 *   chunk outside its row (pos < 0, pos + n_new > cap, n_new outside 1 .. max_new, a slab row outside the slab): nothing
 *   appended, the row's outputs NaN - glb_slab_attention's rule.  Output (r, h, t) and the slab afterwards carry the bits
 *   that t + 1 successive glb_slab_attention calls on that row leave.  float32 / bfloat16 / float16, head_dim 16 / 32 / 64 / 128
 *   (glb_slab_attention's),
 *   pointers and strides multiples of 16 bytes.  No atomics, no allocation: fit for a captured graph.
 */
#define GLB_KV_CHUNK_MAX 16
int glb_match_prefix_rows(const int32_t *tokens, const int64_t *starts, const int32_t *lengths, const int32_t *rep,
                          const int32_t *n_groups, int64_t n, const int32_t *row_tok, const int32_t *row_len,
                          const uint64_t *row_hash, int64_t n_rows, int64_t cap, int32_t max_new, int32_t *out_old_row,
                          int32_t *out_keep, uint64_t *out_hash, void *hip_stream);
typedef struct glb_kv_plan_chunk_args {
  uint32_t struct_size; /* sizeof(glb_kv_plan_chunk_args) - ABI guard */
  glb_kv_plan_args plan; /* as for the one-token entry (its own struct_size set); out_head: 10 words */
  const int32_t *old_keep;
  int32_t *out_n_new_a, *out_n_new_of_row;
} glb_kv_plan_chunk_args;
int glb_kv_plan_chunk(const glb_kv_plan_chunk_args *args, void *hip_stream);
int glb_slab_attention_chunk(const void *q, const int64_t q_strides[3], const void *k_new, const int64_t k_strides[3],
                             const void *v_new, const int64_t v_strides[3], void *k_slab, void *v_slab, const int32_t *pos,
                             const int32_t *n_new, const int32_t *row_of, int64_t n_rows, int64_t n_slab_rows, int64_t heads,
                             int64_t kv_heads, int64_t cap, int64_t head_dim, int64_t max_new, float scale, int32_t dtype,
                             void *out, void *hip_stream);

/*
 * Attention of a one-token forward over KV slab rows where they lie (the read side of the device-resident KV, SURVEY.md
 * §8 f1; the reference hands zero-padded per-query KV to the model's own attention, hf.py:247-281): for every row r and
 * query head h, softmax(q . K[r, h / G, 0 .. pos[r]] * scale) . V[r, h / G, 0 .. pos[r]], where position pos[r] is the token
 * of this forward - its K / V (k_new, v_new: [n_rows, kv_heads, head_dim], each by its own element strides: the projections' outputs)
 * are used from where they are AND written to slab position pos[r] (glb_kv_append, fused).  q by element strides
 * (row, head), unit inner stride; slabs [n_rows, kv_heads, cap, head_dim] contiguous; out [n_rows, heads, head_dim]
 * contiguous; all of one dtype, float32 accumulation; head_dim 16 / 32 / 64 / 128 (GLB_EUNSUPPORTED otherwise); every pointer and
 * stride a multiple of 16 bytes.  One launch per layer instead of two appends, a mask and a dense SDPA call.
 */
int glb_slab_attention(const void *q, int64_t q_stride_row, int64_t q_stride_head, const void *k_new, int64_t k_stride_row,
                       int64_t k_stride_head, const void *v_new, int64_t v_stride_row, int64_t v_stride_head, void *k_slab,
                       void *v_slab, const int32_t *pos,
                       int64_t n_rows, int64_t heads, int64_t kv_heads, int64_t cap, int64_t head_dim, float scale,
                       int32_t dtype, void *out, void *hip_stream);

/*
 * Masked attention of the padded batches of short contexts the path feeds the transformer (hf.py:232-281): for every row u,
 * query head h and query position t, softmax over the keys s it may see of q[u,h,t] . k[u,h/G,s] * scale, times v.  q / k / v
 * by element strides {row, head, position} with unit inner stride (the projections' outputs, cached prefixes in front of
 * the keys); mask: bool / uint8 [n_rows, q_len, k_len] by strides (row, query), nonzero = attend - the 4-D mask
 * transformers builds from the padding mask - or null: causal, key s <= t + k_len - q_len.  out [n_rows, q_len, heads,
 * head_dim] contiguous.  float32 accumulation; head_dim 16 / 32 / 64 / 128; pointers and strides multiples of 16 bytes.
 * One wave per (row, head, query): meant for q_len * k_len of a few hundred (a dozen tokens per context), where the
 * library SDPA kernels spend a fifth of a 24 ms step; long sequences stay with them.
 */
int glb_short_attention(const void *q, const int64_t q_strides[3], const void *k, const int64_t k_strides[3], const void *v,
                        const int64_t v_strides[3], const uint8_t *mask, int64_t mask_stride_row, int64_t mask_stride_query,
                        int64_t n_rows, int64_t heads, int64_t kv_heads, int64_t q_len, int64_t k_len, int64_t head_dim,
                        float scale, int32_t dtype, void *out, void *hip_stream);

/*
 * The same attention over a ROW-PACKED batch whose contexts share the rows of their prompt: q / k / v are
 * [n_rows, heads, head_dim] views by element strides {row, head} with unit inner stride (one projection output, read where
 * it lies), plan [n_segments][4] int32 on the device: (pre_start, pre_len, tail_start, tail_len) per segment.  The tail_len
 * queries of a segment are rows tail_start ..; its keys are rows pre_start .. pre_start + pre_len - 1 (the prompt, shared by
 * every context behind it), then rows tail_start ..; query t sees keys 0 .. pre_len + t.  A prompt is a segment with
 * pre_len = 0.  out [n_rows, heads, head_dim] contiguous; rows no segment names are not written.  max_keys: the most keys
 * (pre_len + tail_len) of a segment, 1 .. 32 - GLB_EINVAL beyond, nothing launched.  A query's output has the bits
 * glb_short_attention gives it on the right-padded batch of the same contexts.
 * The plan is device data: a segment with more than max_keys keys, no query, or rows outside [0, n_rows) is never
 * followed - it writes nothing and adds 1 to *err_word (a device word, e.g. glb_workspace_error_word's).  head_dim
 * 16 / 32 / 64 / 128 (GLB_EUNSUPPORTED otherwise); pointers and strides multiples of 16 bytes; n_segments * kv_heads and
 * n_rows below 2^31.
 */
int glb_short_attention_packed(const void *q, int64_t q_stride_row, int64_t q_stride_head, const void *k, int64_t k_stride_row,
                               int64_t k_stride_head, const void *v, int64_t v_stride_row, int64_t v_stride_head,
                               const int32_t *plan, int64_t n_segments, int64_t n_rows, int64_t heads, int64_t kv_heads,
                               int64_t max_keys, int64_t head_dim, float scale, int32_t dtype, void *out, uint32_t *err_word,
                               void *hip_stream);

/*
 * Systematic resampling of the whole population from the all-gathered log-weights (the step the all-gather of
 * README.md:108-110's weights exists for; the reference itself stops at the normalised weights).  Exact integer
 * comb over the fixed-point weights of glb_normalize_weights with one Philox draw keyed by (seed, offset):
 * every rank that holds the same gathered vector computes the same ancestors.
 *   out_ancestors [n] int32 (non-decreasing); out_stats [1] optional: logsumexp of the weights
 *   workspace: glb_resample_workspace(n) bytes, 8-byte aligned.  n <= 262144.
 */
size_t glb_resample_workspace(int64_t n);
int glb_resample_systematic(const float *log_weights, int64_t n, uint64_t seed, uint64_t offset,
                            int32_t *out_ancestors, float *out_stats, void *workspace, size_t workspace_bytes,
                            void *hip_stream);

/*
 * Token -> byte trie masses.  Replaces TokenCharacterTrie.weight_sum / weight_max and their batch_
 * forms (trie/base.py:147-213 with the numba loops at :346-393; trie/parallel.py:92-145): for every node of the
 * trie over the vocabulary's byte strings, the sum / maximum of the weights of the tokens below it, for a batch of
 * weight rows at once.  The trie arrives flattened (built once per vocabulary on the host):
 *   leaf_node   [vocab]        device: node id of token k's leaf
 *   level_start [n_levels + 1] HOST array (it sizes the launches): level_nodes[level_start[d] .. level_start[d+1]) are
 *   level_nodes                the internal nodes d levels above the deepest ones (device); a node's children always sit
 *                              in an earlier level or are leaves
 *   child_ptr   [n_nodes + 1], child_idx: device CSR of every node's children, ascending (the reference's `jump`)
 * out[r, node] = the value as float32; a node's children are added in ascending order in double and the result is
 * rounded to float32 per node (the reference keeps doubles: agreement to ~1e-7 relative per level).
 * from_logprobs != 0: weights = exp(row).  GLB_TRIE_MAX floors internal nodes at 0 like the reference (:385).
 * One launch for the leaves + one per tree level, all rows each.  Batches of 32 rows or more run on node-major
 * values (coalesced levels) if the caller lends glb_trie_workspace(n_rows, n_nodes) bytes of device scratch (16-byte
 * aligned; workspace may be null: the row-major kernels then serve any batch, a few times slower for large ones).
 */
enum { GLB_TRIE_SUM = 0, GLB_TRIE_MAX = 1 };
size_t glb_trie_workspace(int64_t n_rows, int64_t n_nodes);
int glb_trie_reduce(const float *weights, int64_t ld, int64_t n_rows, int64_t vocab, int64_t n_nodes, int64_t n_levels,
                    const int32_t *leaf_node, const int32_t *level_start_host, const int32_t *level_nodes,
                    const int32_t *child_ptr, const int32_t *child_idx, int32_t op, int32_t from_logprobs, float *out,
                    int64_t out_ld, void *workspace, size_t workspace_bytes, void *hip_stream);

/*
 * The same propagation with everything the pipeline around it wants (SURVEY.md §8 f2 "fuses with the logprob kernel"):
 *   - weights of any element type; with from_logprobs the leaf weight is exp(x * logit_scale - lse[r]): handing over the
 *     LOGITS and the lse the fused step returned (out_lse) gives the masses of softmax(logits) without a [B, V]
 *     log-probability matrix ever being written or read (lse nullable: then x are log-probabilities / weights);
 *   - three outputs, any subset: `out` row-major [n_rows, n_nodes]; `out_sel` [n_rows, n_sel], only the nodes a caller
 *     asks for (the children of the nodes its particles stand on); keep_node_major: nothing is transposed back, the
 *     values stay in `workspace` as float32 [n_nodes, pitch], pitch = n_rows rounded up to 64 (the 795 MB transposed
 *     copy of a 1024 x 194k-node batch is more than the propagation itself).
 * workspace: glb_trie_workspace_ex(n_rows, n_nodes) bytes, 16-byte aligned; without it only `out` is served (row-major
 * kernels).
 * The tree is whatever the arrays say: a caller may hand over its trie with the one-child nodes folded away (such a node
 * has its child's value, bit for bit; a byte trie of a BPE vocabulary is mostly such chains: 194 k nodes, 66 k of them
 * leaves or branching) - n_nodes then counts the remaining "slots", leaf_node / level_nodes / child_idx name slots, and
 * sel_nodes maps the nodes the caller wants (all of them, for the reference's [n_rows, n_nodes] result) to their slots.
 * The propagation then moves a third of the bytes (genlm_backend_amd.trie.TokenByteTrie.compact does this).
 */
typedef struct glb_trie_args {
  uint32_t struct_size;  /* sizeof(glb_trie_args) - ABI guard */
  const void *weights;   /* [n_rows, ld] device */
  int32_t dtype;         /* GLB_F32 / GLB_BF16 / GLB_F16 */
  int64_t ld, n_rows, vocab;
  const float *lse;      /* [n_rows] device, nullable */
  float logit_scale;     /* from_logprobs: x * logit_scale (1/temperature) */
  int32_t from_logprobs;
  int32_t op;            /* GLB_TRIE_SUM / GLB_TRIE_MAX */
  int64_t n_nodes, n_levels;
  const int32_t *leaf_node, *level_start_host, *level_nodes, *child_ptr, *child_idx; /* as glb_trie_reduce */
  float *out;            /* nullable */
  int64_t out_ld;
  const int32_t *sel_nodes; /* [n_sel] device */
  int64_t n_sel;
  float *out_sel;        /* nullable */
  int64_t out_sel_ld;
  int32_t keep_node_major;
  void *workspace;
  size_t workspace_bytes;
} glb_trie_args;
size_t glb_trie_workspace_ex(int64_t n_rows, int64_t n_nodes);
int glb_trie_masses(const glb_trie_args *args, void *hip_stream);

/*
 * The same masses with ONE ROW's values of a part of the trie resident in LDS (round 4; glb_trie.hip).  Replaces the
 * batch paths of trie/base.py:196-216 and trie/parallel.py:92-145 for row-major results: the weights are read once
 * and the output written once - no node-major scratch, no transposes.  `plan` is the folded trie cut into parts of at
 * most 160 KB / 6 slots (a slot takes a float32 value and a 16-bit child pointer in LDS;
 * genlm_backend_amd.trie.TokenByteTrie.plan builds it; every array lives on the device):
 *   desc [n_parts + 1][16] int32, per part: slot_base, n_local, n_roots, n_depths, (unused), cptr_off, leaf_off,
 *        n_leaves, cut_base, node_off, n_nodes, inode_off, n_inodes, idepth_off, run_off, n_runs; part n_parts is the
 *        top when n_top > 0
 *   local slots of a part are numbered breadth first over its subtrees: the children of local slot s are
 *        cptr16[cptr_off + s] .. cptr16[cptr_off + s + 1] (ascending child order; cptr_off even)
 *   inode16 [inode_off ..+ n_inodes] (inode_off even): the part's internal local slots depth by depth; depth k is
 *        idepth[idepth_off + k] .. idepth[idepth_off + k + 1] of them, its children all sit in depth k + 1
 *   leaf_src / leaf_local [leaf_off ..+ n_leaves]: the part's tokens in ascending order (top: indices of cut roots) and
 *        the local slots their weights go to
 *   the trie nodes whose value a local slot of the part holds are n_runs runs of consecutive node ids (a subtree is an
 *        interval of the post-order numbering): run_tab [run_off ..+ n_runs][2] = (first node, count), and
 *        pn_local16 [node_off ..+ n_nodes]: the local slots of those nodes, run after run
 *   top_local [n_top]: local slot of top slot top_base + i;  slot_of [n_nodes]: node -> slot (parts first, top last)
 *   lds_bytes: the largest part's 4 n_local + 2 (n_local + 1, rounded up to even) + 2 (n_inodes, rounded up to even)
 *        + 128 (its depth table: n_depths <= 30)
 * Same arithmetic per node as glb_trie_reduce (children in ascending order, accumulated in double, stored as float32),
 * so the results are bit-equal to glb_trie_masses on the same folded trie.
 * Outputs (any subset): out_slots [n_rows, n_slots] in the plan's slot numbering; out_nodes [n_rows, n_nodes];
 * out_sel [n_rows, n_sel] = the nodes sel_nodes[0 .. n_sel), n_sel <= 2^20 - or, with sel_row_stride, every row's own
 * nodes.  workspace: glb_trie_rows_workspace bytes (the values of the parts' subtree roots, read by the top's launch; the
 * slots of the selected nodes; a row's needed parts).
 */
typedef struct glb_trie_plan {
  uint32_t struct_size;  /* sizeof(glb_trie_plan) - ABI guard */
  int32_t n_parts, n_top, n_cut, n_slots, max_local, top_base, lds_bytes;
  int64_t n_nodes;
  const int32_t *desc, *idepth, *leaf_src, *leaf_local, *run_tab, *top_local, *slot_of;
  const uint16_t *cptr16, *inode16, *pn_local16;
  /* ABI 8 - a SWEEP plan (tok_local16 non-null; TokenByteTrie.plan(sweep=True)): a (row, part) workgroup reads the whole
   * row front to back instead of gathering the part's tokens; a persistent workgroup keeps a part's values in LDS
   * (lds_bytes >= 4 * max_local + 128: parts of up to 40 000 slots), the tokens' slots and the part's internal nodes in
   * registers, and has the head of the next row on its way while it reduces and writes the current one:
   *   tok_local16 [n_parts][(vocab + 7) & ~7]: token -> its local slot in that part; another part's token -> a word of the
   *            32-word slack behind the part's values, n_local + (token / 8) % 32 (the kernel stores every token's weight);
   *   inode64: per part at desc[D_INODE_OFF], the part's internal nodes as inode16 lists them (depth by depth):
   *            local slot | first child << 16 | number of children << 32;
   *   lds_top_bytes: the LDS of the launch over the top (its values and 16-bit tables, as for a gathered part);
   *   vocab: the vocabulary tok_local16 was made for (glb_trie_rows_args.vocab must equal it).
   * All null / 0: the gathered plan of rounds 4-5. */
  const uint16_t *tok_local16;
  const uint64_t *inode64;
  int32_t lds_top_bytes, vocab;
} glb_trie_plan;
typedef struct glb_trie_rows_args {
  uint32_t struct_size;  /* sizeof(glb_trie_rows_args) - ABI guard */
  const void *weights;   /* [n_rows, ld] device */
  int32_t dtype;         /* GLB_F32 / GLB_BF16 / GLB_F16 */
  int64_t ld, n_rows, vocab;
  const float *lse;      /* [n_rows] device, nullable (from_logprobs: exp(x * logit_scale - lse[r])) */
  float logit_scale;
  int32_t from_logprobs;
  int32_t op;            /* GLB_TRIE_SUM / GLB_TRIE_MAX */
  float *out_slots;      /* nullable */
  int64_t out_slots_ld;
  float *out_nodes;      /* nullable */
  int64_t out_nodes_ld;
  const int32_t *sel_nodes; /* [n_sel] device */
  int64_t n_sel;
  float *out_sel;        /* nullable */
  int64_t out_sel_ld;
  void *workspace;
  size_t workspace_bytes;
  int64_t sel_row_stride; /* 0: sel_nodes [n_sel] is one selection for every row.  > 0: a selection PER ROW - sel_nodes
                             [n_rows, sel_row_stride], row r asks for its first n_sel entries (a negative entry: nothing,
                             its output is 0; n_rows * n_sel <= 2^20) - e.g. every particle's current node's children, what a
                             byte-level sampler reads after trie/base.py:147-213.  Only the parts of the trie that hold a row's
                             nodes are read and reduced for that row (every part when a node sits above the cut). */
} glb_trie_rows_args;
size_t glb_trie_rows_workspace(int64_t n_rows, const glb_trie_plan *plan);
int glb_trie_rows(const glb_trie_rows_args *args, const glb_trie_plan *plan, void *hip_stream);

/*
 * torch's CPU generator for GLB_RNG_NOISE (parity mode).  The reference draws every token with torch.multinomial on the
 * CPU (README.md:87, base.py:136-141): V float32 Exp(1) variates per particle from ONE serial MT19937 stream - each
 * variate is one random64() = two MT words, u = (r & (2^53 - 1)) 2^-53, E = (float)(-log1p(-u)) - particles in
 * resolution order (hf.py:285-288).
 *
 * Host, serial (validation, small cases): glb_mt19937_seed + glb_mt19937_exponential_f32 fill out[0..n) with what
 * torch.empty(n).exponential_(1, generator) produces for a generator seeded alike.  Host pointers only.
 */
typedef struct glb_mt19937 {
  uint32_t mt[624];
  int32_t idx;
} glb_mt19937;
void glb_mt19937_seed(glb_mt19937 *st, uint64_t seed);
int glb_mt19937_exponential_f32(glb_mt19937 *st, float *out, int64_t n);

/*
 * The same stream on the DEVICE, entered at every particle's row at once (csrc/glb_mt.hip).  The stream's position is a
 * WINDOW: the 624 untempered words x[o .. o+623] that precede the next output (after seeding: the seeded array itself,
 * glb_mt19937_window).  A window `J` words ahead is g_J(T) applied to a window, g_J(t) = t^J mod the generator's minimal
 * polynomial: glb_mt19937_jump_polys computes, on the host, once per stride (stride_words = 2 V: one particle's row),
 *     polys[r]           = g_{r * stride}              r = 0 .. n_small - 1
 *     polys[n_small + m] = g_{m * n_small * stride}    m = 0 .. n_big - 1
 * (GLB_MT_POLY_WORDS 64-bit words each, coefficient i = bit i % 64 of word i / 64; about 2 ms per polynomial), enough
 * for n_small * n_big - 1 rows per call.  glb_mt19937_jump_host applies one polynomial to a window on the host (tests).
 * Only the top bit of a window's word 0 is state; its other 31 bits are unspecified after a jump.
 */
#define GLB_MT_POLY_WORDS 312
int glb_mt19937_window(uint64_t seed, uint32_t *out_window /* [624] host */);
int glb_mt19937_jump_polys(int64_t stride_words, int32_t n_small, int32_t n_big, uint64_t *out_polys /* host */);
int glb_mt19937_jump_host(const uint32_t *window_in, const uint64_t *poly, uint32_t *window_out);
/*
 * out[i, 0..V) = the V exponentials of stream row row_slot[i] (row k = words [2 V k, 2 V (k + 1)) after the position
 * `window`); row_slot[i] < 0: a row of ones (a particle that draws nothing this step); row_slot null: identity.  Then
 * window_out (nullable; may be `window` itself) = the position after *n_draw rows (n_draw: device scalar <= max_draw_rows,
 * null: max_draw_rows) - the stream moves on by what was consumed, decided on the device.  Three launches, no host
 * synchronisation.  All pointers device pointers.  When the output rows take at most half of the stream's rows (a rank of a
 * sharded population that enters ONE global stream: n_out_rows of max_draw_rows), only the windows some output row - or
 * window_out - reads are made (a word per row in the workspace says which).
 */
typedef struct glb_mt_rows_args {
  uint32_t struct_size;
  const uint32_t *window;   /* [624] */
  uint32_t *window_out;     /* [624], nullable */
  const uint64_t *polys;    /* [(n_small + n_big), GLB_MT_POLY_WORDS] as glb_mt19937_jump_polys made them for stride 2 * vocab */
  int32_t n_small, n_big;
  int64_t vocab;            /* V */
  int64_t max_draw_rows;    /* host: upper bound of the stream rows this call consumes; < n_small * n_big */
  const int32_t *n_draw;    /* device scalar, nullable */
  int64_t n_out_rows;
  const int32_t *row_slot;  /* [n_out_rows], nullable */
  float *out;               /* [n_out_rows, out_ld] */
  int64_t out_ld;           /* >= vocab */
  void *workspace;          /* >= glb_mt19937_rows_workspace(max_draw_rows, n_small) bytes */
  size_t workspace_bytes;
  /* Two-phase use (ABI 8), for a caller that generates the NEXT step's rows ahead of time on another stream - they do not
   * depend on the step's data, only on where the stream stands -: call 1 (ahead): row_slot null, n_out_rows = the rows
   * that may be needed, out = a buffer G, window_out null.  Call 2 (when the step knows its row_slot and n_draw), same
   * window / polys / max_draw_rows / workspace: reuse_windows = 1 (the workspace still holds every row's window: the two
   * jump launches are skipped), rows_from = G (out rows are COPIED from G[row_slot[i]], ones for a negative slot, instead of
   * generated), window_out = the position after *n_draw rows.  Both 0 / null: one call does everything. */
  int32_t reuse_windows;
  const float *rows_from;   /* [>= max_draw_rows, rows_from_ld] */
  int64_t rows_from_ld;
} glb_mt_rows_args;
size_t glb_mt19937_rows_workspace(int64_t max_draw_rows, int32_t n_small);
int glb_mt19937_exponential_rows(const glb_mt_rows_args *args, void *hip_stream);

/*
 * The path's one collective for a caller WITHOUT PyTorch (SURVEY.md §8(b) sketched glb_allgather_f32(comm, ...)): once the
 * particles are split over GPUs, README.md:108-110's normalisation needs every shard's log-weights on every rank - an
 * all-gather of n floats per rank over RCCL / xGMI (4 KiB at 1024 particles: latency-bound).  Rank 0 makes an id
 * (glb_comm_unique_id, GLB_COMM_ID_BYTES bytes) and hands it to the other ranks by whatever channel the integrator has;
 * every rank calls glb_comm_init with its device current; recv holds world * n floats, rank-major.  RCCL is taken from the
 * process at run time (dlopen); GLB_EUNSUPPORTED when there is none.  The Python host uses torch.distributed ("nccl" is
 * the same RCCL) and never calls these.
 */
#define GLB_COMM_ID_BYTES 128
int glb_comm_unique_id(void *out_id);
int glb_comm_init(const void *id, int32_t rank, int32_t world, void **out_comm);
int glb_allgather_f32(void *comm, const float *send, int64_t n, float *recv, void *hip_stream);
int glb_comm_destroy(void *comm);

/*
 * fp32 projection GEMM on bf16 MFMA ("split bf16"): C[m, n] = A[m, k] . W[k, n] + bias, optionally followed by
 * the tanh GELU (torch.nn.GELU(approximate="tanh") in fp32) - GPT-2's Conv1D, `addmm(bias, x, weight)` (hf
 * modeling_gpt2.py).  Every operand element is split into three bf16 values by round-to-nearest (hi + mid + lo == x) and
 * six of the nine products (mid.mid, lo.hi, hi.lo, mid.hi, hi.mid, hi.hi, in that order) go into one fp32 accumulator:
 * fp32-accurate at 6/16 of the fp32 MFMA's cycles.
 * W is split once per weight into a packed image of glb_gemm_split_bytes(k, n) bytes (6 per element; 0 when the shape is
 * not served: the build serves n % 128 == 0 and k % 64 == 0), rebuilt by the caller whenever W changes.  A row-major with
 * row pitch lda (elements; A and lda * 4 16-byte aligned), C row-major with pitch ldc, bias [n] or null.
 * Only A[0 .. m-1][0 .. k-1] is read and only C[0 .. m-1][0 .. n-1] written, whatever lda and ldc are; the bits of one
 * element of C depend on its row of A, its column of W and its bias alone - not on m, on the row's position or on the
 * other rows and columns (tests/test_split_gemm_exact_gpu.py).
 * Non-finite and out-of-range operands - this is NOT addmm's behaviour: an element of A or W that is NaN, +-inf, or finite
 * with |x| >= 0x1.ffp127 (3.3961775e38, +-FLT_MAX included: such a value rounds to a bf16 infinity and its residual is
 * inf - inf) makes every element of its row of C (an element of A) or of its column of C (an element of W) non-finite,
 * where addmm gives +-inf or, for the finite ones, a number.  Every other row and column keeps the bits of the call
 * without that element.  Finite |x| below that threshold are served as numbers.  Below 2^-109 the split is exact to
 * 2^-134 only (lo falls among bf16's subnormals).  A caller that needs IEEE results for such operands runs its library GEMM.
 * Argument errors return GLB_EINVAL before any GPU work, shapes and alignments the kernel does not serve
 * GLB_EUNSUPPORTED (the caller then runs its library GEMM).  Launches go on the given stream, allocate nothing and may be
 * captured into a hipGraph.
 */
enum { GLB_GEMM_BIAS = 0, GLB_GEMM_BIAS_GELU_TANH = 1 };
typedef struct glb_gemm_args {
  uint32_t struct_size; /* sizeof(glb_gemm_args) - ABI guard */
  int64_t m, n, k;
  const float *a;
  int64_t lda;
  const void *w_split; /* glb_gemm_split_weights' image of W */
  const float *bias;   /* [n], nullable */
  float *c;
  int64_t ldc;
  int32_t epilogue; /* GLB_GEMM_BIAS or GLB_GEMM_BIAS_GELU_TANH */
} glb_gemm_args;
size_t glb_gemm_split_bytes(int64_t k, int64_t n);
int glb_gemm_split_weights(const float *w, int64_t k, int64_t n, int64_t ldw, void *out, size_t out_bytes, void *hip_stream);
int glb_gemm_f32_split(const glb_gemm_args *args, void *hip_stream);
/* The kernel has two tile forms: 128 x 128 output tiles (large) and 64 x 64 (small: more blocks for launches whose large
 * tiles would leave CUs empty).  An element of C is the same chain of operations in both, so the bits of a call DO NOT
 * depend on the form (tests/test_split_gemm_forms_gpu.py); the choice is one of speed alone.
 * glb_gemm_split_pick: the form glb_gemm_f32_split runs for an (m, n, k) call on a device of n_cus CUs, into *form.  A
 * function of its arguments only - host code, no GPU work, callable on a machine without one - and monotone: once a row
 * count picks the large form, every larger one does (tests/test_split_gemm_pick_cpu.py).  GLB_EINVAL for a null pointer or
 * a non-positive argument.
 * glb_gemm_f32_split_form: glb_gemm_f32_split with the form forced; form 0 picks (exactly glb_gemm_f32_split), any value
 * other than 0 and the two constants returns GLB_EINVAL without a launch. */
enum { GLB_GEMM_FORM_LARGE = 1, GLB_GEMM_FORM_SMALL = 2 };
int glb_gemm_split_pick(int64_t m, int64_t n, int64_t k, int n_cus, int *form);
int glb_gemm_f32_split_form(const glb_gemm_args *args, int form, void *hip_stream);
/* The residual epilogue: C[row, col] = (acc + bias[col]) + R[row, col] - two separately rounded fp32 adds, the bias first -
 * with R = `residual`, fp32 [m, n] of row pitch ldr >= n, 4-byte aligned, memory of the current device.  The bits are those
 * of glb_gemm_f32_split followed by a float add of R in either operand order; a transformer block's `x + proj(h)` in one
 * launch and without the pass over [m, n] the add takes.  R is read under the store's guard: nothing outside its m x n
 * elements is read, and a non-finite element of R reaches its own element of C only.  C may be R itself (same pointer and
 * ldc == ldr: every element is read and written by one thread, in that order); any other overlap of the two, a null or
 * misaligned R, ldr < n, an R the current device does not own and an epilogue other than GLB_GEMM_BIAS return GLB_EINVAL
 * without a launch.  Every other check, `form` and the return codes are glb_gemm_f32_split_form's. */
int glb_gemm_f32_split_residual(const glb_gemm_args *args, const float *residual, int64_t ldr, int form, void *hip_stream);
/* How many blocks of the split GEMM's kernel (gelu != 0: the instantiation with the GELU epilogue) the runtime keeps resident
 * on one CU of the current device, given the kernel's registers and its dynamic LDS (hipOccupancyMaxActiveBlocksPerMultiprocessor).
 * The kernel is built for three; no GPU work.  This is the large form; glb_gemm_split_form_blocks_per_cu
 * reports either form's (the small one is built for six; a bad form: GLB_EINVAL). */
int glb_gemm_split_blocks_per_cu(int gelu, int *blocks);
int glb_gemm_split_form_blocks_per_cu(int form, int gelu, int *blocks);

/*
 * The plan of a row-packed encoding (kv.encode_packed): context u of the n_sel selected ones is prompt
 * grp[u] of n_groups prompts plus a tail of t_u = lengths[sel[u]] - group_lens[grp[u]] tokens; the packed batch holds the
 * prompts' n_pre rows once, then the tails in context order, M = n_pre + n_tail_rows rows (n_tail_rows: the CALLER's number,
 * nothing is read back).  Inputs, all device memory: the ragged batch tokens [n_tokens] / starts [n_contexts] / lengths
 * [n_contexts], sel and grp (their first n_sel entries), the prompts' group_starts / group_lens [n_groups],
 * group_segments [n_groups, 4], group_ids / group_pos [n_pre].  Outputs: segments int32 [n_groups + n_sel, 4] =
 * (pre_start, pre_len, tail_start, tail_len) with the prompts' rows first, ids and pos int64 [M] (pos clamped to
 * [0, pos_cap - 1]), last int64 [n_sel] (the row of every context's last token, clamped into [0, M - 1]); ends int32
 * [n_sel] is scratch (the tails' inclusive sums).  Two plain launches on the stream - one workgroup scans the tails, then a
 * thread per row finds its context by binary search - no workspace beyond these, no allocation, safe under stream capture.
 * Lengths that do not match n_tail_rows, tails < 1 and grp out of range are NOT errors here: every index is clamped into
 * range (grp into [0, n_groups - 1], a tail row's context into [0, n_sel - 1], its token's index into [0, n_tokens - 1],
 * sel read as an index from the end when negative and kept inside [0, n_contexts - 1]), int32 sums wrap, and
 * glb_short_attention_packed refuses the bad segments row by row.  GLB_EINVAL: null pointers, a size below 1,
 * n_tail_rows < n_sel, M or n_sel beyond INT32_MAX.
 */
typedef struct glb_packed_plan_args {
  uint32_t struct_size; /* sizeof(glb_packed_plan_args) - ABI guard */
  int64_t n_tokens, n_contexts, n_sel, n_groups, n_pre, n_tail_rows, pos_cap;
  const int32_t *tokens;
  const int64_t *starts;
  const int32_t *lengths;
  const int32_t *sel;
  const int32_t *grp;
  const int32_t *group_starts;
  const int32_t *group_lens;
  const int32_t *group_segments;
  const int64_t *group_ids;
  const int64_t *group_pos;
  int32_t *segments;
  int64_t *ids;
  int64_t *pos;
  int64_t *last;
  int32_t *ends;
} glb_packed_plan_args;
int glb_packed_plan(const glb_packed_plan_args *args, void *hip_stream);

/*
 * LoRA merge: out = W + scale * B . A for every matrix of an adapter in one call - what peft's merged
 * weights are (peft lora/layer.py get_delta_weight), made once per adapter switch so the forward runs the base model's
 * kernels.  Per job: W and out [n_out, k_in] (nn.Linear) or [k_in, n_out] (w_transposed: GPT-2's Conv1D, peft's
 * fan_in_fan_out), row pitches ldw / ldo; A = lora_A [r, k_in] (pitch lda), B = lora_B [n_out, r] (pitch ldb); all device
 * pointers aligned to their element.  Arithmetic contract, for every element (i output feature, j input feature):
 *     acc = +0.0f;  for t = 0 .. r-1 ascending: acc = fmaf(f32(B[i, t]), f32(A[t, j]), acc)
 *     out[i, j] = round_to_w_dtype(fmaf(scale, acc, f32(W[i, j])))      (round to nearest even)
 * f32() is exact for every element type; the bits depend on nothing else (no atomics, no launch-geometry dependence),
 * so the result is restated bit for bit on the CPU (tests/lora_engine.py).  r 1 .. 256 and any n_out, k_in >= 1 up to
 * 2^30 are served (GLB_EUNSUPPORTED otherwise).  No job's out may overlap any job's w, a or b, nor another job's out
(GLB_EINVAL: the blocks of one call run in any order).  The job table is copied into the
 * caller's device `workspace` (glb_lora_merge_workspace_bytes(n_jobs) bytes, 16-byte aligned) before the call returns;
 * argument errors return GLB_EINVAL before any GPU work.  One launch per W dtype among the jobs (split when its grid
exceeds 2^24 - 1 blocks), on the given stream;
 * not for stream capture (the table copy reads host memory).
 */
typedef struct glb_lora_job {
  uint32_t struct_size; /* sizeof(glb_lora_job) - ABI guard */
  int32_t w_dtype;      /* GLB_F32 / GLB_BF16 / GLB_F16: W and out */
  int32_t ab_dtype;     /* GLB_F32 / GLB_BF16 / GLB_F16: A and B */
  int32_t w_transposed; /* 0: W is [n_out, k_in] (nn.Linear); 1: W is [k_in, n_out] (GPT-2 Conv1D) */
  int64_t n_out, k_in, r;
  const void *w;
  int64_t ldw; /* row pitches in elements */
  const void *a;
  int64_t lda; /* lora_A [r, k_in] */
  const void *b;
  int64_t ldb; /* lora_B [n_out, r] */
  float scale;
  void *out;
  int64_t ldo; /* same dtype and layout as w */
} glb_lora_job;
size_t glb_lora_merge_workspace_bytes(int32_t n_jobs);
int glb_lora_merge(const glb_lora_job *jobs /* host */, int32_t n_jobs, void *workspace /* device */, size_t workspace_bytes,
                   void *hip_stream);

/*
 * LoRA per row: peft's unmerged form with the adapter chosen per row of one projection, in place on the
 * projection's output.  X [m, k] is the module's input, Y [m, n] its output (one dtype, GLB_F32 / GLB_BF16 / GLB_F16, row
 * pitches ldx / ldy in elements; ldy > n serves a column slice of a joint [q; k; v] or [gate; up] output):
 *     slot = row_slot[i]                (int32, device; negative: the base model)
 *     slot < 0, slot >= n_slots, or no entry for `module` in that slot: Y[i, :] is not written (its bits are untouched,
 *                                        as are the columns beyond n of every row)
 *     else  T[i, t] = sum_k A[t, k] * X[i, k];   Y[i, j] = round_to_y_dtype(fmaf(scale, sum_t B[j, t] * T[i, t], f32(Y[i, j])))
 * The table (device memory, glb_lora_rows_table_bytes bytes, 16-byte aligned) holds one entry per (slot, module), made from
 * a host array entries[slot * n_modules + module] by glb_lora_rows_table_upload when the set of adapters changes: A =
 * lora_A [r, k_in] (pitch lda), B = lora_B [n_out, r] (pitch ldb) in their stored dtype (independent of X's; slots may
 * differ in dtype and rank), r 1 .. 256, r == 0: the slot does not target the module.  At most 64 slots and 4096 modules
 * (GLB_EUNSUPPORTED beyond, as for r > 256).  An entry whose n_out / k_in are not the call's n / k, or whose rank exceeds
 * the call's r_max, leaves its rows untouched.
 * Numerics: both sums run on MFMA with float32 accumulation.  X and A / B of ONE 16-bit dtype: v_mfma_f32_16x16x32 of that
 * dtype, and T is rounded once to it (round to nearest even) between the two sums; every other combination widens the
 * operands to float32 (exact), runs v_mfma_f32_16x16x4_f32 and keeps T in float32.  k is summed in chunks of 32 dealt to
 * four partial sums (chunk c to sum c % 4, each ascending), added as ((s0 + s1) + s2) + s3; t ascending; one rounding of Y.
 * Row independence: the bits of row i depend on X[i, :], Y[i, :] and its slot's A, B and scale only - not on m, on other
 * rows' slots or values (rows of different slots may be in any order), or on replay from a hipGraph.  No atomics.
 * Alignment: x, y, a, b to their element, row_slot to 4 bytes, table and workspace to 16 bytes; 16-byte vector accesses
 * are used where a pointer and its pitch are multiples of 16 bytes and element accesses elsewhere, so every n, k >= 1 is
 * served.  x and y must not overlap.  `workspace`: glb_lora_rows_workspace_bytes(m, r_max) bytes of device memory (T).
 * Argument errors return GLB_EINVAL before any GPU work; glb_lora_rows launches twice on the given stream, allocates
 * nothing, reads no host memory besides its argument block and may be captured into a hipGraph (the upload may not: it
 * copies from host memory).
 */
typedef struct glb_lora_rows_entry {
  uint32_t struct_size; /* sizeof(glb_lora_rows_entry) - ABI guard */
  int32_t ab_dtype;     /* GLB_F32 / GLB_BF16 / GLB_F16: A and B */
  int64_t n_out, k_in, r; /* r == 0: absent (the other fields are ignored) */
  const void *a;
  int64_t lda; /* lora_A [r, k_in] */
  const void *b;
  int64_t ldb; /* lora_B [n_out, r] */
  float scale;
} glb_lora_rows_entry;
typedef struct glb_lora_rows_args {
  uint32_t struct_size; /* sizeof(glb_lora_rows_args) - ABI guard */
  int32_t dtype;        /* GLB_F32 / GLB_BF16 / GLB_F16: x and y */
  int64_t m, n, k;
  const void *x;
  int64_t ldx;
  void *y;
  int64_t ldy;
  const void *row_slot; /* int32 [m] */
  const void *table;    /* device table of glb_lora_rows_table_upload */
  int32_t n_slots, n_modules;
  int32_t module; /* which module of the table this projection is */
  int32_t r_max;  /* >= the rank of every entry that is to be applied; sizes the workspace */
  void *workspace;
  size_t workspace_bytes;
} glb_lora_rows_args;
size_t glb_lora_rows_table_bytes(int32_t n_slots, int32_t n_modules);
int glb_lora_rows_table_upload(const glb_lora_rows_entry *entries /* host */, int32_t n_slots, int32_t n_modules,
                               void *table /* device */, size_t table_bytes, void *hip_stream);
size_t glb_lora_rows_workspace_bytes(int64_t m, int32_t r_max);
int glb_lora_rows(const glb_lora_rows_args *args, void *hip_stream);

/*
 * 4-bit block-quantised weights: the block format bitsandbytes uses for Linear4bit, without double
 * quantisation.  A weight W[n, k] (nn.Linear layout; `transposed`: the memory holds W^T [k, n], GPT-2's Conv1D) is cut into
 * blocks of 64 consecutive elements along k; a block stores absmax = max |w| as float32 and 64 four-bit codes into a
 * 16-entry float32 codebook that the caller passes as data (`codebook`: HOST pointer, 16 finite floats, copied into the
 * launch; NF4 and FP4 are two tables).  Arithmetic contract, restated bit for bit in tests/quant4_engine.py:
 *     quantise:   sort the codebook ascending (c_0 .. c_15), m_i = (c_i + c_{i+1}) * 0.5f in float32; the code of w is the
 *                 sorted entry whose index is the number of float32 products m_i * absmax strictly below f32(w)
 *     dequantise: w' = codebook[code] * absmax, one float32 multiplication, then one round-to-nearest-even to the dtype
 * Weights must be finite.  glb_w4_bytes(n, k) = n k / 2 + 4 n k / 64 bytes of image (16-byte aligned), 0 for a shape that
 * is not served (k % 64 != 0, more than 2^34 elements); the order inside the image is private to the library
 * (glb_w4_dequantize inverts glb_w4_quantize).  `dtype` / `w` / `ldw` (row pitch in elements): the source of quantize,
 * the destination of dequantize.  glb_w4_gemm: Y[m, n] = X[m, k] . W'^T (+ bias), X, Y and bias of one 16-bit dtype
 * (GLB_BF16 / GLB_F16), rows of unit inner stride with pitches ldx / ldy, reading the image directly: codes are expanded
 * in registers to exactly glb_w4_dequantize's 16-bit element, multiplied on v_mfma_f32_16x16x32, summed in float32 -
 * K is split over workgroups by a rule that depends on (n, k) only, the slices are added in ascending order by a second
 * launch (no atomics: same bits every run) - and rounded once.  It is the few-row kernel: 1 <= m <=
 * glb_w4_gemm_max_rows(), n % 16 == 0, X and ldx 16-byte aligned; everything else returns GLB_EUNSUPPORTED (the caller
 * dequantises and runs its library GEMM).  `workspace`: glb_w4_gemm_workspace_bytes(m, n, k) bytes of device memory,
 * 16-byte aligned (0: the call is not served).  Argument errors return GLB_EINVAL before any GPU work; launches go on
 * the given stream, allocate nothing and may be captured into a hipGraph.
 * Containment (tests/test_w4_gemm_exact_gpu.py): only X[0 .. m-1][0 .. k-1] is read and only Y[0 .. m-1][0 .. n-1] written,
 * whatever ldx and ldy are; the bits of one element of Y depend on its row of X, its row of W' and its bias alone - not on
 * m (every row count runs the same additions in the same order), on the row's position or on the other rows and columns.
 * A NaN or an infinity in X makes only its own row of Y non-finite; a block whose W' is infinite in the 16-bit dtype (a
 * float32 absmax beyond the dtype's range) or zero touches only its own column; finite operands whose sum leaves the
 * dtype's range give +-inf as IEEE addition does.  A -0 of W' reaches Y as +0 (the sums start at +0).
 */
typedef struct glb_w4_args {
  uint32_t struct_size; /* sizeof(glb_w4_args) - ABI guard */
  int32_t dtype;        /* GLB_F32 / GLB_BF16 / GLB_F16 of w */
  int32_t transposed;   /* 0: w is [n, k]; 1: w is [k, n] */
  int64_t n, k;
  void *w; /* read by quantize, written by dequantize */
  int64_t ldw;
  const float *codebook; /* host, 16 entries */
  void *image;
  size_t image_bytes;
} glb_w4_args;
typedef struct glb_w4_gemm_args {
  uint32_t struct_size; /* sizeof(glb_w4_gemm_args) - ABI guard */
  int32_t dtype;        /* GLB_BF16 / GLB_F16: x, bias and y */
  int64_t m, n, k;
  const void *x;
  int64_t ldx;
  const void *image;
  const float *codebook; /* host, 16 entries */
  const void *bias;      /* [n], nullable */
  void *y;
  int64_t ldy;
  void *workspace;
  size_t workspace_bytes;
} glb_w4_gemm_args;
size_t glb_w4_bytes(int64_t n, int64_t k);
int glb_w4_quantize(const glb_w4_args *args, void *hip_stream);
int glb_w4_dequantize(const glb_w4_args *args, void *hip_stream);
int glb_w4_gemm_max_rows(void);
size_t glb_w4_gemm_workspace_bytes(int64_t m, int64_t n, int64_t k);
int glb_w4_gemm(const glb_w4_gemm_args *args, void *hip_stream);

/*
 * Byte-level DFA constraints: token masks made on the device from an automaton over bytes.
 * The automaton: `delta` int32 [n_states, 256] (-1: no transition), `accepting` / `live` one byte per state (live[s]: an
 * accepting state is reachable from s, s included - computed by the caller), `start`.  The vocabulary: the tokens' byte
 * strings back to back in `tok_bytes` [n_bytes], token t owning [tok_ptr[t], tok_ptr[t + 1]), and `skip` [vocab] (nonzero:
 * never allowed - special tokens).  next(s, t) = the state after walking t's bytes from s, or -1 (dead) when a transition
 * is missing, the state reached is not live, the token is empty, skipped or outside [0, vocab), or s < 0.  The mask of
 * state s (GLB_MASK_BITS layout): bit t = next(s, t) >= 0 for t != eos_id, bit eos_id = accepting[s], bits >= vocab zero.
 *
 * The mask bank: int32 [capacity, bank_ld] bit rows the fused step reads raw (mask_kind GLB_MASK_BITS, ids = rows).  Row 0
 * is all zeros (a dead particle), row 1 EOS only, rows 2 .. hold one state each: row_of_state [n_states] (-1: none yet),
 * `work` [capacity] pairs (state, row) in the order rows were claimed, `counters` [GLB_DFA_COUNTERS] int32:
 *   [0] rows in use   [1] work entries filled so far   [2] overflow (sticky)   [3] reserved
 *   glb_dfa_bank_init   rows 0 and 1, row_of_state = -1, counters = {2, 0, 0, 0}
 *   glb_dfa_advance     state_out[i] = the state after tokens[i, from[i] .. to[i]) of the int32 [n, ld] matrix, starting at
 *                       state_in[i] (null: `start` for everybody); -1 once dead; from == to copies; a range outside
 *                       [0, ld] or a state outside [0, n_states) gives -1.  state_out may be state_in.
 *   glb_dfa_claim_rows  every state of state_in [n] without a row gets the next one (vector atomics on row_of_state and
 *                       counters[0]; one row per distinct state) and an entry in `work`.  Beyond `capacity`: nothing is
 *                       written, counters[2] = 1.  Which state gets which row depends on the atomics' order; a row's bits
 *                       do not.
 *   glb_dfa_fill_masks  writes the mask rows of the work entries [counters[1], counters[0] - 2) - words 0 ..
 *                       ceil(vocab / 32) - 1 of each row, nothing else - and moves counters[1] up (a second, one-thread launch).  The grid is sized by
 *                       `max_work` (an upper bound of the entries waiting; more are served, only slower).
 *   glb_dfa_mask_ids    out_rows[i] = the bank row of state_in[i]: 0 for a dead state or one without a row; where done[i]
 *                       (nullable) is nonzero, 1 if the state is accepting and 0 otherwise.
 *   glb_dfa_bank_rows   host: rows of a bank of `bank_bytes` for this vocabulary, at most n_states + 2 and 65535.
 * Every index read from device memory (states, tokens, byte offsets, rows) is range-checked: bad input gives dead / no
 * write, never an access out of bounds.  Argument errors return GLB_EINVAL before any GPU work; launches go on the given
 * stream, allocate nothing, never synchronise.  Calls that share a bank must be ordered on one stream.
 */
#define GLB_DFA_COUNTERS 4
typedef struct glb_dfa_args {
  uint32_t struct_size; /* sizeof(glb_dfa_args) - ABI guard */
  int32_t n_states, start, eos_id;
  const int32_t *delta;     /* [n_states, 256] */
  const uint8_t *accepting; /* [n_states] */
  const uint8_t *live;      /* [n_states] */
  int64_t vocab;
  const uint8_t *tok_bytes; /* [n_bytes] */
  int64_t n_bytes;
  const int32_t *tok_ptr; /* [vocab + 1] */
  const uint8_t *skip;    /* [vocab] */
  /* advance / claim_rows / mask_ids: n particles */
  int64_t n;
  const int32_t *tokens; /* [n, ld] */
  int64_t ld;
  const int32_t *from, *to; /* [n] */
  const int32_t *state_in;  /* [n]; advance: nullable */
  int32_t *state_out;       /* [n] */
  /* the bank */
  int32_t *bank; /* [capacity, bank_ld] */
  int64_t bank_ld, capacity;
  int32_t *row_of_state; /* [n_states] */
  int32_t *work;         /* [capacity, 2] */
  int32_t *counters;     /* [GLB_DFA_COUNTERS] */
  int64_t max_work;
  const int32_t *done; /* [n], nullable */
  int32_t *out_rows;   /* [n] */
} glb_dfa_args;
int glb_dfa_bank_init(const glb_dfa_args *args, void *hip_stream);
int glb_dfa_advance(const glb_dfa_args *args, void *hip_stream);
int glb_dfa_claim_rows(const glb_dfa_args *args, void *hip_stream);
int glb_dfa_fill_masks(const glb_dfa_args *args, void *hip_stream);
int glb_dfa_mask_ids(const glb_dfa_args *args, void *hip_stream);
int64_t glb_dfa_bank_rows(size_t bank_bytes, int64_t vocab, int64_t n_states);

/*
 * Weighted byte automata: the same deterministic automaton in the log semiring - `arc_logw` float32
 * [n_states, 256] beside `delta`, `final_logw` float32 [n_states] (-inf: not accepting; accepting[s] = final_logw[s] >
 * -inf, and an arc of weight -inf is no arc: the caller removes both before it computes `live`).  A state's row is a row
 * of float log-weights the fused step adds to the log-probabilities (mask_kind GLB_MASK_F32, ids = rows).  Row of state s:
 *   column t != eos_id   walk t's bytes exactly as next(s, t) above does, with w = 0.0f; w = w + arc_logw[cur][b] in
 *                        float32, in byte order, cur the state the byte is read in; the column is w if next(s, t) >= 0 and
 *                        -inf otherwise (a token is dead by the same rules: empty, skipped, a missing arc, a destination
 *                        that is not live)
 *   column eos_id        final_logw[s]
 *   columns [vocab, wbank_ld)  never written
 * The sum is one fixed chain of float32 additions (no fused multiply-add to contract, no reassociation): rows are exact
 * against the same chain on a host.  The weight bank: float32 [dfa.capacity, wbank_ld] in place of the bit bank; row 0 all
 * -inf, row 1 -inf except 0.0f at eos_id (a particle forced to end: its final weight is the caller's to add), rows 2 ..
 * one state each.  States, row_of_state, work, counters and the overflow word are the machinery above and
 * glb_dfa_advance / glb_dfa_claim_rows / glb_dfa_mask_ids serve a weight bank unchanged (they never touch `bank`; give
 * them any non-null pointer and bank_ld >= ceil(vocab / 32)).  In the embedded block `dfa.bank` and `dfa.bank_ld` are not
 * read by the calls below.
 *   glb_dfa_weight_bank_init  rows 0 and 1 of wbank, row_of_state = -1, counters = {2, 0, 0, 0}
 *   glb_dfa_fill_weights      the rows of the work entries [counters[1], counters[0] - 2), columns 0 .. vocab - 1, and moves
 *                             counters[1] up, as glb_dfa_fill_masks does; grid sized by dfa.max_work
 *   glb_dfa_weight_bank_rows  host: rows of a bank of `bank_bytes` whose rows are `vocab` floats padded to a multiple of 64
 *                             (256-byte rows: a wave's store is one aligned line), at most n_states + 2 and 65535
 * GLB_EINVAL before any launch: struct_size of either block wrong, wbank_ld < vocab, a null table; the same range checks
 * of indices read from device memory; launches allocate nothing and may be captured.
 */
typedef struct glb_dfa_weight_args {
  uint32_t struct_size; /* sizeof(glb_dfa_weight_args) - ABI guard */
  glb_dfa_args dfa;     /* its own struct_size set too */
  const float *arc_logw;   /* [n_states, 256] */
  const float *final_logw; /* [n_states] */
  float *wbank;            /* [dfa.capacity, wbank_ld] */
  int64_t wbank_ld;
} glb_dfa_weight_args;
int glb_dfa_weight_bank_init(const glb_dfa_weight_args *args, void *hip_stream);
int glb_dfa_fill_weights(const glb_dfa_weight_args *args, void *hip_stream);
int64_t glb_dfa_weight_bank_rows(size_t bank_bytes, int64_t vocab, int64_t n_states);

/*
 * A bank smaller than the automaton: the bank as a cache over the states, least recently used rows
 * recycled on the device.  The block embeds glb_dfa_args, its own struct_size set too, and serves either kind of bank:
 * `wbank` null - the bit bank dfa.bank / dfa.bank_ld; `wbank` set - the float bank, its four fields those of
 * glb_dfa_weight_args: arc_logw, final_logw, wbank, wbank_ld; dfa.bank is then not read.  Beside row_of_state:
 *   row_state [capacity]   the state that owns each row, -1: none (rows 0 and 1: always -1)
 *   row_stamp [capacity]   the epoch of the serve call that last requested the row; 0: never used
 *   claimants [capacity]   the distinct states of the running call that have no row, in the atomics' order
 *   victims   [capacity]   the rows taken for them
 *   ecounters [GLB_DFA_EVICT_COUNTERS]  [0] claimants of the running call  [1] rows taken by it (both zero between calls)
 *                          [2] rows filled, cumulative  [3] of these, rows that were taken from another state, cumulative
 *   epoch [1]              the number of the running call, from 1; advanced on the device, never read by the host
 * dfa.counters keeps its meaning: [0] rows in use (2 + rows that own a state), [2] overflow (sticky); [1] and `work`'s
 * order are the claim path's and are not used: `work` holds the running call's (state, row) pairs from entry 0.
 *   glb_dfa_evict_bank_init  what glb_dfa_bank_init / glb_dfa_weight_bank_init do, and row_state = -1, row_stamp = 0,
 *                            ecounters = 0, epoch = 1
 *   glb_dfa_evict_serve      gives every state of dfa.state_in [n] a filled row and writes dfa.out_rows [n]; in stream order:
 *     1 touch     every state of state_in that has a row: row_stamp[row] = epoch.  Each distinct state without one wins
 *                 the CAS election on row_of_state (-1 -> -2) exactly once and is appended to `claimants`.
 *     2 select    one workgroup; leaves at once when there are no claimants.  The candidates are the rows of [2, capacity)
 *                 whose stamp is not the epoch - a row requested in this call is never taken.  take = min(claimants,
 *                 candidates) rows are chosen in ascending order of stamp (an exact radix select over the 32-bit stamps;
 *                 never-used rows, stamp 0, go first; ties break in any order) into `victims`.
 *     3 reassign  (same launch) claimant j < take gets victims[j]: the row's old state loses it (row_of_state[old] = -1),
 *                 row_state, row_of_state, row_stamp = epoch and work entry j are written.  Claimants j >= take get
 *                 nothing: row_of_state back to -1, counters[2] = 1, nothing else written for them.
 *     4 fill      work entries [0, take) by the fill of glb_dfa_fill_masks / glb_dfa_fill_weights (grid sized by
 *                 dfa.max_work)
 *     5 ids       out_rows as glb_dfa_mask_ids writes them (`done` included); a state left without a row gets 0
 *     6 epoch     epoch += 1 (it stops at 2^31 - 1: from then on no row is a candidate and every claimant overflows),
 *                 ecounters[0] = ecounters[1] = 0
 * Row ids are valid until the next serve call on the bank (stream order).  Which state gets which row depends on the
 * atomics' order; which rows may be taken, how many, and every row's contents do not.  GLB_EINVAL before any launch,
 * buffers untouched: struct_size of either block wrong, a null table, capacity < 3, a float bank with wbank_ld < vocab or
 * one of its tables null, and what glb_dfa_mask_ids / glb_dfa_fill_masks refuse.  Every index read from device memory
 * (states, rows, list entries, counts) is range-checked; nothing synchronises or allocates; the launches may be captured.
 */
#define GLB_DFA_EVICT_COUNTERS 4
typedef struct glb_dfa_evict_args {
  uint32_t struct_size; /* sizeof(glb_dfa_evict_args) - ABI guard */
  glb_dfa_args dfa;     /* its own struct_size set too */
  const float *arc_logw;   /* [n_states, 256]; a bit bank: null */
  const float *final_logw; /* [n_states]; a bit bank: null */
  float *wbank;            /* [dfa.capacity, wbank_ld]; a bit bank: null */
  int64_t wbank_ld;
  int32_t *row_state; /* [capacity] */
  int32_t *row_stamp; /* [capacity] */
  int32_t *claimants; /* [capacity] */
  int32_t *victims;   /* [capacity] */
  int32_t *ecounters; /* [GLB_DFA_EVICT_COUNTERS] */
  int32_t *epoch;     /* [1] */
} glb_dfa_evict_args;
int glb_dfa_evict_bank_init(const glb_dfa_evict_args *args, void *hip_stream);
int glb_dfa_evict_serve(const glb_dfa_evict_args *args, void *hip_stream);

/*
 * Weight pushing: the backward weights of a weighted byte automaton and the automaton reweighted by them,
 * made on the device.  beta[s] is the semiring sum of the weights of all accepted byte strings from s - the weighted form
 * of `live` - and the pushed automaton
 *   arc_out[s][b] = (arc_logw[s][b] + beta[delta[s][b]]) - beta[s]      final_out[s] = final_logw[s] - beta[s]
 * (float32, in this order; everything of a state with beta[s] = -inf is -inf, and so is an arc delta does not have: -1 or
 * a destination outside [0, n_states)) weighs every accepted string what it weighed minus beta[start], with the look-ahead
 * in every state's row: under GLB_DFA_PUSH_LOG a live state's arcs and final weight sum to one, under GLB_DFA_PUSH_MAX
 * their maximum is 0.  The block stands alone: no vocabulary, bank or work list.
 *   glb_dfa_backward      `restart` != 0: beta = final_logw and status = 0 first.  Then `sweeps` launches, launch j reading
 *                         beta_k from `beta` (j even) or `scratch` (j odd) and writing beta_{k+1} to the other - never in
 *                         place:   beta_{k+1}[s] = final_logw[s] (+) (+)_b (arc_logw[s][b] + beta_k[delta[s][b]])
 *                         (+) = max under MAX; under LOG m + log(sum exp(x - m)), m the maximum of the 257 terms, the sum in
 *                         one fixed order (a lane's four bytes l, l + 64, l + 128, l + 192 pairwise, a butterfly over the
 *                         64 lanes, the final weight's term last); m = -inf gives exactly -inf.  A result depends on the
 *                         inputs alone.  A sweep is marked changed when some state moved: new != old under MAX; under LOG
 *                         |new - old| > tol * max(1, |new|) (-inf to -inf: no change).  The launch after a sweep that did
 *                         not change leaves at once, and so does every later one of the call and of later calls without
 *                         `restart`.  The call's last launch copies `scratch` to `beta` when the last sweep performed wrote
 *                         there, so `beta` holds the result whenever a call's work is done, and writes status:
 *                           [0] sweeps performed since the restart   [1] converged: the last sweep performed did not change
 *                           [2] flags, sticky: bit 0 - some sweep produced +inf or NaN (the weights do not sum)
 *                           [3] sweeps performed by the last call    [4 .. 6] the sweeps' marks, zero between calls   [7] unused
 *                         Marks are plain stores of 1 by the waves that saw a change, into three rotating words; nothing
 *                         is counted with atomics.  A block never restarted has no meaning: the first call sets `restart`.
 *   glb_dfa_push_weights  arc_out / final_out from `beta` by the formulas above (scratch and status are not touched).
 * GLB_EINVAL before any launch, buffers untouched, for both calls: struct_size wrong, n_states < 1, start outside
 * [0, n_states), an unknown semiring, sweeps < 1, tol negative or NaN, and a null table among those the call uses (backward:
 * delta, arc_logw, final_logw, beta, scratch, status; push_weights: delta, arc_logw, final_logw, beta, arc_out, final_out).
 * Every destination read from `delta` is range-checked; nothing synchronises or allocates: the host reads `status` between
 * calls.
 */
#define GLB_DFA_PUSH_STATUS 8
#define GLB_DFA_PUSH_LOG 0
#define GLB_DFA_PUSH_MAX 1
typedef struct glb_dfa_push_args {
  uint32_t struct_size; /* sizeof(glb_dfa_push_args) - ABI guard */
  int32_t n_states, start;
  int32_t semiring;        /* GLB_DFA_PUSH_LOG / GLB_DFA_PUSH_MAX */
  const int32_t *delta;    /* [n_states, 256] */
  const float *arc_logw;   /* [n_states, 256] */
  const float *final_logw; /* [n_states] */
  float *beta;             /* [n_states], out */
  float *scratch;          /* [n_states] */
  float *arc_out;          /* [n_states, 256] */
  float *final_out;        /* [n_states] */
  int32_t *status;         /* [GLB_DFA_PUSH_STATUS] */
  int32_t sweeps;          /* launches of this call */
  int32_t restart;
  float tol;
} glb_dfa_push_args;
int glb_dfa_backward(const glb_dfa_push_args *args, void *hip_stream);
int glb_dfa_push_weights(const glb_dfa_push_args *args, void *hip_stream);

/*
 * Minimisation: the coarsest partition of an automaton's states that its labels allow, found on the device
 * by Moore's refinement, and the quotient automaton.  The block stands alone: no vocabulary, bank or work list.  `keep` says
 * which states take part (a host passes live & reachable).  An arc (s, b) is PRESENT when 0 <= delta[s][b] < n_states and
 * keep[delta[s][b]]; every other arc is absent, whatever arc_bits holds there.  The result: cls[s] = -1 where !keep[s]; over
 * the kept states `cls` is the coarsest partition in which the states of one class
 *   - have equal final_bits,
 *   - agree for every byte on whether the arc is present, and their present arcs lead into one class,
 *   - and, when arc_bits is given, carry equal arc_bits on their present arcs;
 * a class's id is its smallest member.  That partition is unique, so `cls` is one well-defined array.  Labels are compared
 * as bit patterns: with final_bits / arc_bits the bits of a weighted automaton's float32 final_logw / arc_logw this is the
 * coarsest bisimulation on (byte, weight bits), and the quotient by it leaves the weight of every path unchanged bit for
 * bit - the same floats are added in the same order.  After weight pushing (above) it merges what weighted minimisation
 * merges wherever rounding left equal bits; weights that differ in their last bit are different labels - nothing is merged
 * within a tolerance.  An unweighted automaton: final_bits = accepting, arc_bits null.
 *   glb_dfa_refine    `restart` != 0: first the classes by final_bits into `cls` and status = 0, status[3] their number.  Then
 *                     `rounds` rounds, round j of the call reading the classes from `cls` (j even) or `scratch` (j odd) and
 *                     writing the refined ones to the other - never in place.  A round is three launches: the table is
 *                     cleared (a launch of its own); every kept state's signature - its class, the class behind each
 *                     byte (-1: absent) and the arcs' bits - is hashed to 64 bits and the hash entered into `table` (open
 *                     addressing; a 64-bit compare-and-swap on the key, an atomic minimum on the member); every state
 *                     looks its hash up, compares its signature with the elected member's element by element and takes the
 *                     member as its class.  A difference there is a hash collision: it sets flag bit 0 and the state stays
 *                     a class of its own - never a silent merge.  Refinement only splits, so a round that leaves the
 *                     number of classes as it was has changed nothing: it sets the converged word, and every later launch
 *                     of the call and of later calls without `restart` leaves at once.  The call's last launch copies
 *                     `scratch` to `cls` when the last round performed wrote there, and writes status:
 *                       [0] rounds performed since the restart, the one that found nothing to split included
 *                       [1] converged   [2] flags, sticky: bit 0 - a hash collision; bit 1 - a key without a slot
 *                       [3] classes after the last round performed
 *                       [4 .. 6] the rounds' class counts, rotating, zero between calls   [7] rounds performed by the last call
 *                     The result does not depend on the order the atomics take: a launch ends with the same set of keys,
 *                     each with the smallest of its states.  `table`: 12 bytes a slot (table_slots 64-bit keys, then
 *                     table_slots int32 members), aligned to 8; its contents mean nothing between calls.
 *   glb_dfa_quotient  row j of the outputs, j < n_new, is the row of state rep[j] relabelled: delta_out[j][b] =
 *                     new_id[delta[rep[j]][b]] where that arc is present and the id lies in [0, n_new), else -1; arc_out
 *                     the arc's arc_logw there, else -inf; final_out[j] = final_logw[rep[j]], accepting_out[j] =
 *                     accepting[rep[j]].  arc_out / final_out / accepting_out may each be null (then its input may be too).
 *                     A rep[j] outside [0, n_states) gives a row without arcs, -inf and 0.  `cls` is not read: the host
 *                     derives new_id (every state's quotient state, -1 where dropped) and rep from it.
 * GLB_EINVAL before any launch, buffers untouched, the field named in the message: struct_size wrong, n_states < 1, delta or
 * keep null; refine: rounds outside [1, 65536], table_slots not a power of two or below 2 n_states, final_bits, cls, scratch,
 * table or status null; quotient: n_new outside [1, n_states], new_id, rep or delta_out null, an output without its input.
 * Every index read from device memory is range-checked; nothing synchronises or allocates: the host reads `status` between
 * calls.
 */
#define GLB_DFA_MIN_STATUS 8
typedef struct glb_dfa_min_args {
  uint32_t struct_size; /* sizeof(glb_dfa_min_args) - ABI guard */
  int32_t n_states;
  const int32_t *delta;       /* [n_states, 256] */
  const uint8_t *keep;        /* [n_states] */
  const uint32_t *final_bits; /* [n_states] */
  const uint32_t *arc_bits;   /* [n_states, 256]; unweighted: null */
  int32_t *cls;               /* [n_states], out */
  int32_t *scratch;           /* [n_states] */
  void *table;                /* 12 * table_slots bytes */
  int64_t table_slots;        /* a power of two >= 2 * n_states */
  int32_t *status;            /* [GLB_DFA_MIN_STATUS] */
  int32_t rounds;             /* rounds of this call */
  int32_t restart;
  /* glb_dfa_quotient */
  const int32_t *new_id;      /* [n_states] */
  const int32_t *rep;         /* [n_new] */
  int32_t n_new;
  const float *arc_logw;      /* [n_states, 256] or null */
  const float *final_logw;    /* [n_states] or null */
  const uint8_t *accepting;   /* [n_states] or null */
  int32_t *delta_out;         /* [n_new, 256] */
  float *arc_out;             /* [n_new, 256] or null */
  float *final_out;           /* [n_new] or null */
  uint8_t *accepting_out;     /* [n_new] or null */
} glb_dfa_min_args;
int glb_dfa_refine(const glb_dfa_min_args *args, void *hip_stream);
int glb_dfa_quotient(const glb_dfa_min_args *args, void *hip_stream);

/*
 * Products: the automaton of the strings that two byte automata A and B both accept (GLB_FSA_AND), that
 * either accepts (GLB_FSA_OR) or that A accepts and B does not (GLB_FSA_SUB), found by a breadth-first search over the pairs
 * of states.  A component of a pair is OUT, and stored as -1, when it is -1, outside its automaton or not live there.  Under
 * AND a pair with a side out does not exist; under SUB a pair with the A side out; under OR a pair with both sides out.
 * State 0 is the start pair - (-1, -1), without arcs, where that pair does not exist - and the states are numbered in the
 * order in which a queue search meets them that takes the states in id order and the bytes 0 .. 255 in ascending order.
 * The numbering does not depend on the order the atomics take: a new pair's slot in `table` (open addressing on the full
 * 64-bit key (a + 1) (n_b + 1) + (b + 1): equal keys are equal pairs) keeps the smallest arc index, frontier position * 256
 * + byte, of the round that found it, and a scan over the round's winning arcs hands out the ids.  State s accepts where
 * both sides do (AND), either does (OR), A's does and B's does not (SUB); a side that is out never accepts.
 * Weights: arc_a / final_a and arc_b / final_b are null for an unweighted operand; OR takes none, SUB takes A's alone.  An
 * arc of the product weighs arc_a + arc_b where both are given (one float32 addition, in that order), else the one given;
 * an arc that does not exist weighs -inf.  final_out likewise, -inf where the state does not accept.  arc_out / final_out
 * are given exactly when an operand has weights.
 *   glb_fsa_product_round  `restart` != 0: first the table emptied, status = 0 and state 0 made.  Then `rounds` rounds, six
 *                     launches each, every grid sized to the device and striding over the frontier that the status words
 *                     bound: every arc of the frontier expanded (delta_out, arc_out; the state's accepting_out and
 *                     final_out), the winning arcs counted a state, the counts scanned, the new states numbered (`pairs`),
 *                     delta_out's arcs into them resolved, the frontier moved on.  A round that numbers no state sets the
 *                     converged word; with it or a flag set every later launch leaves at once.  status:
 *                       [0] rounds performed since the restart   [1] converged
 *                       [2] flags, sticky: bit 0 - more than max_states states (nothing of that round is numbered);
 *                           bit 1 - an id out of range: a bug, never an input
 *                       [3] states numbered   [4], [5] the frontier   [6] private
 *                       [7] with flag bit 0: the pairs found when the search stopped, more than max_states
 *                       [12] private: the distinct pairs entered into the table, state 0 included
 *                     The expansion counts the new pairs as it enters them, so bit 0 goes up in the MIDDLE of the launch that
 *                     passes max_states; its blocks leave at their next state and its probes within 32 slots.  A round of
 *                     a wide frontier can bring 256 new pairs a state - many times the table - and neither fills it nor
 *                     probes a full table arc by arc.  Should the table fill before the flag is seen, that is bit 0 as well
 *                     (table_slots >= 2 max_states distinct pairs are more than max_states), [7] = table_slots.  One
 *                     below the true count, [7] is the true count; further below it is whatever the launch had entered.
 *                     `table`: 16 bytes a slot (table_slots 64-bit keys, then int32 arc indices, then int32 ids), aligned
 *                     to 8.  `counts`: max_states int32 of scratch.  max_states <= 2^22.
 *   glb_fsa_live      over the first n_states rows of delta_out: `restart` != 0: live = accepting_out and status[8 .. 11] =
 *                     0.  Then `rounds` sweeps of live[s] |= any live[delta_out[s][b]], in place (the rule only adds: the
 *                     fixed point is unique), two launches each.  status [8] sweeps performed, the one that changed nothing
 *                     included   [9] converged   [10] zero   [11] private.  Reads n_states, max_states, delta_out,
 *                     accepting_out, live, status, rounds, restart alone.
 * GLB_EINVAL before any launch, buffers untouched, the field named in the message: struct_size wrong, max_states outside
 * [1, 2^22], rounds outside [1, 65536], delta_out, accepting_out or status null; round: op unknown, n_a / n_b < 1, a start
 * outside its automaton, an operand's delta, accepting or live null, arc without final, weights the op does not take,
 * arc_out / final_out not matching them, table_slots not a power of two or below 2 max_states, table, pairs or counts null;
 * live: n_states outside [1, max_states], live null.  Nothing synchronises or allocates: the host reads `status`.
 */
#define GLB_FSA_STATUS 16
#define GLB_FSA_AND 0
#define GLB_FSA_OR 1
#define GLB_FSA_SUB 2
typedef struct glb_fsa_product_args {
  uint32_t struct_size; /* sizeof(glb_fsa_product_args) - ABI guard */
  int32_t op;
  int32_t n_a, n_b, start_a, start_b;
  const int32_t *delta_a, *delta_b;       /* [n, 256] */
  const uint8_t *accepting_a, *accepting_b; /* [n] */
  const uint8_t *live_a, *live_b;         /* [n] */
  const float *arc_a, *final_a;           /* [n_a, 256], [n_a] or both null */
  const float *arc_b, *final_b;           /* [n_b, 256], [n_b] or both null */
  int32_t max_states;
  int32_t n_states;                       /* glb_fsa_live: the states numbered */
  void *table;                            /* 16 * table_slots bytes */
  int64_t table_slots;                    /* a power of two >= 2 * max_states */
  int32_t *pairs;                         /* [max_states, 2], out */
  int32_t *delta_out;                     /* [max_states, 256], out */
  uint8_t *accepting_out;                 /* [max_states], out */
  float *arc_out;                         /* [max_states, 256], out, or null */
  float *final_out;                       /* [max_states], out, or null */
  uint8_t *live;                          /* [max_states], out (glb_fsa_live) */
  int32_t *counts;                        /* [max_states] */
  int32_t *status;                        /* [GLB_FSA_STATUS] */
  int32_t rounds;                         /* rounds / sweeps of this call */
  int32_t restart;
} glb_fsa_product_args;
int glb_fsa_product_round(const glb_fsa_product_args *args, void *hip_stream);
int glb_fsa_live(const glb_fsa_product_args *args, void *hip_stream);

/*
 * Determinisation: the deterministic automaton of a byte NFA with empty arcs, by the subset construction.
 * The NFA: n_states states, `start`; empty arcs as a CSR by source (eps_off [n_states + 1], eps_to [n_eps]); byte arcs as a
 * CSR by source over the IMPORTANT states (arc_off [n_important + 1], arc_dst [n_arcs], arc_bytes [n_arcs][4]: bit b of the
 * 256 is set where the arc reads byte b).  A state is important when it has a byte arc or accepts; bit_of [n_states] gives an
 * important state its bit index in [0, n_important) and every other state -1, accepting_mask [n_words] has the bits of the
 * accepting states.  A state of the result is the set of important states inside the empty-arc closure of what was reached,
 * a bitset of n_words = max(1, ceil(n_important / 64)) 64-bit words, n_important <= GLB_NFA_MAX_IMPORTANT: a wave holds a set,
 * a lane a word.  State 0 is the closure of `start` (it may be empty: a state without arcs).  The empty set is no other
 * state: an arc into it is -1.  A state accepts where its set holds an accepting state.  The states are numbered in the order
 * in which a queue search first meets the sets, states in id order and bytes 0 .. 255 ascending, whatever order the atomics
 * take.  Bytes that no arc's set tells apart form a GROUP (group_of [256], int32; group_lo [n_groups], the lowest byte of
 * every group, ascending): the search expands a group once, at its lowest byte, and writes delta_out for all its bytes.
 *   glb_nfa_closure       `restart` != 0: eclose [n_states][n_words] = every important state's own bit, status[8 .. 11] = 0.
 *                     Then `rounds` sweeps of eclose[v] |= eclose[u] over the empty arcs v -> u, in place (the rule only
 *                     adds: the fixed point is unique), two launches each.  status [8] sweeps performed, the one that
 *                     changed nothing included   [9] converged   [10] zero   [11] private.  Reads n_states, start,
 *                     n_important, n_words, n_eps, eps_off, eps_to, bit_of, eclose, status, rounds, restart alone.
 *   glb_nfa_subset_round  over a converged eclose.  `restart` != 0: the table emptied, status[0 .. 7] and [12 ..] = 0, state 0
 *                     made.  Then `rounds` rounds, seven launches each, every grid sized to the device and striding over
 *                     the states the status words bound; a round takes the next `chunk` states of the queue: the target
 *                     set of every (state, group) written to `cand` [chunk][n_groups][n_words]; every target entered into
 *                     `table`; the arcs that are first to a new set counted a state, the counts scanned, the new states
 *                     numbered (`sets` [max_states][n_words], accepting_out), delta_out's arcs into them resolved, the
 *                     queue moved on.  A round that finds the queue empty behind it sets the converged word; with it or a
 *                     flag set every later launch leaves at once.  status:
 *                       [0] rounds performed since the restart   [1] converged
 *                       [2] flags, sticky: bit 0 - more than max_states states (nothing of that round is numbered);
 *                           bit 1 - a reference or an id out of range: a bug, never an input
 *                       [3] states numbered   [4], [5] the states of the round   [6] private
 *                       [7] with flag bit 0: the sets found when the search stopped, more than max_states
 *                       [12] private: the distinct sets entered into the table, state 0 included
 *                     Bit 0 goes up in the middle of the launch that enters the set past max_states, and that launch
 *                     drains: its waves leave at their next target and their probes within 32 slots.
 *                     `table`: 12 bytes a slot (table_slots 64-bit words, then int32 arc indices), aligned to 8.  A slot's
 *                     word holds no set: 31 bits of the set's hash and a reference, the arc index (queue position in the
 *                     round * 256 + the group's lowest byte) that claimed it in this round - the set is that arc's row of
 *                     `cand` - or the id of a numbered state - the set is its row of `sets`.  An equal hash is followed by
 *                     a compare of the sets, unequal sets probe on.  hash_mask != 0 is ANDed onto the 64-bit hash before
 *                     it is used (a test's way of making nearly all sets collide: the arrays must not change).
 *                     `counts`: `chunk` int32 of scratch.  max_states <= 2^22, chunk in [1, max_states].
 * GLB_EINVAL before any launch, buffers untouched, the field named in the message: struct_size wrong, n_states outside
 * [1, 2^24], n_important outside [0, min(n_states, GLB_NFA_MAX_IMPORTANT)], n_words not what n_important gives, start outside
 * the automaton, rounds outside [1, 65536], eclose or status null; closure: n_eps negative, eps_off, eps_to or bit_of null;
 * round: n_arcs negative, n_groups outside [1, 256], max_states or chunk out of range, an arc, mask or group table null,
 * table_slots not a power of two or below 2 max_states, table, cand, sets, delta_out, accepting_out or counts null.  Nothing
 * synchronises or allocates: the host reads `status`.  Liveness of the result: glb_fsa_live over delta_out / accepting_out.
 */
#define GLB_NFA_STATUS 16
#define GLB_NFA_MAX_IMPORTANT 4096
typedef struct glb_nfa_args {
  uint32_t struct_size; /* sizeof(glb_nfa_args) - ABI guard */
  int32_t n_states, start;
  int32_t n_important, n_words;
  int32_t n_arcs, n_eps, n_groups;
  const int32_t *eps_off, *eps_to;        /* [n_states + 1], [n_eps] */
  const int32_t *bit_of;                  /* [n_states] */
  const int32_t *arc_off, *arc_dst;       /* [n_important + 1], [n_arcs] */
  const uint64_t *arc_bytes;              /* [n_arcs][4] */
  const uint64_t *accepting_mask;         /* [n_words] */
  const int32_t *group_of, *group_lo;     /* [256], [n_groups] */
  uint64_t *eclose;                       /* [n_states][n_words] */
  uint64_t hash_mask;                     /* 0: every bit of the hash */
  int32_t max_states;
  int32_t chunk;                          /* states of the queue a round takes */
  void *table;                            /* 12 * table_slots bytes */
  int64_t table_slots;                    /* a power of two >= 2 * max_states */
  uint64_t *cand;                         /* [chunk][n_groups][n_words] */
  uint64_t *sets;                         /* [max_states][n_words], out */
  int32_t *delta_out;                     /* [max_states, 256], out */
  uint8_t *accepting_out;                 /* [max_states], out */
  int32_t *counts;                        /* [chunk] */
  int32_t *status;                        /* [GLB_NFA_STATUS] */
  int32_t rounds;                         /* sweeps / rounds of this call */
  int32_t restart;
} glb_nfa_args;
int glb_nfa_closure(const glb_nfa_args *args, void *hip_stream);
int glb_nfa_subset_round(const glb_nfa_args *args, void *hip_stream);

/*
 * Lazy determinisation: a byte NFA served as a constraint, its subset states made on the device when a
 * particle reaches them.  The NFA arrays are those of glb_nfa_args - arc_off, arc_dst, arc_bytes, accepting_mask, n_important,
 * n_words = W - and `eclose` a converged closure of glb_nfa_closure, every row of which the caller has ANDed with `useful`: the
 * important states from which an accepting state can be reached.
 *   States and sets.  A state is a set of important NFA states closed under empty arcs, inside `useful`, a bitset of W words.
 *     So a set is live exactly when it is not empty, and there is no `live` table.  Id 0 is the closure of nfa_start (it may
 *     be empty: the language is).  The empty set is no state: it is -1, the dead state of glb_dfa_*.  A state accepts where
 *     its set meets accepting_mask.  The ids are [0, max_states); status[0] of them are numbered.
 *   step(set, b) = the union of eclose[dst] over the byte arcs (m, dst) of the set's members m whose byte set holds b.
 *   next(set, t) = step over the bytes of token t in turn, or empty when the token is skipped, empty, outside [0, vocab) or
 *     its offsets are not the vocabulary's: the rules of glb_dfa_advance.
 *   glb_lazy_advance: state_out[i] of dfa.tokens[i, from[i] .. to[i]) from dfa.state_in[i] (null: id 0).  A range outside
 *     [0, ld] or from > to, or a state outside [0, n) - n the states numbered when the call began - gives -1.  from == to
 *     gives the state back.  Else the tokens are walked from the state's set; an empty set at any point gives -1.  Sets in
 *     the middle of a range are never numbered: the set the particle ends in is looked up and, when new, numbered.
 *   Numbering.  The new sets of a call get consecutive ids, from status[0] up, in the order of the smallest particle index
 *     that ended in them - whatever order the atomics take; sets[id], accepting_out[id] are written.
 *   Overflow.  A new set beyond max_states gets no id: its particles get -1 and status[1] bit 0 (sticky) goes up.  What
 *     fits is decided by the same order.  The table never fills first: a call's particles are walked `cand_rows` at a time
 *     (the order of the chunks is the order of the particles), cand_rows <= table_slots - max_states, and a chunk that
 *     begins with every id taken claims no slot; the slots of the sets that found no id in the one chunk that crossed the
 *     bound stay behind as tombstones.
 *   Rows.  The row of state s in the bank (of glb_dfa_args: bank, row_of_state, work, counters, rows 0 and 1, `done`, the
 *     lifetime of ids) has bit t = next(sets[s], t) not empty, bit eos_id = accepting_out[s].  An id in [status[0],
 *     max_states) that a caller names before a set has it (glb_lazy_advance never returns one) is served row 0: the fill
 *     takes its claim back, so that the set that takes the id later gets a row of its own; the row claimed for it is lost
 *     to a bank that does not evict and free in one that does.
 * The embedded glb_dfa_args, its own struct_size set, carries the vocabulary, the particles, the bank and its counters; its
 * n_states, start, delta, accepting and live are not read: max_states, 0 and accepting_out stand in their places.
 *   status [GLB_LAZY_STATUS]: [0] states numbered  [1] flags, sticky: GLB_LAZY_OVERFLOW, GLB_LAZY_BUG (a reference out of
 *     range: never an input)  [2] the states numbered when the running call began  [3] private
 *   table: 12 bytes a slot as in glb_nfa_args - table_slots 64-bit words (31 bits of the set's hash; a particle index of the
 *     running chunk, its row of `cand`, or a numbered id, its row of `sets`), then int32 [table_slots], the smallest particle
 *     index that brought the slot's set.  hash_mask as in glb_nfa_args.
 *   glb_lazy_init     the table emptied, status = {1, 0, 1, ..}, accepting_out zeroed, sets[0] = eclose[nfa_start] and entered;
 *                     the bank started over (rows 0 and 1, row_of_state = -1 over max_states, counters) and, where the
 *                     eviction tables are given, those too (glb_dfa_evict_bank_init).
 *   glb_lazy_advance  six launches a chunk of cand_rows particles, no wave waiting on another's stores: walk (a wave per
 *                     particle, the set a word a lane; the end set to `cand`), enter (the table probed; a new set's slot
 *                     claimed by one compare-and-swap; the smallest particle index kept by atomicMin), count, scan, number
 *                     (cand copied to sets[id], accepting_out[id], the slot's reference turned into the id), resolve.
 *                     state_out may be state_in.  dfa.n == 0 is GLB_EINVAL, as for glb_dfa_advance.
 *   glb_lazy_serve    out_rows of state_in [n], `done` as glb_dfa_mask_ids: without eviction tables the launches of
 *                     glb_dfa_claim_rows, the fill, the commit, glb_dfa_mask_ids; with them those of glb_dfa_evict_serve.
 *                     The fill walks every token from sets[s]: n_words == 1 and force_wave == 0 - a lane a token, the set a
 *                     register, 64 tokens one ballot; else a wave a token, the set across the lanes, a workgroup of four
 *                     waves the 32 tokens of one word, eight each, the word written once.  force_wave != 0 gives a one-word
 *                     automaton the second form (a test compares the two).
 * GLB_EINVAL before any launch, the field named: struct_size of either block wrong; max_states outside [1, 2^22]; n_important
 * outside [0, min(n_nfa_states, GLB_NFA_MAX_IMPORTANT)]; n_words not max(1, ceil(n_important / 64)); n_nfa_states outside
 * [1, 2^24]; nfa_start outside the automaton; n_arcs negative; a null arc, mask, closure, table, sets, accepting_out, cand,
 * counts or status pointer; table_slots no power of two in [2 max_states, 2^30]; table not aligned to 8; cand_rows outside
 * [1, table_slots - max_states]; the eviction tables given in part; and for the bank and the vocabulary what glb_dfa_* refuse.
 * Everything read from device memory is range-checked; a bad work entry is skipped.  Nothing synchronises or allocates.
 */
#define GLB_LAZY_STATUS 8
#define GLB_LAZY_OVERFLOW 1
#define GLB_LAZY_BUG 2
typedef struct glb_lazy_args {
  uint32_t struct_size; /* sizeof(glb_lazy_args) - ABI guard */
  glb_dfa_args dfa;     /* its own struct_size set too: vocabulary, particles, bank, counters */
  int32_t n_nfa_states, nfa_start;
  int32_t n_important, n_words;
  int32_t n_arcs;
  int32_t max_states;
  const int32_t *arc_off, *arc_dst; /* [n_important + 1], [n_arcs] */
  const uint64_t *arc_bytes;        /* [n_arcs][4] */
  const uint64_t *accepting_mask;   /* [n_words] */
  const uint64_t *eclose;           /* [n_nfa_states][n_words], converged, inside `useful` */
  uint64_t hash_mask;               /* 0: every bit of the hash */
  void *table;                      /* 12 * table_slots bytes */
  int64_t table_slots;              /* a power of two >= 2 * max_states */
  uint64_t *cand;                   /* [cand_rows][n_words] */
  int32_t *counts;                  /* [ceil(cand_rows / 256)] */
  int64_t cand_rows;                /* particles a chunk of glb_lazy_advance takes */
  uint64_t *sets;                   /* [max_states][n_words] */
  uint8_t *accepting_out;           /* [max_states] */
  int32_t *status;                  /* [GLB_LAZY_STATUS] */
  /* the tables of glb_dfa_evict_args, all null: a bank that never evicts */
  int32_t *row_state, *row_stamp, *claimants, *victims; /* [dfa.capacity] each */
  int32_t *ecounters;                                   /* [GLB_DFA_EVICT_COUNTERS] */
  int32_t *epoch;                                       /* [1] */
  int32_t force_wave; /* debug: the wave form of the fill where n_words == 1 */
} glb_lazy_args;
int glb_lazy_init(const glb_lazy_args *args, void *hip_stream);
int glb_lazy_advance(const glb_lazy_args *args, void *hip_stream);
int glb_lazy_serve(const glb_lazy_args *args, void *hip_stream);

/*
 * Nested languages: a real-time deterministic pushdown automaton over bytes served as a constraint, its
 * configurations numbered on the device when a particle ends a call in them - the machinery of glb_lazy_* with a
 * configuration in place of a set.
 *   The automaton.  delta int32 [n_pda_states][n_symbols + 1][256], the middle index the top of the stack: plane 0 the empty
 *     stack, planes 1 .. G = n_symbols the stack symbols.  An entry is -1 (dead) or next | op << 24: next in [0, n_pda_states),
 *     op 0 (keep), g in 1 .. G (push g) or 127 (pop).  accepting uint8 [n_pda_states].  A byte string is accepted when its walk
 *     from (start, the empty stack) never dies and ends in an accepting state with the empty stack.
 *   Configurations.  A configuration is W = n_words = 1 + ceil(max_depth / 8) 64-bit words, 1 <= max_depth <=
 *     GLB_PDA_MAX_DEPTH, so W <= 64: word 0 is state | depth << 32, words 1 .. hold the stack, one byte a symbol, bottom
 *     first (symbol i: word 1 + i / 8, byte i % 8), every byte above depth zero - two configurations are equal exactly when
 *     their words are.  Id 0 is (start, empty).  The dead configuration is no state: it is -1, the dead state of glb_dfa_*.
 *     The ids are [0, max_states); status[0] of them are numbered.
 *   step(c, b): the entry delta[state, top(c), b], top the symbol at depth - 1 or 0 on the empty stack.  Dead on -1, on a
 *     push at depth == max_depth, on a pop from the empty stack and on an entry or a top whose fields are out of range
 *     (next >= n_pda_states, op in (G, 127), top > G).  Else the state becomes next and the stack is kept, pushed or popped.
 *   next(c, t) = step over the bytes of token t in turn, dead as soon as a step is; dead when the token is skipped, empty,
 *     outside [0, vocab) or its offsets are not the vocabulary's: the rules of glb_dfa_advance.
 *   glb_pda_advance: state_out[i] of dfa.tokens[i, from[i] .. to[i]) from dfa.state_in[i] (null: id 0).  A range outside
 *     [0, ld] or from > to, or a state outside [0, n) - n the configurations numbered when the call began - gives -1.
 *     from == to gives the state back.  Else the tokens are walked from the state's configuration; dead at any point gives
 *     -1.  Configurations in the middle of a range are never numbered: the one the particle ends in is looked up and, when
 *     new, numbered.
 *   Numbering.  The new configurations of a call get consecutive ids, from status[0] up, in the order of the smallest
 *     particle index that ended in them - whatever order the atomics take; configs[id] and accepting_out[id] =
 *     accepting[state] && depth == 0 are written.
 *   Overflow.  A new configuration beyond max_states gets no id: its particles get -1 and status[1] bit 0 (sticky) goes up.
 *     What fits is decided by the same order.  The table never fills first: a call's particles are walked `cand_rows` at a
 *     time (the order of the chunks is the order of the particles), cand_rows <= table_slots - max_states, and a chunk that
 *     begins with every id taken claims no slot; the slots of the configurations that found no id in the one chunk that
 *     crossed the bound stay behind as tombstones.
 *   Rows.  The row of state s in the bank (of glb_dfa_args: bank, row_of_state, work, counters, rows 0 and 1, `done`, the
 *     lifetime of ids) has bit t = next(configs[s], t) not dead, bit eos_id = accepting_out[s].  An id in [status[0],
 *     max_states) that a caller names before a configuration has it (glb_pda_advance never returns one) is served row 0: the
 *     fill takes its claim back, so that the configuration that takes the id later gets a row of its own; the row claimed for
 *     it is lost to a bank that does not evict and free in one that does.
 * The embedded glb_dfa_args, its own struct_size set, carries the vocabulary, the particles, the bank and its counters; its
 * n_states, start, delta, accepting and live are not read: max_states, 0 and accepting_out stand in their places.
 *   status [GLB_PDA_STATUS]: [0] configurations numbered  [1] flags, sticky: GLB_PDA_OVERFLOW, GLB_PDA_BUG (a reference
 *     out of range: never an input)  [2] the configurations numbered when the running call began  [3] private
 *   table: 12 bytes a slot as in glb_lazy_args.  hash_mask as in glb_nfa_args.
 *   max_token_bytes: at least the length of the vocabulary's longest token.  A lane of the fill keeps what a token pushed in
 *     min(max_token_bytes, max_depth) bytes; a token that pushes more than that is served dead.
 *   glb_pda_init     the table emptied, status = {1, 0, 1, ..}, accepting_out zeroed, configs[0] = (start, empty) and
 *                    entered; the bank started over and, where the eviction tables are given, those too.
 *   glb_pda_advance  six launches a chunk of cand_rows particles, no wave waiting on another's stores: walk (a wave per
 *                    particle, the configuration a word a lane: the top one lane's word in every lane and a shift, a push
 *                    or a pop a masked update in that lane; the end configuration to `cand`), then enter, count, scan,
 *                    number, resolve as glb_lazy_advance has them, keyed on the W raw words.  state_out may be state_in.
 *                    dfa.n == 0 is GLB_EINVAL, as for glb_dfa_advance.
 *   glb_pda_serve    out_rows of state_in [n], `done` as glb_dfa_mask_ids: without eviction tables the launches of
 *                    glb_dfa_claim_rows, the fill, the commit, glb_dfa_mask_ids; with them those of glb_dfa_evict_serve.
 *                    The fill: a lane a token, a workgroup one wave, 64 tokens one ballot and two words of the row; the
 *                    served configuration's stack read-only in LDS, a lane's own pushes in dynamic LDS [position][lane].
 * GLB_EINVAL before any launch, the field named: struct_size of either block wrong; max_states outside [1, 2^22];
 * n_pda_states outside [1, 2^24]; n_symbols outside [1, 126]; start outside the automaton; max_depth outside [1,
 * GLB_PDA_MAX_DEPTH]; n_words not 1 + ceil(max_depth / 8); a null delta, accepting, table, configs, accepting_out, cand,
 * counts or status pointer; table_slots no power of two in [2 max_states, 2^30]; table, configs or cand not aligned to 8;
 * cand_rows outside [1, table_slots - max_states]; max_token_bytes < 1 (glb_pda_serve); the eviction tables given in part;
 * and for the bank and the vocabulary what glb_dfa_* refuse.
 * Everything read from device memory is range-checked; a bad work entry is skipped.  Nothing synchronises or allocates.
 */
#define GLB_PDA_MAX_DEPTH 504
#define GLB_PDA_STATUS 8
#define GLB_PDA_OVERFLOW 1
#define GLB_PDA_BUG 2
typedef struct glb_pda_args {
  uint32_t struct_size; /* sizeof(glb_pda_args) - ABI guard */
  glb_dfa_args dfa;     /* its own struct_size set too: vocabulary, particles, bank, counters */
  int32_t n_pda_states, n_symbols, start;
  int32_t max_depth, n_words, max_states;
  const int32_t *delta;     /* [n_pda_states][n_symbols + 1][256] */
  const uint8_t *accepting; /* [n_pda_states] */
  uint64_t hash_mask;       /* 0: every bit of the hash */
  void *table;              /* 12 * table_slots bytes */
  int64_t table_slots;      /* a power of two >= 2 * max_states */
  uint64_t *cand;           /* [cand_rows][n_words] */
  int32_t *counts;          /* [ceil(cand_rows / 256)] */
  int64_t cand_rows;        /* particles a chunk of glb_pda_advance takes */
  uint64_t *configs;        /* [max_states][n_words] */
  uint8_t *accepting_out;   /* [max_states] */
  int32_t *status;          /* [GLB_PDA_STATUS] */
  /* the tables of glb_dfa_evict_args, all null: a bank that never evicts */
  int32_t *row_state, *row_stamp, *claimants, *victims; /* [dfa.capacity] each */
  int32_t *ecounters;                                   /* [GLB_DFA_EVICT_COUNTERS] */
  int32_t *epoch;                                       /* [1] */
  int32_t max_token_bytes; /* >= the longest token of the vocabulary */
} glb_pda_args;
int glb_pda_init(const glb_pda_args *args, void *hip_stream);
int glb_pda_advance(const glb_pda_args *args, void *hip_stream);
int glb_pda_serve(const glb_pda_args *args, void *hip_stream);

/*
 * Conjunctions of constraints: K = n_parts constraints of any kind - each with a bank of rows and state ids
 * of its own - served as one.  A state of the conjunction is the tuple of the K part states, numbered on the device when a
 * particle ends a call in it: the machinery of glb_lazy_* and glb_pda_* with a tuple in place of a set or a configuration.
 * No product automaton is made: a token survives from a tuple exactly when it survives from every part, so the tuple's row
 * is combined from the parts' rows.
 *   Tuples.  A tuple is W = n_words = ceil(K / 2) 64-bit words, 2 <= K <= GLB_CONJ_MAX_PARTS: part 2 j in the low half of
 *     word j, part 2 j + 1 in the high half; for odd K the high half of the last word is zero.  Every part state of a tuple is
 *     >= 0: a tuple with a dead part is no state but -1.  Id 0 is part_start[0 .. K).  The ids are [0, max_states);
 *     status[0] of them are numbered.
 *   glb_conj_unpack: part_states[k * part_ld + i] = part k of tuples[state_in[i]] (state_in null: id 0) for i in [0, n);
 *     every part -1 where state_in[i] is outside [0, status[0]).  With claim_states (glb_conj_serve's input, [n]):
 *     claim_states[i] = state_in[i] where it is numbered and done (nullable) is not set for i, else -1, and rep[state_in[i]]
 *     = i for those - some particle that holds the state, whichever store comes last.  One launch, a lane a particle.
 *   glb_conj_number: state_out[i] = the id of the tuple part_states[0 .. K)[i], -1 where a part is < 0.  Numbering and
 *     overflow are glb_pda_advance's, word for word: the new tuples of a call get consecutive ids, from status[0] up, in the
 *     order of the smallest particle index that ended in them; a new tuple beyond max_states gets no id, its particles -1,
 *     and status[1] bit 0 (sticky) goes up; the particles are taken cand_rows at a time, cand_rows <= table_slots -
 *     max_states, and a chunk that begins with every id taken claims no slot.  Five launches a chunk - enter, count, scan,
 *     number, resolve - a LANE a particle: a tuple is at most four words, which a lane packs from part_states, hashes and
 *     compares by itself (a reference to a particle of the chunk is compared against that particle's part states, so the
 *     packed tuples are not stored anywhere before they are numbered).
 *   glb_conj_serve: out_rows[i] of state_in[i] given claim_states, rep and part_rows[k] (int32 [n]: particle i's row in
 *     part k's bank, as that part's own serve call returned it under the same `done`).  Where done[i] is set: row 1 when
 *     part_rows[k][i] == 1 for every k, else row 0.  A state outside [0, max_states) or without a row: row 0.  Without
 *     eviction tables the launches are glb_dfa_claim_rows's (over claim_states), the combine, the commit and the ids; with
 *     them touch, select, the combine and the ids, as glb_dfa_evict_serve has them.
 *   The combine fills the row of every work entry (s, r) from the part rows of particle rep[s]: an entry whose s, r, rep[s]
 *     (it must hold s in claim_states) or part row (outside [0, part_capacity[k])) is out of range is skipped and its claim
 *     taken back.  A bit bank (wbank null): word w of the row is the AND over the parts of word w of their rows, words
 *     [0, ceil(vocab / 32)).  A float bank (wbank given): float t = 0.0f + the floats t of the weighted parts' rows (part
 *     order, float32, no fma), then -inf where the bit t of any unweighted part's row is clear; floats [0, vocab).  A part
 *     with part_weighted[k] != 0 has float rows [part_capacity[k]][part_bank_ld[k]], else int32 bit rows.  A lane takes
 *     four words (four floats) as one 16-byte access a part; what is left of a row is taken word by word.  A word or a
 *     float is written once: no atomic, no zeroing launch.
 * The embedded glb_dfa_args, its own struct_size set, carries vocab, eos_id, the particles (n, state_in, state_out, done,
 * out_rows) and the bank's bookkeeping (bank - or wbank here -, capacity, row_of_state [max_states], work, counters,
 * max_work); nothing else of it is read.
 *   status [GLB_CONJ_STATUS]: [0] tuples numbered  [1] flags, sticky: GLB_CONJ_OVERFLOW, GLB_CONJ_BUG (a reference out of
 *     range: never an input)  [2] the tuples numbered when the running call began  [3] private
 *   table: 12 bytes a slot as in glb_lazy_args.  hash_mask as in glb_nfa_args.
 *   glb_conj_init  the table emptied, status = {1, 0, 1, ..}, tuples[0] = part_start packed and entered, rep = -1; the bank
 *                  started over (rows 0 and 1 as glb_dfa_bank_init / glb_dfa_weight_bank_init write them) and, where the
 *                  eviction tables are given, those too.
 * GLB_EINVAL before any launch, the field named: struct_size of either block wrong; n_parts outside [2,
 * GLB_CONJ_MAX_PARTS]; n_words not ceil(n_parts / 2); max_states outside [1, 2^22]; a null table, tuples, status or rep
 * pointer; table_slots no power of two in [2 max_states, 2^30]; table or tuples not aligned to 8; the eviction tables given
 * in part; vocab outside [1, 2^31 - 256]; n <= 0; part_start[k] < 0 (init); a null part_states, part_ld < n (unpack,
 * number); a null state_out, counts, cand_rows outside [1, table_slots - max_states] (number); a null state_in,
 * claim_states, out_rows, part_rows[k] or part_bank[k], part_bank_ld[k] or bank_ld (wbank_ld) below a row's elements,
 * part_capacity[k] < 2, max_work <= 0 (serve); for the bank what glb_dfa_* refuse.
 * Everything read from device memory is range-checked.  Nothing synchronises or allocates.
 */
#define GLB_CONJ_MAX_PARTS 8
#define GLB_CONJ_STATUS 8
#define GLB_CONJ_OVERFLOW 1
#define GLB_CONJ_BUG 2
typedef struct glb_conj_args {
  uint32_t struct_size; /* sizeof(glb_conj_args) - ABI guard */
  glb_dfa_args dfa;     /* its own struct_size set too: vocab, eos_id, particles, the bank's bookkeeping */
  int32_t n_parts, n_words, max_states;
  int32_t part_start[GLB_CONJ_MAX_PARTS]; /* init: the parts of id 0 */
  uint64_t hash_mask;                     /* 0: every bit of the hash */
  void *table;                            /* 12 * table_slots bytes */
  int64_t table_slots;                    /* a power of two >= 2 * max_states */
  uint64_t *tuples;                       /* [max_states][n_words] */
  int32_t *status;                        /* [GLB_CONJ_STATUS] */
  int32_t *counts;                        /* [ceil(cand_rows / 256)] */
  int64_t cand_rows;                      /* particles a chunk of glb_conj_number takes */
  int32_t *part_states;                   /* [n_parts][part_ld] */
  int64_t part_ld;                        /* >= dfa.n */
  int32_t *claim_states;                  /* [n]: unpack (nullable there), serve */
  int32_t *rep;                           /* [max_states] */
  const int32_t *part_rows[GLB_CONJ_MAX_PARTS]; /* [n] each */
  const void *part_bank[GLB_CONJ_MAX_PARTS];    /* int32 or float [part_capacity][part_bank_ld] */
  int64_t part_bank_ld[GLB_CONJ_MAX_PARTS], part_capacity[GLB_CONJ_MAX_PARTS];
  int32_t part_weighted[GLB_CONJ_MAX_PARTS];
  float *wbank; /* [dfa.capacity][wbank_ld]; null: the bit bank dfa.bank */
  int64_t wbank_ld;
  /* the tables of glb_dfa_evict_args, all null: a bank that never evicts */
  int32_t *row_state, *row_stamp, *claimants, *victims; /* [dfa.capacity] each */
  int32_t *ecounters;                                   /* [GLB_DFA_EVICT_COUNTERS] */
  int32_t *epoch;                                       /* [1] */
} glb_conj_args;
int glb_conj_init(const glb_conj_args *args, void *hip_stream);
int glb_conj_unpack(const glb_conj_args *args, void *hip_stream);
int glb_conj_number(const glb_conj_args *args, void *hip_stream);
int glb_conj_serve(const glb_conj_args *args, void *hip_stream);

/*
 * Importance-weighted particle step: propose from q, weight toward p.  Per particle i, with target
 * row p = target[row_of[i]], proposal row q = proposal[row_of[i]] (the same context under two models; proposal null: the
 * target's own row, read from memory once), y_j = fl32(q_j * proposal_scale) when the scale is not 1 (else q_j), and mask row
 * m (GLB_MASK_BITS: 0 / -inf; GLB_MASK_F32: any float, -inf ok):
 *     qt(j)  ∝ exp(y_j + m_j)                              the proposal actually drawn from
 *     token  ~ qt
 *     dlogw  = (p_tok - lse(p)) - (y_tok - lse(y + m))     = log[softmax(p)_tok e^{m_tok}] - log qt(tok)
 * so that E_qt[exp(dlogw)] = sum_j softmax(p)_j e^{m_j}: adding dlogw to a particle's log-weight where the fused step adds
 * logZ keeps the population properly weighted for the same target.  With proposal null and scale 1, dlogw IS the fused
 * step's logZ, whatever token is drawn.
 *   out_token          -1 when nothing has proposal mass (the mask allows nothing, or y + m is -inf everywhere)
 *   out_dlogw          -inf for token -1 and where p_tok is -inf
 *   out_lse_target     lse(p)
 *   out_logZ_proposal  lse(y + m) - lse(y); -inf for token -1
 * Each output is nullable.  Masks: the table, mask_ld, n_masks, mask_id / row_mask_id and their null rules are those of
 * the fused step's argument block; kinds GLB_MASK_NONE, GLB_MASK_BITS (raw rows) and GLB_MASK_F32 - GLB_MASK_PREPARED is
 * the fused step's own layout and GLB_EINVAL here.  A row or mask id read from device memory that is out of range makes its
 * particle one whose mask allows nothing.  +inf and NaN logits, and logits beyond 2^21 in magnitude, are not supported
 * (no fault; the results are unspecified).
 * The draw: the fused step's Philox block - counter = (particle_base + i, offset), key = seed -, R1 = its words 0 and 1,
 * R2 = its words 2 and 3 (low word first).  Chunks are 4096 consecutive vocabulary indices; R1 / 2^64 picks the chunk by
 * inverse CDF over the chunks' masses under qt in chunk order, R2 / 2^64 the element by inverse CDF over that chunk's
 * elements of nonzero mass in index order.  Results are a function of the inputs alone: the same for a row alone or among
 * others, shared by many particles or copied for each, and however the particles are cut into calls (particle_base).
 * Arithmetic: a term is the hardware's 2^(x log2 e - N - 1) against the chunk's binary scale N; log-sum-exps within 1e-4
 * of the exact values of the inputs (observed: DESIGN.md section 28), CDF boundaries within 1e-5 of the stage's mass.
 * Two plain launches on `hip_stream` (one wave per unit and chunk - a unit is a logits row when row_mask_id or no mask is
 * given, else a particle -, then one wave per particle); nothing waits inside a launch, nothing synchronises or allocates;
 * safe under stream capture.  workspace: device scratch of at least the bytes glb_importance_workspace_bytes names (64 per
 * unit and chunk), 16-byte aligned, not shared with a workspace that glb_workspace_init registered; too small: GLB_ENOSPC.
 * GLB_EINVAL before any launch: struct_size wrong; target null; a dtype outside GLB_F32 .. GLB_F16 (the proposal's only
 * when a proposal is given - proposal_dtype and ld_q are not read otherwise); sizes not positive or beyond 31 bits; ld_p
 * or ld_q below vocab; a NaN scale; row_of null with n_particles != n_rows; a bad mask_kind; with a mask: the table null,
 * mask_ld below a row's elements, both id arrays given, no ids with n_masks neither 1 nor the number of units; workspace
 * null or misaligned.  With GLB_MASK_NONE no mask field is read.
 */
typedef struct glb_importance_args {
  uint32_t struct_size; /* sizeof this block - ABI guard */
  const void *target;   /* [n_rows, ld_p] device */
  int32_t target_dtype; /* GLB_F32 / GLB_BF16 / GLB_F16 */
  int64_t ld_p;         /* row pitch in elements, >= vocab */
  const void *proposal; /* [n_rows, ld_q] device, nullable: the target's own rows */
  int32_t proposal_dtype;
  int64_t ld_q;
  int64_t n_rows, vocab;
  float proposal_scale;
  int64_t n_particles;
  const int32_t *row_of; /* [n_particles] device, nullable: identity (needs n_particles == n_rows) */
  int32_t mask_kind;
  const void *mask; /* [n_masks, mask_ld] device: uint32 words or floats */
  int64_t mask_ld, n_masks;
  const int32_t *mask_id;     /* [n_particles] device, nullable */
  const int32_t *row_mask_id; /* [n_rows] device, nullable; exclusive with mask_id */
  uint64_t seed, offset;
  int64_t particle_base;
  int32_t *out_token;       /* [n_particles] */
  float *out_dlogw;         /* [n_particles] */
  float *out_lse_target;    /* [n_particles] */
  float *out_logZ_proposal; /* [n_particles] */
  void *workspace;
  size_t workspace_bytes;
} glb_importance_args;
size_t glb_importance_workspace_bytes(int64_t n_particles, int64_t n_rows, int64_t vocab);
int glb_importance_step(const glb_importance_args *args, void *hip_stream);

/*
 * Score given tokens: per logits row r, with y_j = fl32(x_j * logit_scale) when the scale is not 1
 * (else x_j), t = token[r] and mask row m (GLB_MASK_BITS: 0 / -inf; GLB_MASK_F32: any float, -inf ok):
 *     out_lse          = lse(y)
 *     out_logp         = y_t - lse(y)
 *     out_logZ         = lse(y + m) - lse(y)               -inf when nothing has mass
 *     out_logp_masked  = fl32(y_t + m_t) - lse(y + m)      -inf when m_t = -inf or nothing has mass
 * Each output is nullable, float32 [n_rows].  A token outside [0, vocab) gives -inf in out_logp and out_logp_masked (nothing
 * is loaded for it); a mask id outside [0, n_masks) makes the row one whose mask allows nothing; a row of all -inf gives -inf
 * in every output.  +inf and NaN logits, and logits beyond 2^21 in magnitude, are not supported (no fault; the results are
 * unspecified).  Masks: the table, mask_ld, n_masks, row_mask_id and the null rules are those of the fused step's argument
 * block with the logits row as the unit; kinds GLB_MASK_NONE, GLB_MASK_BITS (raw rows) and GLB_MASK_F32 -
 * GLB_MASK_PREPARED is GLB_EINVAL.  With GLB_MASK_NONE no mask field is read, out_logZ is 0 (-inf for a row of all -inf) and
 * out_logp_masked equals out_logp.
 * Sequence sums (seq_start non-null): out_seq_*[s] = the sum of the per-row output over rows seq_start[s] ..
 * seq_start[s + 1] - 1 in row order, accumulated in double and rounded once; an empty sequence sums to 0, any -inf term makes
 * the sum -inf.  seq_start is read on the device (ascending, last value n_rows; bounds outside [0, n_rows] are clipped).  A
 * sequence output needs its per-row output (out_seq_logp needs out_logp, and so on).
 * One launch, one workgroup of four waves per row: every logit and every mask word of the row is read once in 16-byte
 * loads (element aligned: any base and pitch), nothing of size [n_rows, vocab] is written, y_t and m_t are taken by the lane
 * that streams index t.  One more small launch per sequence sum asked for.  Nothing waits inside a launch, nothing
 * synchronises or allocates; safe under stream capture; no workspace.  A row's outputs are a function of that row's inputs
 * alone: the reduction tree (chunks of 4096 indices, chunk c on wave c mod 4, the four waves folded in order) does not
 * depend on n_rows, so the bits are the same for a row alone or among others and however the rows are cut into calls.
 * Arithmetic: glb_importance_step's - log-sum-exps within 1e-4 of the exact values of the inputs.
 * GLB_EINVAL before any launch: struct_size wrong; logits or token null; a dtype outside GLB_F32 .. GLB_F16; n_rows or vocab
 * not positive or beyond 31 bits; ld below vocab; logits not element aligned; a scale that is NaN, not positive or infinite; a bad or prepared mask_kind; with
 * a mask: the table null or misaligned, mask_ld below a row's elements, n_masks not positive or beyond 31 bits, no ids with
 * n_masks neither 1 nor n_rows; seq_start given with n_seq < 0; a sequence output given without seq_start or without its
 * per-row output.
 */
typedef struct glb_score_args {
  uint32_t struct_size; /* sizeof this block - ABI guard */
  const void *logits;   /* [n_rows, ld] device */
  int32_t dtype;        /* GLB_F32 / GLB_BF16 / GLB_F16 */
  int64_t n_rows, vocab;
  int64_t ld; /* row pitch in elements, >= vocab */
  float logit_scale;
  const int32_t *token; /* [n_rows] device */
  int32_t mask_kind;
  const void *mask; /* [n_masks, mask_ld] device: uint32 words or floats */
  int64_t mask_ld, n_masks;
  const int32_t *row_mask_id; /* [n_rows] device, nullable: n_masks == 1 ? 0 : identity */
  float *out_logp;            /* [n_rows] each, nullable */
  float *out_lse;
  float *out_logZ;
  float *out_logp_masked;
  const int64_t *seq_start; /* [n_seq + 1] device, nullable */
  int64_t n_seq;
  float *out_seq_logp; /* [n_seq] each, nullable */
  float *out_seq_logZ;
  float *out_seq_logp_masked;
} glb_score_args;
int glb_score_rows(const glb_score_args *args, void *hip_stream);
/* The sequence sums alone, for per-row values that several glb_score_rows calls wrote (rows scored in chunks): out[s] = the
 * sum of values[seq_start[s] .. seq_start[s + 1]) under the same rules.  One launch; GLB_EINVAL for a null pointer or a size
 * that is negative or beyond 31 bits; n_seq == 0 launches nothing. */
int glb_score_seq_sums(const float *values, int64_t n_rows, const int64_t *seq_start, int64_t n_seq, float *out, void *hip_stream);

/*
 * The k most probable tokens of every logits row: per logits row r, with y_j = fl32(x_j * logit_scale)
 * when the scale is not 1 (else x_j), mask row m (GLB_MASK_BITS: 0 / -inf; GLB_MASK_F32: any float, -inf ok) and
 * key_j = fl32(y_j + m_j), for k in 1 .. 64, dense outputs [n_rows, k] (out_lse, out_logZ: [n_rows]), each nullable except
 * out_token:
 *     out_token        the indices of the k largest keys, largest first.  Keys compare as floats, -0 equals +0, equal keys
 *                      order by lower index.  A key of -inf is never selected: positions beyond the number of finite keys
 *                      hold token -1, and -inf in both float outputs.
 *     out_logp         = key - lse(y)        bit masks: the token's log-probability under the model; float masks: that plus
 *                                            the token's weight - what a search adds up
 *     out_logp_masked  = key - lse(y + m)
 *     out_lse          = lse(y)
 *     out_logZ         = lse(y + m) - lse(y)               -inf when nothing has mass
 * A mask id outside [0, n_masks) makes the row one whose mask allows nothing; a row of all -inf gives every token -1 and
 * every float -inf, no NaN.  +inf and NaN logits or mask floats, and magnitudes beyond 2^21, are not supported (no fault; the
 * results are unspecified).  Masks: the table, mask_ld, n_masks, row_mask_id and the null rules are glb_score_args's; kinds
 * GLB_MASK_NONE, GLB_MASK_BITS (raw rows) and GLB_MASK_F32 - GLB_MASK_PREPARED is GLB_EINVAL.  With GLB_MASK_NONE no mask
 * field is read, out_logZ is 0 (-inf for a row of all -inf) and out_logp_masked equals out_logp.
 * One launch, one workgroup of four waves per row: every logit and every mask word of the row is read once in 16-byte loads
 * (element aligned: any base and pitch), nothing of size [n_rows, vocab] is written.  Nothing waits inside the launch,
 * nothing synchronises or allocates; safe under stream capture; no workspace.
 * The token ids are exact: a key is one rounded multiply and one rounded add, the selection compares keys and indices only, so
 * the ids are a function of the inputs that float32 arithmetic on the host reproduces bit for bit.  The log-sum-exps are
 * glb_score_rows's: within 1e-4 of the exact values of the inputs.  A row's outputs are a function of that row's inputs alone
 * (chunks of 4096 indices, chunk c on wave c mod 4, the four waves folded in order): the same bytes for a row alone or among
 * others and however the rows are cut into calls.
 * GLB_EINVAL before any launch: struct_size wrong; logits or out_token null; k outside 1 .. 64; a dtype outside GLB_F32 ..
 * GLB_F16; n_rows or vocab not positive or beyond 31 bits; ld below vocab; logits not element aligned; a scale that is NaN, not
 * positive or infinite; a bad or prepared mask_kind; with a mask: the table null or misaligned, mask_ld below a row's
 * elements, n_masks not positive or beyond 31 bits, no ids with n_masks neither 1 nor n_rows.
 */
typedef struct glb_topk_args {
  uint32_t struct_size; /* sizeof this block - ABI guard */
  const void *logits;   /* [n_rows, ld] device */
  int32_t dtype;        /* GLB_F32 / GLB_BF16 / GLB_F16 */
  int64_t n_rows, vocab;
  int64_t ld; /* row pitch in elements, >= vocab */
  float logit_scale;
  int32_t k; /* 1 .. 64 */
  int32_t mask_kind;
  const void *mask; /* [n_masks, mask_ld] device: uint32 words or floats */
  int64_t mask_ld, n_masks;
  const int32_t *row_mask_id; /* [n_rows] device, nullable: n_masks == 1 ? 0 : identity */
  int32_t *out_token;         /* [n_rows, k] */
  float *out_logp;            /* [n_rows, k] each, nullable */
  float *out_logp_masked;
  float *out_lse; /* [n_rows] each, nullable */
  float *out_logZ;
} glb_topk_args;
int glb_topk_rows(const glb_topk_args *args, void *hip_stream);
/*
 * A beam step's selection: n_groups groups of `width` beams (1 .. 64).  score float32 [n_groups * width], alive int32
 * [n_groups * width], cand_token int32 and cand_logp float32 [n_groups * width, k] as glb_topk_rows writes them (k in 1 .. 64).
 * Group g's candidates, per beam b: an alive beam with a finite score gives (b, j) with value fl32(score[b] + cand_logp[b, j])
 * for every j with cand_token[b, j] >= 0 and a finite value; a beam that is not alive but has a finite score is a finished
 * hypothesis and gives one candidate (b, token -1) with value score[b]; a beam whose score is not finite gives nothing.
 * out_parent (the beam's index within its group), out_token and out_score, each [n_groups * width]: the `width` largest
 * values, largest first (-0 equals +0), ties by lower (b, j); missing positions get parent -1, token -1, score -inf.
 * One launch, one wave per group, no workspace, nothing waits; safe under stream capture.  GLB_EINVAL before the launch: a
 * null pointer; width or k outside 1 .. 64; n_groups not positive or 2^19 and above.
 */
int glb_beam_select(const float *score, const int32_t *alive, const int32_t *cand_token, const float *cand_logp, int64_t n_groups,
                    int32_t width, int32_t k, int32_t *out_parent, int32_t *out_token, float *out_score, void *hip_stream);

/*
 * Top-k, top-p (nucleus) and min-p truncation: the keep set of every logits row as a bit row.  Keys as
 * glb_topk_rows takes them: y_j = fl32(x_j * logit_scale), mask row m (GLB_MASK_NONE, raw GLB_MASK_BITS, GLB_MASK_F32),
 * key_j = fl32(y_j + m_j), -0 equals +0, a key that is not above -inf is never kept.  The row's threshold is
 * tau = max(tau_k, tau_p, tau_m):
 *     tau_k   the top_k-th largest key, counted with multiplicity; -inf when top_k is 0 or the row has no more than top_k finite
 *             keys.  Exact.
 *     tau_m   fl32(key_max + log_min_p); log_min_p = -inf: off.  The host passes the float32 log(min_p).  Exact.
 *     tau_p   over the keys at or above tau_k (top-k first, then top-p: the order of the common samplers): with
 *             w_j = exp(key_j - key_max) and Z_k their sum over key_j >= tau_k, the largest key t of the row with
 *             sum over key_j >= t of w_j >= top_p * Z_k; top_p = 1: off.  The device's tau_p is the exact answer for some p'
 *             with |p' - top_p| <= 1e-4.
 * The keep set is {j : key_j > -inf and key_j >= tau}: every tie at tau is kept (a row may keep more than top_k tokens), and
 * the row's largest key is always kept.
 *     out_bits       uint32 [n_rows, out_ld], required: words 0 .. ceil(vocab / 32) - 1 of every row are written - bit j % 32 of
 *                    word j / 32 is token j, as glb_mask_f32_to_bits writes them, pad bits 0 - and read as raw GLB_MASK_BITS rows
 *                    by the fused step, glb_score_rows and glb_topk_rows; words beyond are not touched.
 *     out_threshold  float32 [n_rows], nullable: tau
 *     out_kept       int32 [n_rows], nullable: the number of kept tokens
 *     out_logmass    float32 [n_rows], nullable: log(kept mass / mass of all finite keys), within 1e-4
 * A row without a finite key (a mask id outside [0, n_masks) allows nothing) gives zero bits, kept 0, tau +inf and logmass -inf,
 * no NaN.  +inf and NaN inputs and magnitudes beyond 2^21 are not supported (no fault; the results are unspecified).
 * One launch, one workgroup of four waves per row, no workspace; nothing waits inside the launch, nothing synchronises or
 * allocates; safe under stream capture.  The row is read once for its maximum, three times for tau_k, three times for tau_p
 * (twice when tau_k was taken: the first pass is shared) and once to write the bits; an option that is off costs no pass.
 * A row's outputs are a function of that row's inputs alone - a key's mass is a function of the key and the row's maximum,
 * every sum of counts and masses is an integer sum (round(w * 2^40) per key, hence vocab <= 2^24) - the same bytes for a row
 * alone or among others, however the rows are cut into calls, run after run.
 * GLB_EINVAL before any launch: every rule of glb_topk_args but the one on k, and top_k < 0; top_p NaN, <= 0 or > 1; log_min_p NaN
 * or > 0; out_bits null or not 4-byte aligned; out_ld < ceil(vocab / 32); vocab > 2^24.
 */
typedef struct glb_truncate_args {
  uint32_t struct_size; /* sizeof this block - ABI guard */
  const void *logits;   /* [n_rows, ld] device */
  int32_t dtype;        /* GLB_F32 / GLB_BF16 / GLB_F16 */
  int64_t n_rows, vocab;
  int64_t ld; /* row pitch in elements, >= vocab */
  float logit_scale;
  int32_t mask_kind;
  const void *mask; /* [n_masks, mask_ld] device: uint32 words or floats */
  int64_t mask_ld, n_masks;
  const int32_t *row_mask_id; /* [n_rows] device, nullable: n_masks == 1 ? 0 : identity */
  int64_t top_k;              /* 0: off */
  float top_p;                /* (0, 1]; 1: off */
  float log_min_p;            /* <= 0; -inf: off */
  uint32_t *out_bits;         /* [n_rows, out_ld] */
  int64_t out_ld;             /* row pitch in words, >= ceil(vocab / 32) */
  float *out_threshold;       /* [n_rows] each, nullable */
  int32_t *out_kept;
  float *out_logmass;
} glb_truncate_args;
int glb_truncate_rows(const glb_truncate_args *args, void *hip_stream);

/*
 * A byte-level beam over tokenisations: next-byte distributions of a token model, marginalised over the
 * token sequences that spell a byte prefix.  A candidate is (token context, trie node n, u = log-probability of the committed
 * tokens, w = u + log mass of n under the context's next-token distribution); n_groups groups of `width` candidates (1 .. 64)
 * live in slots that never move: group g owns slots g * width .. g * width + width - 1 of node int32, u and w float32, alive
 * int32.  The trie is TokenByteTrie's CSR (child_ptr int32 [n_nodes + 1], child_idx int32, ascending children) with the edge
 * symbols child_sym int16 beside child_idx: 0 .. 255 a byte, 256 + j the node's j-th leaf child (a token that ends here;
 * j < GLB_BYTELM_LEAVES), any other value an edge that is never selected (-2: an ignored token's leaf).  The EOS tokens have
 * empty byte strings: their leaves are the root's.  leaf_token int32 [n_nodes]: the token a leaf ends, -1 for other nodes.
 *
 * glb_bytelm_children  sel int32 [n_slots, GLB_BYTELM_SEL]: columns 0 .. 255 the byte children of the slot's node, 256 .. 259
 *     its leaf children, -1 where there is none; all -1 for a slot that is not alive or whose node lies outside the trie.  Reads
 *     node, alive and the CSR.  One wave per slot.  The rows are what glb_trie_rows takes as per-row selections; the masses
 *     it returns for them are `mass`, float32 [n_slots, GLB_BYTELM_SEL], below (a mass that is not above 0, NaN too, counts as
 *     none).
 * glb_bytelm_extend  a token boundary: per group, every alive candidate with a finite w and u is an existing entry of weight
 *     w; every alive candidate whose node is not the root offers, for each leaf child l (column 256 + j) with mass m > 0,
 *     a spawned candidate of weight fl32(u + logf(m)) that has committed leaf_token[l].  The `width` largest weights are
 *     kept: equal weights by existing before spawned, then lower slot, then lower j; -0 equals +0; a weight that is not
 *     finite is never kept.  A kept existing candidate stays in its slot as it is; the r-th best spawned survivor takes the
 *     r-th lowest slot of the group that no kept candidate holds, at the root with u = w = its weight.  Per slot:
 *     out_parent (the slot itself for a kept candidate, the slot of the candidate that offered it for a spawned one, -1
 *     for an empty slot: alive 0, u = w = -inf, node root), out_token (the committed token of a spawned candidate, else -1),
 *     out_node, out_alive, out_u, out_w - the new state, which may not lie over the old one.  out_spawned int32 [n_slots]:
 *     the slots that hold a spawned candidate, ascending, -1 behind them; out_n_spawned int32 [1] their number.  fresh int32
 *     [n_groups], nullable: a group whose entry is 0 has not moved since it was last extended and offers nothing; the call
 *     sets the entries to 0.  Reads node, u, w, alive, sel, mass.  One wave per group, then one wave for the list.
 * glb_bytelm_next  with a = the largest finite u of the group's alive candidates and e_s = expf(u_s - a), in float32:
 *     num[b] = sum over the slots s in ascending order of e_s * mass[s, b] for the bytes b, num[256] the same sum of
 *     e_s * (mass[s, 256] + .. + mass[s, 259]) over the candidates at the root, Z = the sum of all 257 in a fixed order.
 *     byte null: out_next float32 [n_groups, GLB_BYTELM_ROW] = logf(num) - logf(Z), -inf where num is 0; out_logZ float32
 *     [n_groups] = a + logf(Z).  A group without an alive candidate or without mass gets -inf everywhere, no NaN.
 *     byte int32 [n_groups] given: nothing of the above is written; a group whose byte is outside 0 .. 256 is left alone;
 *     else logp[g] += the row's entry for the byte, and every alive candidate moves to sel[s, byte] with
 *     w = fl32(u + logf(mass[s, byte])), or dies (alive 0, w -inf) when there is no such child, its mass is not above 0, or
 *     the byte is 256 (EOS ends the group); fresh[g], if given, becomes 1.  Writes node, w, alive, logp in place.
 *     One wave per group.  A group's outputs depend on that group's inputs alone: the same bytes however groups are batched.
 * Each call: no workspace beyond its arguments, nothing waits, synchronises or allocates; safe under stream capture.
 * GLB_EINVAL before any launch: struct_size wrong; width outside 1 .. 64; n_groups or n_nodes not positive; n_groups * width or
 * n_nodes beyond 31 bits; root outside the trie; a null pointer among those the call reads or writes.
 */
#define GLB_BYTELM_SEL 260
#define GLB_BYTELM_ROW 257
#define GLB_BYTELM_LEAVES 4
typedef struct glb_bytelm_args {
  uint32_t struct_size; /* sizeof this block - ABI guard */
  int32_t width;        /* 1 .. 64 */
  int64_t n_groups;
  int64_t n_nodes;
  int32_t root;
  const int32_t *child_ptr; /* [n_nodes + 1] */
  const int32_t *child_idx;
  const int16_t *child_sym;
  const int32_t *leaf_token; /* [n_nodes] */
  int32_t *node;             /* [n_slots] each */
  int32_t *alive;
  const float *u;
  float *w;
  int32_t *sel;      /* [n_slots, GLB_BYTELM_SEL] */
  const float *mass; /* [n_slots, GLB_BYTELM_SEL] */
  int32_t *fresh;    /* [n_groups], nullable */
  int32_t *out_parent; /* [n_slots] each */
  int32_t *out_token;
  int32_t *out_node;
  int32_t *out_alive;
  float *out_u;
  float *out_w;
  int32_t *out_spawned;   /* [n_slots] */
  int32_t *out_n_spawned; /* [1] */
  const int32_t *byte;    /* [n_groups], nullable */
  float *out_next;        /* [n_groups, GLB_BYTELM_ROW] */
  float *out_logZ;        /* [n_groups] */
  float *logp;            /* [n_groups] */
} glb_bytelm_args;
int glb_bytelm_children(const glb_bytelm_args *args, void *hip_stream);
int glb_bytelm_extend(const glb_bytelm_args *args, void *hip_stream);
int glb_bytelm_next(const glb_bytelm_args *args, void *hip_stream);

/*
 * One byte step of the beam under a byte automaton: per group g, in one launch, what glb_bytelm_next, a
 * mask, a normalisation, a draw and glb_bytelm_next(byte) do.  The automaton's tables are those of the constraint calls: delta
 * int32 [n_states, 256] (a target outside 0 .. n_states - 1: no arc), accepting and live uint8 [n_states], and - both or
 * neither - arc_logw float32 [n_states, 256] and final_logw float32 [n_states].  Per group: state int32 (the automaton's state,
 * -1 once the group has ended or died), ended int32 (1 after EOS was read from an accepting state), log_weight float32.
 *
 * A group with ended[g] != 0 is skipped: of the group nothing is written; its out_row and out_logZc are -inf and a drawn step's
 * out_byte is -1.  Otherwise, with row[0 .. 256] and logZ exactly glb_bytelm_next's and s = state[g]:
 *     lc[b]   = row[b] + arc_logw[s, b] (+ 0 without weights) where t = delta[s, b] lies in 0 .. n_states - 1 and live[t] != 0,
 *               else -inf;  lc[256] = row[256] + final_logw[s] (+ 0 without weights) where accepting[s] != 0, else -inf.  A sum
 *               that is not finite (a weight of -inf, NaN or +inf) is -inf.  s outside 0 .. n_states - 1: all -inf, nothing
 *               of the tables is read.
 *     logZc   = m + logf(sum of expf(lc - m)), m the largest lc; the sum in the fixed order of glb_bytelm_next's Z.  -inf where
 *               every lc is.  out_logZc[g] = logZc; out_row[g, :] (nullable) = lc - logZc, -inf where lc is.
 *     peek != 0: nothing else happens; beam.byte and uniform are not read.
 *     the byte  beam.byte given: byte[g]; outside 0 .. 256 the group is left wholly alone, as an ended one.
 *               uniform float32 [n_groups] given: the first column c in the order 0 .. 256 with lc[c] > -inf whose cumulative
 *               probability exceeds uniform[g]; the cumulative probability of column q * 64 + l is the sum of the totals of
 *               the 64-column blocks before block q plus the inclusive scan of expf(out_row) over the block's lanes 0 .. l
 *               (doubling steps 1, 2, .. 32), all in float32; where none exceeds it, the last column with lc > -inf.
 *               neither: that rule with uniform = (float)(r0 >> 8) * 2^-24, r0 word 0 of glb_philox4x32_10 with counter
 *               {low 32 bits of g, high 32 bits of g, low 32 bits of offset, high 32 bits of offset} and key {low 32 bits of
 *               seed, high 32 bits of seed} - the counter and key of the fused step's draws (g in the particle's place), whose
 *               draws are integers; this one is the 24 high bits of one word.
 *     the group dies when every lc is -inf, or when the given byte's lc is -inf: state -1, log_weight -inf, every candidate
 *               dead (alive 0, w -inf), fresh 1; logp grows by the given byte's row entry, and not at all without a byte;
 *               out_byte (nullable when the byte is given) gets -1 when the byte was to be drawn, else the given byte.
 *     otherwise node, w, alive, fresh and logp change exactly as under glb_bytelm_next(byte) - logp by the UNCONSTRAINED row's
 *               entry; state[g] = delta[s, byte], or -1 after EOS, which also sets ended[g] = 1; log_weight[g] += logZc for a
 *               drawn byte, and for a given one += what the automaton gives it, lc[byte] - row[byte]: arc_logw[s, byte]
 *               (final_logw[s] for EOS), 0 without weights; out_byte[g] = the byte.
 * One wave per group; a group's outputs depend on that group's inputs alone.  No workspace, nothing waits, synchronises or
 * allocates; safe under stream capture.  GLB_EINVAL before any launch: what glb_bytelm_next refuses for `beam` (its struct_size
 * included); struct_size wrong; n_states not positive or n_states * 256 beyond 31 bits; null delta, accepting, live, state,
 * ended or out_logZc; arc_logw without final_logw or the reverse; without peek: null beam.logp or log_weight, and null
 * out_byte where the byte is drawn.
 */
typedef struct glb_bytelm_step_args {
  uint32_t struct_size; /* sizeof this block - ABI guard */
  int32_t peek;         /* nonzero: out_row / out_logZc only, nothing moves */
  glb_bytelm_args beam; /* the beam, as for glb_bytelm_next; beam.byte: the given bytes, nullable */
  int64_t n_states;
  const int32_t *delta;     /* [n_states, 256] */
  const uint8_t *accepting; /* [n_states] */
  const uint8_t *live;      /* [n_states] */
  const float *arc_logw;    /* [n_states, 256], nullable (with final_logw) */
  const float *final_logw;  /* [n_states], nullable */
  int32_t *state;           /* [n_groups] each */
  int32_t *ended;
  float *log_weight;
  const float *uniform; /* [n_groups], nullable */
  uint64_t seed;
  uint64_t offset;
  int32_t *out_byte; /* [n_groups] */
  float *out_row;    /* [n_groups, GLB_BYTELM_ROW], nullable */
  float *out_logZc;  /* [n_groups] */
} glb_bytelm_step_args;
int glb_bytelm_step(const glb_bytelm_step_args *args, void *hip_stream);

/* Philox4x32-10 block function, exposed so hosts can reproduce the device draws. */
void glb_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* GLB_H */
