"""ctypes binding of libglb_hip.so (C ABI: include/glb.h).

There is no fallback: if the shared object is missing or cannot be loaded this module raises, and
every compute entry point raises when the HIP runtime sees no device.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libglb_hip.so")

ABI_VERSION = 9
GLB_OK, GLB_EINVAL, GLB_EUNSUPPORTED, GLB_EHIP, GLB_ENOSPC = 0, 1, 2, 3, 4
F32, BF16, F16 = 0, 1, 2
MASK_NONE, MASK_BITS, MASK_F32, MASK_PREPARED = 0, 1, 2, 3
RNG_NONE, RNG_PHILOX, RNG_NOISE = 0, 1, 2
STEP_HW_EXP = 1  # glb_step_args.flags: the hardware-exponential contract of 16-bit rows
GEMM_BIAS, GEMM_BIAS_GELU_TANH = 0, 1  # glb_gemm_args.epilogue
GEMM_FORM_LARGE, GEMM_FORM_SMALL = 1, 2  # glb_gemm_f32_split_form's tile form (0: picked from the shape)


class GlbError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"glb error {code}: {msg}")
        self.code = code


class StepArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("logits", C.c_void_p),
        ("dtype", C.c_int32),
        ("n_rows", C.c_int64),
        ("vocab", C.c_int64),
        ("ld", C.c_int64),
        ("logit_scale", C.c_float),
        ("n_particles", C.c_int64),
        ("row_of", C.c_void_p),
        ("mask_kind", C.c_int32),
        ("mask", C.c_void_p),
        ("mask_ld", C.c_int64),
        ("n_masks", C.c_int64),
        ("mask_id", C.c_void_p),
        ("row_mask_id", C.c_void_p),
        ("rng_mode", C.c_int32),
        ("noise", C.c_void_p),
        ("noise_ld", C.c_int64),
        ("seed", C.c_uint64),
        ("offset", C.c_uint64),
        ("particle_base", C.c_int64),
        ("out_logZ", C.c_void_p),
        ("out_lse", C.c_void_p),
        ("out_token", C.c_void_p),
        ("out_margin", C.c_void_p),
        ("flags", C.c_int32),
        ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_size_t),
    ]


class TriePlan(C.Structure):
    _fields_ = [("struct_size", C.c_uint32)] + [(k, C.c_int32) for k in ("n_parts", "n_top", "n_cut", "n_slots", "max_local", "top_base",
                                                                          "lds_bytes")] + [
        ("n_nodes", C.c_int64)] + [(k, C.c_void_p) for k in ("desc", "idepth", "leaf_src", "leaf_local", "run_tab", "top_local", "slot_of",
                                                             "cptr16", "inode16", "pn_local16", "tok_local16", "inode64")] + [
        ("lds_top_bytes", C.c_int32), ("vocab", C.c_int32)]


class TrieRowsArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("weights", C.c_void_p),
        ("dtype", C.c_int32),
        ("ld", C.c_int64),
        ("n_rows", C.c_int64),
        ("vocab", C.c_int64),
        ("lse", C.c_void_p),
        ("logit_scale", C.c_float),
        ("from_logprobs", C.c_int32),
        ("op", C.c_int32),
        ("out_slots", C.c_void_p),
        ("out_slots_ld", C.c_int64),
        ("out_nodes", C.c_void_p),
        ("out_nodes_ld", C.c_int64),
        ("sel_nodes", C.c_void_p),
        ("n_sel", C.c_int64),
        ("out_sel", C.c_void_p),
        ("out_sel_ld", C.c_int64),
        ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_size_t),
        ("sel_row_stride", C.c_int64),
    ]


class TrieArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("weights", C.c_void_p),
        ("dtype", C.c_int32),
        ("ld", C.c_int64),
        ("n_rows", C.c_int64),
        ("vocab", C.c_int64),
        ("lse", C.c_void_p),
        ("logit_scale", C.c_float),
        ("from_logprobs", C.c_int32),
        ("op", C.c_int32),
        ("n_nodes", C.c_int64),
        ("n_levels", C.c_int64),
        ("leaf_node", C.c_void_p),
        ("level_start_host", C.c_void_p),
        ("level_nodes", C.c_void_p),
        ("child_ptr", C.c_void_p),
        ("child_idx", C.c_void_p),
        ("out", C.c_void_p),
        ("out_ld", C.c_int64),
        ("sel_nodes", C.c_void_p),
        ("n_sel", C.c_int64),
        ("out_sel", C.c_void_p),
        ("out_sel_ld", C.c_int64),
        ("keep_node_major", C.c_int32),
        ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_size_t),
    ]


class KvPlanArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n", C.c_int64), ("n_rows", C.c_int64), ("cap", C.c_int64),
        ("group_of", C.c_void_p), ("rep", C.c_void_p), ("n_groups", C.c_void_p),
        ("old_row", C.c_void_p),
        ("old_row_by_context", C.c_int32),
        ("lengths", C.c_void_p),
        ("row_stamps", C.c_void_p),
        ("call_no", C.c_int64),
        ("row_tok", C.c_void_p), ("row_len", C.c_void_p),
        ("row_hash", C.c_void_p),
        ("group_hash", C.c_void_p),
        ("tokens", C.c_void_p),
        ("starts", C.c_void_p),
        ("out_group_row", C.c_void_p), ("out_logits_row", C.c_void_p), ("out_rows_a", C.c_void_p), ("out_ctx_a", C.c_void_p),
        ("out_pos_a", C.c_void_p), ("out_ctx_b", C.c_void_p), ("out_rows_b", C.c_void_p), ("out_copy_src", C.c_void_p),
        ("out_copy_len", C.c_void_p), ("out_ctx_of_row", C.c_void_p), ("out_pos_of_row", C.c_void_p),
        ("out_row_of_context", C.c_void_p), ("out_head", C.c_void_p),
        ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_size_t),
    ]


class KvPlanChunkArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("plan", KvPlanArgs),
        ("old_keep", C.c_void_p),
        ("out_n_new_a", C.c_void_p), ("out_n_new_of_row", C.c_void_p),
    ]


KV_CHUNK_MAX = 16  # GLB_KV_CHUNK_MAX


class MT19937(C.Structure):
    _fields_ = [("mt", C.c_uint32 * 624), ("idx", C.c_int32)]


MT_POLY_WORDS = 312


class MtRowsArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("window", C.c_void_p), ("window_out", C.c_void_p), ("polys", C.c_void_p),
        ("n_small", C.c_int32), ("n_big", C.c_int32),
        ("vocab", C.c_int64), ("max_draw_rows", C.c_int64),
        ("n_draw", C.c_void_p),
        ("n_out_rows", C.c_int64),
        ("row_slot", C.c_void_p),
        ("out", C.c_void_p), ("out_ld", C.c_int64),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("reuse_windows", C.c_int32), ("rows_from", C.c_void_p), ("rows_from_ld", C.c_int64),
    ]


class GemmArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("m", C.c_int64), ("n", C.c_int64), ("k", C.c_int64),
        ("a", C.c_void_p), ("lda", C.c_int64),
        ("w_split", C.c_void_p),
        ("bias", C.c_void_p),
        ("c", C.c_void_p), ("ldc", C.c_int64),
        ("epilogue", C.c_int32),
    ]


class PackedPlanArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_tokens", C.c_int64), ("n_contexts", C.c_int64), ("n_sel", C.c_int64), ("n_groups", C.c_int64),
        ("n_pre", C.c_int64), ("n_tail_rows", C.c_int64), ("pos_cap", C.c_int64),
        ("tokens", C.c_void_p), ("starts", C.c_void_p), ("lengths", C.c_void_p), ("sel", C.c_void_p), ("grp", C.c_void_p),
        ("group_starts", C.c_void_p), ("group_lens", C.c_void_p), ("group_segments", C.c_void_p),
        ("group_ids", C.c_void_p), ("group_pos", C.c_void_p),
        ("segments", C.c_void_p), ("ids", C.c_void_p), ("pos", C.c_void_p), ("last", C.c_void_p), ("ends", C.c_void_p),
    ]


class LoraJob(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("w_dtype", C.c_int32), ("ab_dtype", C.c_int32), ("w_transposed", C.c_int32),
        ("n_out", C.c_int64), ("k_in", C.c_int64), ("r", C.c_int64),
        ("w", C.c_void_p), ("ldw", C.c_int64),
        ("a", C.c_void_p), ("lda", C.c_int64),
        ("b", C.c_void_p), ("ldb", C.c_int64),
        ("scale", C.c_float),
        ("out", C.c_void_p), ("ldo", C.c_int64),
    ]


class LoraRowsEntry(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("ab_dtype", C.c_int32),
        ("n_out", C.c_int64), ("k_in", C.c_int64), ("r", C.c_int64),
        ("a", C.c_void_p), ("lda", C.c_int64),
        ("b", C.c_void_p), ("ldb", C.c_int64),
        ("scale", C.c_float),
    ]


class LoraRowsArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("dtype", C.c_int32),
        ("m", C.c_int64), ("n", C.c_int64), ("k", C.c_int64),
        ("x", C.c_void_p), ("ldx", C.c_int64),
        ("y", C.c_void_p), ("ldy", C.c_int64),
        ("row_slot", C.c_void_p),
        ("table", C.c_void_p),
        ("n_slots", C.c_int32), ("n_modules", C.c_int32), ("module", C.c_int32), ("r_max", C.c_int32),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
    ]


class W4Args(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("dtype", C.c_int32), ("transposed", C.c_int32),
        ("n", C.c_int64), ("k", C.c_int64),
        ("w", C.c_void_p), ("ldw", C.c_int64),
        ("codebook", C.POINTER(C.c_float)),
        ("image", C.c_void_p), ("image_bytes", C.c_size_t),
    ]


class W4GemmArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("dtype", C.c_int32),
        ("m", C.c_int64), ("n", C.c_int64), ("k", C.c_int64),
        ("x", C.c_void_p), ("ldx", C.c_int64),
        ("image", C.c_void_p),
        ("codebook", C.POINTER(C.c_float)),
        ("bias", C.c_void_p),
        ("y", C.c_void_p), ("ldy", C.c_int64),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
    ]


DFA_COUNTERS = 4  # GLB_DFA_COUNTERS: rows in use, work entries filled, overflow (sticky), private


class DfaArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_states", C.c_int32), ("start", C.c_int32), ("eos_id", C.c_int32),
        ("delta", C.c_void_p), ("accepting", C.c_void_p), ("live", C.c_void_p),
        ("vocab", C.c_int64),
        ("tok_bytes", C.c_void_p), ("n_bytes", C.c_int64), ("tok_ptr", C.c_void_p), ("skip", C.c_void_p),
        ("n", C.c_int64),
        ("tokens", C.c_void_p), ("ld", C.c_int64), ("from_", C.c_void_p), ("to", C.c_void_p),
        ("state_in", C.c_void_p), ("state_out", C.c_void_p),
        ("bank", C.c_void_p), ("bank_ld", C.c_int64), ("capacity", C.c_int64),
        ("row_of_state", C.c_void_p), ("work", C.c_void_p), ("counters", C.c_void_p),
        ("max_work", C.c_int64),
        ("done", C.c_void_p), ("out_rows", C.c_void_p),
    ]


class DfaWeightArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("dfa", DfaArgs),
        ("arc_logw", C.c_void_p), ("final_logw", C.c_void_p),
        ("wbank", C.c_void_p), ("wbank_ld", C.c_int64),
    ]


DFA_EVICT_COUNTERS = 4  # GLB_DFA_EVICT_COUNTERS: the call's claimants and rows taken, rows filled and rows evicted (cumulative)


class DfaEvictArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("dfa", DfaArgs),
        ("arc_logw", C.c_void_p), ("final_logw", C.c_void_p),
        ("wbank", C.c_void_p), ("wbank_ld", C.c_int64),
        ("row_state", C.c_void_p), ("row_stamp", C.c_void_p), ("claimants", C.c_void_p), ("victims", C.c_void_p),
        ("ecounters", C.c_void_p), ("epoch", C.c_void_p),
    ]


DFA_PUSH_STATUS = 8  # GLB_DFA_PUSH_STATUS: sweeps performed, converged, flags, sweeps of the last call, three marks, unused
DFA_PUSH_LOG, DFA_PUSH_MAX = 0, 1


class DfaPushArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_states", C.c_int32), ("start", C.c_int32), ("semiring", C.c_int32),
        ("delta", C.c_void_p), ("arc_logw", C.c_void_p), ("final_logw", C.c_void_p),
        ("beta", C.c_void_p), ("scratch", C.c_void_p), ("arc_out", C.c_void_p), ("final_out", C.c_void_p),
        ("status", C.c_void_p),
        ("sweeps", C.c_int32), ("restart", C.c_int32), ("tol", C.c_float),
    ]


DFA_MIN_STATUS = 8  # GLB_DFA_MIN_STATUS: rounds performed, converged, flags, classes, three rotating counts, rounds of the last call


class DfaMinArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_states", C.c_int32),
        ("delta", C.c_void_p), ("keep", C.c_void_p), ("final_bits", C.c_void_p), ("arc_bits", C.c_void_p),
        ("cls", C.c_void_p), ("scratch", C.c_void_p),
        ("table", C.c_void_p), ("table_slots", C.c_int64),
        ("status", C.c_void_p),
        ("rounds", C.c_int32), ("restart", C.c_int32),
        ("new_id", C.c_void_p), ("rep", C.c_void_p), ("n_new", C.c_int32),
        ("arc_logw", C.c_void_p), ("final_logw", C.c_void_p), ("accepting", C.c_void_p),
        ("delta_out", C.c_void_p), ("arc_out", C.c_void_p), ("final_out", C.c_void_p), ("accepting_out", C.c_void_p),
    ]


FSA_STATUS = 16  # GLB_FSA_STATUS: the search - rounds, converged, flags, states, frontier, private, count reached; [8 ..] liveness
FSA_LIVE_STATUS = 8  # where liveness keeps its words: sweeps, converged, flags (zero), private
FSA_AND, FSA_OR, FSA_SUB = 0, 1, 2
FSA_MAX_STATES = 1 << 22


class FsaProductArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("op", C.c_int32),
        ("n_a", C.c_int32), ("n_b", C.c_int32), ("start_a", C.c_int32), ("start_b", C.c_int32),
        ("delta_a", C.c_void_p), ("delta_b", C.c_void_p),
        ("accepting_a", C.c_void_p), ("accepting_b", C.c_void_p),
        ("live_a", C.c_void_p), ("live_b", C.c_void_p),
        ("arc_a", C.c_void_p), ("final_a", C.c_void_p),
        ("arc_b", C.c_void_p), ("final_b", C.c_void_p),
        ("max_states", C.c_int32),
        ("n_states", C.c_int32),
        ("table", C.c_void_p), ("table_slots", C.c_int64),
        ("pairs", C.c_void_p), ("delta_out", C.c_void_p), ("accepting_out", C.c_void_p),
        ("arc_out", C.c_void_p), ("final_out", C.c_void_p),
        ("live", C.c_void_p), ("counts", C.c_void_p), ("status", C.c_void_p),
        ("rounds", C.c_int32), ("restart", C.c_int32),
    ]


NFA_STATUS = 16  # GLB_NFA_STATUS: the search as FSA_STATUS has it; [8 ..] the closure - sweeps, converged, flags (zero), private
NFA_CLOSURE_STATUS = 8
NFA_MAX_IMPORTANT = 4096  # GLB_NFA_MAX_IMPORTANT: a set of important states is one wave, a 64-bit word a lane
NFA_MAX_STATES = 1 << 22


class NfaArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("n_states", C.c_int32), ("start", C.c_int32),
        ("n_important", C.c_int32), ("n_words", C.c_int32),
        ("n_arcs", C.c_int32), ("n_eps", C.c_int32), ("n_groups", C.c_int32),
        ("eps_off", C.c_void_p), ("eps_to", C.c_void_p), ("bit_of", C.c_void_p),
        ("arc_off", C.c_void_p), ("arc_dst", C.c_void_p), ("arc_bytes", C.c_void_p), ("accepting_mask", C.c_void_p),
        ("group_of", C.c_void_p), ("group_lo", C.c_void_p),
        ("eclose", C.c_void_p),
        ("hash_mask", C.c_uint64),
        ("max_states", C.c_int32), ("chunk", C.c_int32),
        ("table", C.c_void_p), ("table_slots", C.c_int64),
        ("cand", C.c_void_p), ("sets", C.c_void_p),
        ("delta_out", C.c_void_p), ("accepting_out", C.c_void_p), ("counts", C.c_void_p), ("status", C.c_void_p),
        ("rounds", C.c_int32), ("restart", C.c_int32),
    ]


LAZY_STATUS = 8  # GLB_LAZY_STATUS: states numbered, flags (sticky), the states numbered when the running call began, private
LAZY_OVERFLOW, LAZY_BUG = 1, 2


class LazyArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("dfa", DfaArgs),
        ("n_nfa_states", C.c_int32), ("nfa_start", C.c_int32),
        ("n_important", C.c_int32), ("n_words", C.c_int32),
        ("n_arcs", C.c_int32),
        ("max_states", C.c_int32),
        ("arc_off", C.c_void_p), ("arc_dst", C.c_void_p), ("arc_bytes", C.c_void_p), ("accepting_mask", C.c_void_p),
        ("eclose", C.c_void_p),
        ("hash_mask", C.c_uint64),
        ("table", C.c_void_p), ("table_slots", C.c_int64),
        ("cand", C.c_void_p), ("counts", C.c_void_p), ("cand_rows", C.c_int64),
        ("sets", C.c_void_p), ("accepting_out", C.c_void_p), ("status", C.c_void_p),
        ("row_state", C.c_void_p), ("row_stamp", C.c_void_p), ("claimants", C.c_void_p), ("victims", C.c_void_p),
        ("ecounters", C.c_void_p), ("epoch", C.c_void_p),
        ("force_wave", C.c_int32),
    ]


PDA_MAX_DEPTH = 504  # GLB_PDA_MAX_DEPTH: a configuration is one wave, a 64-bit word a lane: the head and 63 words of 8 symbols
PDA_STATUS = 8  # GLB_PDA_STATUS: configurations numbered, flags (sticky), those numbered when the running call began, private
PDA_OVERFLOW, PDA_BUG = 1, 2
PDA_MAX_SYMBOLS, PDA_POP = 126, 127  # an entry of delta: next | op << 24, op 0 (keep), 1 .. G (push), 127 (pop)


class PdaArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("dfa", DfaArgs),
        ("n_pda_states", C.c_int32), ("n_symbols", C.c_int32), ("start", C.c_int32),
        ("max_depth", C.c_int32), ("n_words", C.c_int32), ("max_states", C.c_int32),
        ("delta", C.c_void_p), ("accepting", C.c_void_p),
        ("hash_mask", C.c_uint64),
        ("table", C.c_void_p), ("table_slots", C.c_int64),
        ("cand", C.c_void_p), ("counts", C.c_void_p), ("cand_rows", C.c_int64),
        ("configs", C.c_void_p), ("accepting_out", C.c_void_p), ("status", C.c_void_p),
        ("row_state", C.c_void_p), ("row_stamp", C.c_void_p), ("claimants", C.c_void_p), ("victims", C.c_void_p),
        ("ecounters", C.c_void_p), ("epoch", C.c_void_p),
        ("max_token_bytes", C.c_int32),
    ]


CONJ_MAX_PARTS = 8  # GLB_CONJ_MAX_PARTS: a tuple of part states is at most four 64-bit words, two states a word
CONJ_STATUS = 8  # GLB_CONJ_STATUS: tuples numbered, flags (sticky), those numbered when the running call began, private
CONJ_OVERFLOW, CONJ_BUG = 1, 2


class ConjArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("dfa", DfaArgs),
        ("n_parts", C.c_int32), ("n_words", C.c_int32), ("max_states", C.c_int32),
        ("part_start", C.c_int32 * CONJ_MAX_PARTS),
        ("hash_mask", C.c_uint64),
        ("table", C.c_void_p), ("table_slots", C.c_int64),
        ("tuples", C.c_void_p), ("status", C.c_void_p),
        ("counts", C.c_void_p), ("cand_rows", C.c_int64),
        ("part_states", C.c_void_p), ("part_ld", C.c_int64),
        ("claim_states", C.c_void_p), ("rep", C.c_void_p),
        ("part_rows", C.c_void_p * CONJ_MAX_PARTS), ("part_bank", C.c_void_p * CONJ_MAX_PARTS),
        ("part_bank_ld", C.c_int64 * CONJ_MAX_PARTS), ("part_capacity", C.c_int64 * CONJ_MAX_PARTS),
        ("part_weighted", C.c_int32 * CONJ_MAX_PARTS),
        ("wbank", C.c_void_p), ("wbank_ld", C.c_int64),
        ("row_state", C.c_void_p), ("row_stamp", C.c_void_p), ("claimants", C.c_void_p), ("victims", C.c_void_p),
        ("ecounters", C.c_void_p), ("epoch", C.c_void_p),
    ]


class ImportanceArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("target", C.c_void_p), ("target_dtype", C.c_int32), ("ld_p", C.c_int64),
        ("proposal", C.c_void_p), ("proposal_dtype", C.c_int32), ("ld_q", C.c_int64),
        ("n_rows", C.c_int64), ("vocab", C.c_int64),
        ("proposal_scale", C.c_float),
        ("n_particles", C.c_int64), ("row_of", C.c_void_p),
        ("mask_kind", C.c_int32), ("mask", C.c_void_p), ("mask_ld", C.c_int64), ("n_masks", C.c_int64),
        ("mask_id", C.c_void_p), ("row_mask_id", C.c_void_p),
        ("seed", C.c_uint64), ("offset", C.c_uint64), ("particle_base", C.c_int64),
        ("out_token", C.c_void_p), ("out_dlogw", C.c_void_p), ("out_lse_target", C.c_void_p),
        ("out_logZ_proposal", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
    ]


IMPORTANCE_CHUNK = 4096  # vocabulary indices per chunk of glb_importance_step's two-stage draw
IMPORTANCE_RECORD_BYTES = 64  # workspace bytes per (unit, chunk)


class ScoreArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("logits", C.c_void_p), ("dtype", C.c_int32),
        ("n_rows", C.c_int64), ("vocab", C.c_int64), ("ld", C.c_int64),
        ("logit_scale", C.c_float),
        ("token", C.c_void_p),
        ("mask_kind", C.c_int32), ("mask", C.c_void_p), ("mask_ld", C.c_int64), ("n_masks", C.c_int64),
        ("row_mask_id", C.c_void_p),
        ("out_logp", C.c_void_p), ("out_lse", C.c_void_p), ("out_logZ", C.c_void_p), ("out_logp_masked", C.c_void_p),
        ("seq_start", C.c_void_p), ("n_seq", C.c_int64),
        ("out_seq_logp", C.c_void_p), ("out_seq_logZ", C.c_void_p), ("out_seq_logp_masked", C.c_void_p),
    ]


class TopkArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("logits", C.c_void_p), ("dtype", C.c_int32),
        ("n_rows", C.c_int64), ("vocab", C.c_int64), ("ld", C.c_int64),
        ("logit_scale", C.c_float), ("k", C.c_int32),
        ("mask_kind", C.c_int32), ("mask", C.c_void_p), ("mask_ld", C.c_int64), ("n_masks", C.c_int64),
        ("row_mask_id", C.c_void_p),
        ("out_token", C.c_void_p), ("out_logp", C.c_void_p), ("out_logp_masked", C.c_void_p),
        ("out_lse", C.c_void_p), ("out_logZ", C.c_void_p),
    ]


class ByteLmArgs(C.Structure):  # glb_bytelm_args
    _fields_ = [
        ("struct_size", C.c_uint32), ("width", C.c_int32),
        ("n_groups", C.c_int64), ("n_nodes", C.c_int64), ("root", C.c_int32),
        ("child_ptr", C.c_void_p), ("child_idx", C.c_void_p), ("child_sym", C.c_void_p), ("leaf_token", C.c_void_p),
        ("node", C.c_void_p), ("alive", C.c_void_p), ("u", C.c_void_p), ("w", C.c_void_p),
        ("sel", C.c_void_p), ("mass", C.c_void_p), ("fresh", C.c_void_p),
        ("out_parent", C.c_void_p), ("out_token", C.c_void_p), ("out_node", C.c_void_p), ("out_alive", C.c_void_p),
        ("out_u", C.c_void_p), ("out_w", C.c_void_p), ("out_spawned", C.c_void_p), ("out_n_spawned", C.c_void_p),
        ("byte", C.c_void_p), ("out_next", C.c_void_p), ("out_logZ", C.c_void_p), ("logp", C.c_void_p),
    ]


class ByteLmStepArgs(C.Structure):  # glb_bytelm_step_args
    _fields_ = [
        ("struct_size", C.c_uint32), ("peek", C.c_int32),
        ("beam", ByteLmArgs),
        ("n_states", C.c_int64),
        ("delta", C.c_void_p), ("accepting", C.c_void_p), ("live", C.c_void_p), ("arc_logw", C.c_void_p), ("final_logw", C.c_void_p),
        ("state", C.c_void_p), ("ended", C.c_void_p), ("log_weight", C.c_void_p), ("uniform", C.c_void_p),
        ("seed", C.c_uint64), ("offset", C.c_uint64),
        ("out_byte", C.c_void_p), ("out_row", C.c_void_p), ("out_logZc", C.c_void_p),
    ]


class TruncateArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("logits", C.c_void_p), ("dtype", C.c_int32),
        ("n_rows", C.c_int64), ("vocab", C.c_int64), ("ld", C.c_int64),
        ("logit_scale", C.c_float),
        ("mask_kind", C.c_int32), ("mask", C.c_void_p), ("mask_ld", C.c_int64), ("n_masks", C.c_int64),
        ("row_mask_id", C.c_void_p),
        ("top_k", C.c_int64), ("top_p", C.c_float), ("log_min_p", C.c_float),
        ("out_bits", C.c_void_p), ("out_ld", C.c_int64),
        ("out_threshold", C.c_void_p), ("out_kept", C.c_void_p), ("out_logmass", C.c_void_p),
    ]


# every symbol include/glb.h declares: name -> (restype, argtypes)
_vp, _i32, _i64, _f32, _sz = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_size_t
SYMBOLS = {
    "glb_version": (C.c_char_p, []),
    "glb_abi_version": (C.c_int, []),
    "glb_last_error": (C.c_int, [C.c_char_p, _sz]),
    "glb_device_count": (C.c_int, []),
    "glb_step_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64]),
    "glb_logprob_mask_sample": (C.c_int, [C.POINTER(StepArgs), _vp]),
    "glb_logprob_mask_sample_timed": (C.c_int, [C.POINTER(StepArgs), _vp, _vp, _vp]),
    "glb_workspace_init": (C.c_int, [_vp, _sz, _vp]),
    "glb_workspace_release": (C.c_int, [_vp]),
    "glb_workspace_check": (C.c_int, [_vp, _vp]),
    "glb_workspace_error_word": (_vp, [_vp]),
    "glb_set_spin_limit": (C.c_int, [C.c_uint64]),
    "glb_mask_prepared_bytes": (_sz, [_i64, _i64]),
    "glb_mask_prepare": (C.c_int, [_vp, _i64, _i64, _i64, _i32, _vp, _sz, _vp]),
    "glb_mask_prepare_rows": (C.c_int, [_vp, _i64, _i64, _i64, _i32, _vp, _i64, _vp, _sz, _vp]),
    "glb_log_softmax_workspace_bytes": (_sz, [_i64, _i64]),
    "glb_log_softmax_rows": (C.c_int, [_vp, _i32, _i64, _i64, _i64, _f32, _vp, _i32, _i64, _vp, _vp, _sz, _vp]),
    "glb_mask_f32_to_bits": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp]),
    "glb_group_contexts_workspace": (_sz, [_i64]),
    "glb_group_contexts": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "glb_hash_contexts": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _vp]),
    "glb_match_prefixes": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "glb_gather_padded": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp]),
    "glb_gather_kv_padded": (C.c_int, [_vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _vp]),
    "glb_particles_advance": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp]),
    "glb_normalize_weights": (C.c_int, [_vp, _i64, _vp, _vp, _vp]),
    "glb_kv_append": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _vp]),
    "glb_kv_gather_rows": (C.c_int, [_vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _i32, _vp]),
    "glb_gather_rows_i32": (C.c_int, [_vp, _i64, _vp, _i64, _i64, _vp, _i64, _vp]),
    "glb_match_rows": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp]),
    "glb_slab_attention": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64,
                                     _f32, _i32, _vp, _vp]),
    "glb_short_attention": (C.c_int, [_vp, C.POINTER(C.c_int64), _vp, C.POINTER(C.c_int64), _vp, C.POINTER(C.c_int64), _vp, _i64, _i64,
                                      _i64, _i64, _i64, _i64, _i64, _i64, _f32, _i32, _vp, _vp]),
    "glb_short_attention_packed": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _i64, _i64,
                                             _i64, _f32, _i32, _vp, _vp, _vp]),
    "glb_kv_plan_workspace": (_sz, [_i64, _i64]),
    "glb_kv_plan": (C.c_int, [C.POINTER(KvPlanArgs), _vp]),
    "glb_match_prefix_rows": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp]),
    "glb_kv_plan_chunk": (C.c_int, [C.POINTER(KvPlanChunkArgs), _vp]),
    "glb_slab_attention_chunk": (C.c_int, [_vp, C.POINTER(C.c_int64), _vp, C.POINTER(C.c_int64), _vp, C.POINTER(C.c_int64), _vp, _vp,
                                           _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _f32, _i32, _vp, _vp]),
    "glb_trie_workspace": (_sz, [_i64, _i64]),
    "glb_trie_reduce": (C.c_int, [_vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _i64, _vp, _sz,
                                  _vp]),
    "glb_trie_workspace_ex": (_sz, [_i64, _i64]),
    "glb_trie_masses": (C.c_int, [C.POINTER(TrieArgs), _vp]),
    "glb_trie_rows_workspace": (_sz, [_i64, C.POINTER(TriePlan)]),
    "glb_trie_rows": (C.c_int, [C.POINTER(TrieRowsArgs), C.POINTER(TriePlan), _vp]),
    "glb_resample_workspace": (_sz, [_i64]),
    "glb_resample_systematic": (C.c_int, [_vp, _i64, C.c_uint64, C.c_uint64, _vp, _vp, _vp, _sz, _vp]),
    "glb_mt19937_seed": (None, [C.POINTER(MT19937), C.c_uint64]),
    "glb_mt19937_exponential_f32": (C.c_int, [C.POINTER(MT19937), _vp, _i64]),
    "glb_mt19937_window": (C.c_int, [C.c_uint64, _vp]),
    "glb_mt19937_jump_polys": (C.c_int, [_i64, _i32, _i32, _vp]),
    "glb_mt19937_jump_host": (C.c_int, [_vp, _vp, _vp]),
    "glb_mt19937_rows_workspace": (_sz, [_i64, _i32]),
    "glb_mt19937_exponential_rows": (C.c_int, [C.POINTER(MtRowsArgs), _vp]),
    "glb_comm_unique_id": (C.c_int, [_vp]),
    "glb_comm_init": (C.c_int, [_vp, _i32, _i32, C.POINTER(C.c_void_p)]),
    "glb_allgather_f32": (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    "glb_comm_destroy": (C.c_int, [_vp]),
    "glb_gemm_split_bytes": (_sz, [_i64, _i64]),
    "glb_gemm_split_weights": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _sz, _vp]),
    "glb_gemm_f32_split": (C.c_int, [C.POINTER(GemmArgs), _vp]),
    "glb_gemm_split_pick": (C.c_int, [_i64, _i64, _i64, C.c_int, C.POINTER(C.c_int)]),
    "glb_gemm_f32_split_form": (C.c_int, [C.POINTER(GemmArgs), C.c_int, _vp]),
    "glb_gemm_f32_split_residual": (C.c_int, [C.POINTER(GemmArgs), _vp, _i64, C.c_int, _vp]),
    "glb_packed_plan": (C.c_int, [C.POINTER(PackedPlanArgs), _vp]),
    "glb_gemm_split_blocks_per_cu": (C.c_int, [C.c_int, C.POINTER(C.c_int)]),
    "glb_gemm_split_form_blocks_per_cu": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "glb_lora_merge_workspace_bytes": (_sz, [_i32]),
    "glb_lora_merge": (C.c_int, [C.POINTER(LoraJob), _i32, _vp, _sz, _vp]),
    "glb_lora_rows_table_bytes": (_sz, [_i32, _i32]),
    "glb_lora_rows_table_upload": (C.c_int, [C.POINTER(LoraRowsEntry), _i32, _i32, _vp, _sz, _vp]),
    "glb_lora_rows_workspace_bytes": (_sz, [_i64, _i32]),
    "glb_lora_rows": (C.c_int, [C.POINTER(LoraRowsArgs), _vp]),
    "glb_w4_bytes": (_sz, [_i64, _i64]),
    "glb_w4_quantize": (C.c_int, [C.POINTER(W4Args), _vp]),
    "glb_w4_dequantize": (C.c_int, [C.POINTER(W4Args), _vp]),
    "glb_w4_gemm_max_rows": (C.c_int, []),
    "glb_w4_gemm_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "glb_w4_gemm": (C.c_int, [C.POINTER(W4GemmArgs), _vp]),
    "glb_dfa_bank_init": (C.c_int, [C.POINTER(DfaArgs), _vp]),
    "glb_dfa_advance": (C.c_int, [C.POINTER(DfaArgs), _vp]),
    "glb_dfa_claim_rows": (C.c_int, [C.POINTER(DfaArgs), _vp]),
    "glb_dfa_fill_masks": (C.c_int, [C.POINTER(DfaArgs), _vp]),
    "glb_dfa_mask_ids": (C.c_int, [C.POINTER(DfaArgs), _vp]),
    "glb_dfa_bank_rows": (_i64, [_sz, _i64, _i64]),
    "glb_dfa_weight_bank_init": (C.c_int, [C.POINTER(DfaWeightArgs), _vp]),
    "glb_dfa_fill_weights": (C.c_int, [C.POINTER(DfaWeightArgs), _vp]),
    "glb_dfa_weight_bank_rows": (_i64, [_sz, _i64, _i64]),
    "glb_dfa_evict_bank_init": (C.c_int, [C.POINTER(DfaEvictArgs), _vp]),
    "glb_dfa_evict_serve": (C.c_int, [C.POINTER(DfaEvictArgs), _vp]),
    "glb_dfa_backward": (C.c_int, [C.POINTER(DfaPushArgs), _vp]),
    "glb_dfa_push_weights": (C.c_int, [C.POINTER(DfaPushArgs), _vp]),
    "glb_dfa_refine": (C.c_int, [C.POINTER(DfaMinArgs), _vp]),
    "glb_dfa_quotient": (C.c_int, [C.POINTER(DfaMinArgs), _vp]),
    "glb_fsa_product_round": (C.c_int, [C.POINTER(FsaProductArgs), _vp]),
    "glb_fsa_live": (C.c_int, [C.POINTER(FsaProductArgs), _vp]),
    "glb_nfa_closure": (C.c_int, [C.POINTER(NfaArgs), _vp]),
    "glb_nfa_subset_round": (C.c_int, [C.POINTER(NfaArgs), _vp]),
    "glb_lazy_init": (C.c_int, [C.POINTER(LazyArgs), _vp]),
    "glb_lazy_advance": (C.c_int, [C.POINTER(LazyArgs), _vp]),
    "glb_lazy_serve": (C.c_int, [C.POINTER(LazyArgs), _vp]),
    "glb_pda_init": (C.c_int, [C.POINTER(PdaArgs), _vp]),
    "glb_pda_advance": (C.c_int, [C.POINTER(PdaArgs), _vp]),
    "glb_pda_serve": (C.c_int, [C.POINTER(PdaArgs), _vp]),
    "glb_conj_init": (C.c_int, [C.POINTER(ConjArgs), _vp]),
    "glb_conj_unpack": (C.c_int, [C.POINTER(ConjArgs), _vp]),
    "glb_conj_number": (C.c_int, [C.POINTER(ConjArgs), _vp]),
    "glb_conj_serve": (C.c_int, [C.POINTER(ConjArgs), _vp]),
    "glb_importance_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "glb_importance_step": (C.c_int, [C.POINTER(ImportanceArgs), _vp]),
    "glb_score_rows": (C.c_int, [C.POINTER(ScoreArgs), _vp]),
    "glb_score_seq_sums": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp]),
    "glb_topk_rows": (C.c_int, [C.POINTER(TopkArgs), _vp]),
    "glb_truncate_rows": (C.c_int, [C.POINTER(TruncateArgs), _vp]),
    "glb_beam_select": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp]),
    "glb_bytelm_children": (C.c_int, [C.POINTER(ByteLmArgs), _vp]),
    "glb_bytelm_extend": (C.c_int, [C.POINTER(ByteLmArgs), _vp]),
    "glb_bytelm_next": (C.c_int, [C.POINTER(ByteLmArgs), _vp]),
    "glb_bytelm_step": (C.c_int, [C.POINTER(ByteLmStepArgs), _vp]),
    "glb_philox4x32_10": (None, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
}

_lib = None


def load():
    """Load libglb_hip.so and bind every symbol.  Raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with `make -C genlm-backend_amd/csrc -j8` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback."
        )
    # torch first: it brings its own HIP runtime, and the runtime that is loaded first serves the process - loading
    # this library (linked against /opt/rocm's) ahead of torch leaves torch.cuda unable to find the device
    import torch  # noqa: F401

    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the ABI is incomplete
        fn.restype = res
        fn.argtypes = args
    if lib.glb_abi_version() != ABI_VERSION:
        raise ImportError(f"libglb_hip.so ABI {lib.glb_abi_version()} != {ABI_VERSION}")
    _lib = lib
    return lib


def last_error():
    buf = C.create_string_buffer(512)
    load().glb_last_error(buf, 512)
    return buf.value.decode()


def check(rc):
    if rc != GLB_OK:
        raise GlbError(rc, last_error())
