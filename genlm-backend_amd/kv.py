"""Device-resident KV state of the hot path.

* `SlabKV` — per-particle KV in preallocated slabs `[n, heads, cap, head_dim]`, one pair per layer, handed to the
  HuggingFace forward as a `Cache`.  The reference keeps KV as per-query tuples that are zero-padded and concatenated
  for every batch (hf.py:33-53,247-271) or as per-token slices on trie nodes (cache.py:103-191, mlx.py:177-318); here a
  particle owns row i of every slab, the new token's K/V is written in place at its own position (glb_kv_append:
  ragged lengths, no torch.cat regrow) and a resampling step is one gather launch over all layers
  (glb_kv_gather_rows) into the second slab set.
* `SlabRunner` — the slabs of one population and the forwards over them: executes the block table glb_kv_plan decided
  (`DeviceSIS._step_shared_kv`, `autokv.AutoKV`).
* `PrefixTable` — the device table of cached prompt prefixes and the `DynamicCache` a batch that uses them is run with.
* `encode_ragged` — the one forward that ENCODES a selection of a ragged batch (padded gather, body, last rows, K / V):
  every re-encoding path of `AsyncAmdLM`, `DeviceSIS` and `SlabRunner.run`'s rows of kind B goes through it.
* `encode_packed` — the same encoding ROW-PACKED for contexts that are a shared prompt plus a short tail: every prompt's
  rows once per forward (`PromptGroups`, `PackedKV`, glb_short_attention_packed).
* `PrefixLRU` — byte-budgeted least-recently-used store for the prompt prefixes `cache_kv` pins (hf.py:155-164);
  the eviction policy of cache.py:103-191 (`DynamicTokenTrie`), applied to whole prefix slabs.
"""
import gc
import itertools
from collections import OrderedDict

import numpy as np
import torch
from transformers.cache_utils import Cache, CacheLayerMixin, DynamicCache


# ---- the attention kernels of the path behind transformers' attention interface -----------------------------------------
# Registered under one name; AsyncAmdLM points the configuration of its SHADOW of the model (fuse.shadow_model - never the
# caller's own configuration) at it.  Two forwards of the hot path are served by this library's kernels - the in-place
# one-token forward over KV slab rows (glb_slab_attention: append fused, no mask tensor) and the padded batches of short
# contexts (glb_short_attention: a dozen tokens per row, where the library SDPA kernels spend a fifth of the step) - and
# everything else (long sequences, dropout, training / autograd, exotic masks, CPU runs) goes to transformers' own SDPA
# path exactly as before.  No module-level state: the engine rides on the shadow configuration (`_glb_engine`), the slab
# layer of a running in-place forward on the key tensor `Cache.update` returned (`_glb_layer`).
_ATTN_NAME = "glb"
SHORT_ATTENTION_MAX = 4096  # q_len * k_len up to which glb_short_attention is used


def _glb_attention_forward(module, query, key, value, attention_mask, dropout=0.0, scaling=None, **kwargs):
    from transformers.integrations.sdpa_attention import sdpa_attention_forward

    layer = getattr(key, "_glb_layer", None)
    if layer is not None and layer._new_k is not None and getattr(layer.owner, "n_new", None) is not None:
        # a chunk forward over slab rows (SharedSlabKV.set_forward_chunk): up to 16 new tokens per row, appended by the kernel
        if key is not layer.keys or value is not layer.values:
            raise RuntimeError("glb_slab_attention_chunk: the attention module changed the key / value tensors the KV slab "
                               "handed out: the new tokens were never appended")
        k_new, v_new, layer._new_k, layer._new_v = layer._new_k, layer._new_v, None, None
        o = layer.owner
        scale = scaling if scaling is not None else query.shape[-1] ** -0.5
        return o.engine.slab_attention_chunk(query, k_new, v_new, layer.keys, layer.values, o.pos, o.n_new, scale, rows=o.rows), None
    if layer is not None and layer._new_k is not None:
        # an in-place forward whose append is this kernel's job: the new token's K / V are only in the stash
        if key is not layer.keys or value is not layer.values or query.shape[2] != 1:
            raise RuntimeError("glb_slab_attention: the attention module changed the key / value tensors the KV slab handed "
                               "out (or feeds more than one token): the new token was never appended - run this model with "
                               "SlabForward(fused_attention=False)")
        k_new, v_new, layer._new_k, layer._new_v = layer._new_k, layer._new_v, None, None
        o = layer.owner
        scale = scaling if scaling is not None else query.shape[-1] ** -0.5
        return o.engine.slab_attention(query, k_new, v_new, layer.keys, layer.values, o.pos, scale), None
    packed = getattr(key, "_glb_packed", None)
    if packed is not None:
        # a row-packed forward (encode_packed): batch 1, the M rows of every prompt and every tail; q / k / v are read where
        # c_attn left them and the output is [M, H * Dh] already - no transpose, no copy
        if query.shape[0] != 1 or key.shape[2] != query.shape[2] or query.shape[2] != packed.n_rows or value.shape != key.shape:
            raise RuntimeError("glb_short_attention_packed: the attention module changed the shape of the packed batch")
        scale = scaling if scaling is not None else query.shape[-1] ** -0.5
        out = packed.engine.short_attention_packed(query[0].transpose(0, 1), key[0].transpose(0, 1), value[0].transpose(0, 1),
                                                   packed.segments, packed.max_keys, scale)
        packed.served += 1
        return out.unsqueeze(0), None
    eng = getattr(getattr(module, "config", None), "_glb_engine", None)
    Lq, Lk = query.shape[2], key.shape[2]
    # the kernels write into fresh tensors outside autograd: a forward that may be differentiated keeps the SDPA path
    wants_grad = torch.is_grad_enabled() and (query.requires_grad or key.requires_grad or value.requires_grad)
    if (eng is not None and query.is_cuda and not dropout and not wants_grad and not getattr(module, "training", False)
            and Lq * Lk <= SHORT_ATTENTION_MAX and Lk >= Lq
            and eng.slab_attention_supports(query.dtype, query.shape[-1]) and key.dtype == query.dtype == value.dtype
            and query.stride(3) == 1 and key.stride(3) == 1 and value.stride(3) == 1
            and kwargs.get("is_causal", True) is not False and not kwargs.get("softcap") and not kwargs.get("sliding_window")
            and getattr(module, "is_causal", True)
            and (attention_mask is None or (attention_mask.dtype == torch.bool and attention_mask.dim() == 4
                                            and attention_mask.shape[1] == 1 and attention_mask.shape[-1] == Lk
                                            and attention_mask.stride(3) == 1))
            and all((st * query.element_size()) % 16 == 0 for t in (query, key, value) for st in t.stride()[:3])
            and all(t.data_ptr() % 16 == 0 for t in (query, key, value))):
        scale = scaling if scaling is not None else query.shape[-1] ** -0.5
        return eng.short_attention(query, key, value, attention_mask, scale), None
    return sdpa_attention_forward(module, query, key, value, attention_mask, dropout=dropout, scaling=scaling, **kwargs)


def _register_attention():
    from transformers.masking_utils import ALL_MASK_ATTENTION_FUNCTIONS
    from transformers.modeling_utils import ALL_ATTENTION_FUNCTIONS

    if _ATTN_NAME not in ALL_ATTENTION_FUNCTIONS:
        ALL_ATTENTION_FUNCTIONS.register(_ATTN_NAME, _glb_attention_forward)
        ALL_MASK_ATTENTION_FUNCTIONS.register(_ATTN_NAME, ALL_MASK_ATTENTION_FUNCTIONS["sdpa"])


def use_glb_attention(shadow, engine):
    """Point a SHADOW of a transformers model (fuse.shadow_model: its configuration is a private copy) whose attention goes
    through the attention interface as "sdpa" at this library's attention kernels; returns whether it was done."""
    cfg = getattr(shadow, "config", None)
    if cfg is not None and getattr(cfg, "_attn_implementation", None) == _ATTN_NAME:
        return getattr(cfg, "_glb_engine", None) is engine
    if (cfg is None or not hasattr(engine, "short_attention") or getattr(cfg, "_attn_implementation", None) != "sdpa"
            or getattr(cfg, "attn_logit_softcapping", None) or getattr(cfg, "sliding_window", None)
            or getattr(cfg, "scale_attn_by_inverse_layer_idx", False)):
        return False
    _register_attention()
    cfg._attn_implementation = _ATTN_NAME
    cfg._glb_engine = engine
    return True


class _SlabLayer(CacheLayerMixin):
    """One layer's K / V slabs.  `update` appends one token per row at `owner.pos` and returns the whole slabs; which
    positions a row may attend to is the 2-D attention mask's business (`SlabKV.attention_mask`)."""

    is_compileable = False
    is_sliding = False

    def __init__(self, owner, idx):
        super().__init__()
        self.owner, self.idx = owner, idx
        self._new_k = self._new_v = None

    def lazy_initialization(self, key_states, value_states):
        o = self.owner
        shape_k = (o.n, key_states.shape[1], o.cap, key_states.shape[-1])
        shape_v = (o.n, value_states.shape[1], o.cap, value_states.shape[-1])
        self.keys = torch.zeros(shape_k, dtype=key_states.dtype, device=key_states.device)
        self.values = torch.zeros(shape_v, dtype=value_states.dtype, device=value_states.device)
        self.is_initialized = True

    def update(self, key_states, value_states, *args, **kwargs):
        if not self.is_initialized:
            self.lazy_initialization(key_states, value_states)
        o = self.owner
        if key_states.shape[0] != o.n or key_states.shape[-2] != 1:
            raise ValueError("SlabKV takes one new token for every particle per forward")
        if o.fused_attention:  # glb_slab_attention appends: it gets the new K / V where the projection left them
            self._new_k, self._new_v = key_states, value_states
            self.keys._glb_layer = self  # (how the attention entry finds this layer: no module-level state)
            return self.keys, self.values
        o.engine.kv_append(self.keys, key_states, o.pos)
        o.engine.kv_append(self.values, value_states, o.pos)
        return self.keys, self.values

    def get_mask_sizes(self, query_length):
        return self.owner.cap, 0

    def get_seq_length(self):
        return self.owner.cap - 1  # the query sits "after" every slot: causality is expressed by the 2-D mask alone

    def get_max_length(self):
        return self.owner.cap


class SlabKV(Cache):
    def __init__(self, engine, n, cap, n_layers):
        self.engine, self.n, self.cap = engine, n, cap
        self.pos = None  # int32 [n] device: where this forward's token goes (= tokens already held by the row)
        self.fused_attention = False  # the running forward's attention appends (SlabForward sets it per call)
        super().__init__(layers=[_SlabLayer(self, i) for i in range(n_layers)])
        self._alt = None
        self._ptrs = None

    # ---- forward-side helpers ----------------------------------------------------------------------------------
    def set_forward_in_place(self, pos):
        """pos: int32 [n] device - where every row's token of the next forward goes."""
        self.pos = pos

    def attention_mask(self, pos):
        """[n, cap] 0/1: row i sees its `pos[i]` cached tokens and the one being appended at `pos[i]`."""
        ar = torch.arange(self.cap, device=pos.device, dtype=pos.dtype)
        return (ar[None, :] <= pos[:, None]).to(torch.int64)

    # ---- slab plumbing ---------------------------------------------------------------------------------------------
    def _alloc_like(self, prompt_layers):
        for layer, (k, v) in zip(self.layers, prompt_layers):
            if not layer.is_initialized:
                layer.lazy_initialization(k[:1], v[:1])

    def _tensors(self, which):
        return [t for layer in which for t in (layer.keys, layer.values)]

    def fill_rows(self, src_layers, src_row_of, len_of):
        """Rows i with src_row_of[i] >= 0 take the first len_of[i] positions of row src_row_of[i] of `src_layers`
        ([(K, V)] per layer, each [u, heads, l_src, head_dim], contiguous): fan-out of freshly encoded contexts."""
        self._alloc_like(src_layers)
        srcs = [t for kv in src_layers for t in kv]
        self.engine.kv_gather_rows(srcs, self._tensors(self.layers), src_row_of, len_of, srcs_stable=False)

    def gather(self, src_row_of, len_of):
        """Resampling: row i becomes a copy of row src_row_of[i] (first len_of[i] positions); rows with
        src_row_of[i] < 0 are left to be refilled by the caller.  Works into the second slab set, then swaps."""
        cur = self._tensors(self.layers)
        if self._alt is None:
            self._alt = [torch.zeros_like(t) for t in cur]
        self.engine.kv_gather_rows(cur, self._alt, src_row_of, len_of)
        for j, layer in enumerate(self.layers):
            layer.keys, self._alt[2 * j] = self._alt[2 * j], layer.keys
            layer.values, self._alt[2 * j + 1] = self._alt[2 * j + 1], layer.values

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in self._tensors(self.layers) if t is not None) * (2 if self._alt else 1)


class _SharedLayer(_SlabLayer):
    """One layer of `SharedSlabKV`: the forward's batch row u lives in slab row `owner.rows[u]`; attention reads the
    forward's rows from the staging slabs `owner.stage()` filled them into."""

    def lazy_initialization(self, key_states, value_states):
        o = self.owner
        for name, st in (("keys", key_states), ("values", value_states)):
            shape = (o.n, st.shape[1], o.cap, st.shape[-1])
            setattr(self, name, torch.zeros(shape, dtype=st.dtype, device=st.device))
            setattr(self, "stage_" + name, torch.zeros(shape, dtype=st.dtype, device=st.device))
        self.is_initialized = True

    def update(self, key_states, value_states, *args, **kwargs):
        o = self.owner
        eng = o.engine
        if o.in_place:  # the forward's batch IS the slab: row b's token goes to row b, attention reads the slabs
            if key_states.shape[0] != o.n or key_states.shape[-2] != 1:
                raise ValueError("an in-place forward takes one token for every slab row")
            if o.fused_attention:
                self._new_k, self._new_v = key_states, value_states
                self.keys._glb_layer = self
                return self.keys, self.values
            eng.kv_append(self.keys, key_states, o.pos)
            eng.kv_append(self.values, value_states, o.pos)
            return self.keys, self.values
        U = o.rows.numel()
        if o.n_new is not None:  # a chunk forward: row u's tokens t < n_new[u] go to positions pos[u] + t of slab row rows[u]
            T = key_states.shape[-2]
            if key_states.shape[0] != U:
                raise ValueError("a chunk forward takes the rows SharedSlabKV.set_forward_chunk named")
            if o.fused_attention:  # glb_slab_attention_chunk appends and reads the rows where they lie
                self._new_k, self._new_v = key_states, value_states
                self.keys._glb_layer = self
                return self.keys, self.values
            for t in range(T):  # (a position of -1 appends nothing: the padding behind a row's last new token)
                at = torch.where(o.n_new > t, o.pos + t, torch.full_like(o.pos, -1))
                for slab, stage, new in ((self.keys, self.stage_keys, key_states), (self.values, self.stage_values, value_states)):
                    eng.kv_append(slab, new[:, :, t:t + 1], at, rows=o.rows)
                    eng.kv_append(stage, new[:, :, t:t + 1], at, rows=o.ident[:U])
            return self.stage_keys[:U], self.stage_values[:U]
        if key_states.shape[0] != U or key_states.shape[-2] != 1:
            raise ValueError("SharedSlabKV takes one new token for every row of the forward")
        # the new token's K / V: into the row that keeps it, and beside the gathered prefix the attention reads
        eng.kv_append(self.keys, key_states, o.pos, rows=o.rows)
        eng.kv_append(self.values, value_states, o.pos, rows=o.rows)
        eng.kv_append(self.stage_keys, key_states, o.pos, rows=o.ident[:U])
        eng.kv_append(self.stage_values, value_states, o.pos, rows=o.ident[:U])
        return self.stage_keys[:U], self.stage_values[:U]


class SharedSlabKV(SlabKV):
    """KV rows SHARED between particles (the reference's per-token KV on trie nodes, cache.py:103-191,
    restated for a population): `n` slab rows of `cap` positions, a block table outside (DeviceSIS.row_of) that maps
    particles to rows.  Particles with the same context point to ONE row and one forward row serves them all; when a
    shared row's particles draw different tokens, one keeps the row and the others get a copy of the prefix into free
    rows (copy-on-append, one gather launch over all layers); resampling re-points particles to their ancestors' rows
    and copies nothing.  A forward names its batch's rows (`set_forward`): one gather launch brings their prefixes - all
    layers, K and V - into staging slabs in batch order (the PyTorch attention wants a dense [U, H, cap, Dh]), the new
    token's K / V go into the row that keeps them and beside the gathered prefix."""

    def __init__(self, engine, n_rows, cap, n_layers):
        Cache.__init__(self, layers=[_SharedLayer(self, i) for i in range(n_layers)])
        self.engine, self.n, self.cap = engine, n_rows, cap
        self.pos = None
        self.fused_attention = False
        self.rows = None   # int32 [U]: slab row of every forward row
        self.ident = None  # int32 arange(n)
        self.in_place = False
        self.n_new = None  # int32 [U]: tokens per row of a chunk forward (None: a one-token forward)
        self._alt = None
        self._ptrs = None

    def set_forward_chunk(self, rows, pos, n_new, fused):
        """The next forward feeds row u the n_new[u] <= T tokens at positions pos[u] .. of slab row rows[u] (int32 [U]
        device, batch [U, T], right-padded).  fused: glb_slab_attention_chunk serves it on the rows where they lie; else the
        prefixes are gathered into the staging slabs for the SDPA path (`attention_mask(pos, n_new, T)`)."""
        if fused:
            self.rows, self.pos, self.in_place = rows, pos, False
        else:
            self.set_forward(rows, pos)
        self.n_new = n_new

    def attention_mask(self, pos, n_new=None, T=None, additive_dtype=None):
        """One-token forward: SlabKV's [n, cap] 0/1 mask.  Chunk forward: [U, 1, T, cap], query t of row u sees positions
        0 .. pos[u] + min(t, n_new[u] - 1) (a padded query sees what the row's last token sees: never an empty row) - bool,
        or with `additive_dtype` 0 / most-negative (attention code that adds its mask)."""
        if n_new is None:
            return super().attention_mask(pos)
        t = torch.minimum(torch.arange(T, device=pos.device, dtype=pos.dtype)[None, :], n_new[:, None] - 1)
        last = pos[:, None] + t  # [U, T]
        ar = torch.arange(self.cap, device=pos.device, dtype=pos.dtype)
        see = (ar[None, None, :] <= last[:, :, None])[:, None]
        if additive_dtype is None:
            return see
        return torch.zeros(see.shape, dtype=additive_dtype, device=pos.device).masked_fill_(~see, torch.finfo(additive_dtype).min)

    def set_forward(self, rows, pos):
        """rows, pos: int32 [U] device.  Gathers the U prefixes (pos[u] positions of row rows[u]) into the staging slabs."""
        self.rows, self.pos, self.in_place, self.n_new = rows, pos, False, None
        U = rows.numel()
        if self.ident is None:
            self.ident = torch.arange(self.n, dtype=torch.int32, device=rows.device)
        src_row_of = torch.full((self.n,), -1, dtype=torch.int32, device=rows.device)
        src_row_of[:U] = rows
        len_of = torch.zeros(self.n, dtype=torch.int32, device=rows.device)
        len_of[:U] = pos
        slabs = self._tensors(self.layers)
        stage = [t for layer in self.layers for t in (layer.stage_keys, layer.stage_values)]
        self.engine.kv_gather_rows(slabs, stage, src_row_of, len_of)

    def set_forward_in_place(self, pos):
        """The next forward runs on ALL slab rows where they lie (batch row b = slab row b, pos: int32 [n] device, the
        position row b's token is appended at): no gather.  Worth it when most rows are live - a free row costs a
        forward row whose result nobody reads, the gather costs every live row's whole prefix, read and written."""
        self.rows, self.pos, self.in_place, self.n_new = None, pos, True, None

    def copy_rows(self, src_row_of, len_of):
        """Row r with src_row_of[r] >= 0 takes the first len_of[r] positions of row src_row_of[r] (in place: sources
        are live rows, destinations free ones)."""
        cur = self._tensors(self.layers)
        self.engine.kv_gather_rows(cur, cur, src_row_of, len_of)

    def nbytes(self):
        return 2 * sum(t.numel() * t.element_size() for t in self._tensors(self.layers) if t is not None)


class SlabForward:
    """The one-token forward over ALL rows of a `SlabKV` / `SharedSlabKV` where they lie (`set_forward_in_place`).  Its
    shapes never change - batch = the slab's rows, one token each, the mask a function of the positions - so after two
    eager calls the launch sequence (the transformer body's kernels and this library's glb_kv_append launches between
    them) is captured into a hipGraph once and replayed from static input buffers: same kernels, same bits, without
    the host walking the model's Python for every step (GPT-2-small, 1024 rows: 4.1 -> 3.4 ms; Llama-3.2-1B shape, 512
    rows: 10.4 -> 7.2 ms).  A graph belongs to the slab tensors it was captured over (a resampling `gather` swaps slab
    sets: one graph each).  `graph=False` (or a CPU device) keeps every call eager."""

    def __init__(self, pkv, body, graph=True, fused_attention=True, owner=None):
        self.pkv, self.body = pkv, body
        self.owner = owner  # the AsyncAmdLM whose `refresh_weights()` drops the captured graphs (its weights_epoch moves)
        self._owner_epoch = getattr(owner, "weights_epoch", 0)
        self.graph_ok = bool(graph) and torch.cuda.is_available()
        self.calls = 0
        self.graphs = {}  # identity of the slab set -> (graph, ids, pos, hidden, the slab tensors themselves)
        # weights the shadow keeps derived copies of (fuse._merged_qkv): a captured graph reads the copy it was captured
        # with, so the graphs are dropped when one of the sources changes
        # (a 4-bit projection - quant.W4Linear - has no .weight and no derived copy)
        self._watched = [p.weight for mod in body.modules() if hasattr(mod, "q_proj") and hasattr(mod, "k_proj") and hasattr(mod, "v_proj")
                         for p in (mod.q_proj, mod.k_proj, mod.v_proj) if hasattr(p, "weight")]
        self._watched += [p.weight for mod in body.modules() if hasattr(mod, "gate_proj") and hasattr(mod, "up_proj")
                          for p in (mod.gate_proj, mod.up_proj) if hasattr(p, "weight")]
        self._watched += [mod.weight for mod in body.modules() if type(mod).__name__ == "SplitConv1D"]  # (fuse.py)
        self._watched_version = self._weights_version()
        # glb_slab_attention instead of two appends + a mask + a dense SDPA call per layer: for models whose attention
        # goes through transformers' attention interface with plain softmax(q k^T * scale) v semantics on a HIP device
        cfg = getattr(body, "config", None)
        k0 = pkv.layers[0].keys if pkv.layers and getattr(pkv.layers[0], "is_initialized", False) else None
        # (the body is AsyncAmdLM's shadow of the model, already pointed at the "glb" attention entry when glb_attention is on;
        # a body that is not - the caller's own model, glb_attention=False - keeps appends + mask + SDPA)
        self.fused = bool(fused_attention and cfg is not None and k0 is not None and k0.is_cuda
                          and hasattr(pkv.engine, "slab_attention")
                          and pkv.engine.slab_attention_supports(k0.dtype, k0.shape[-1])
                          and getattr(cfg, "_attn_implementation", None) == _ATTN_NAME
                          and getattr(cfg, "_glb_engine", None) is pkv.engine)

    def _weights_version(self):
        return sum(t._version for t in self._watched)

    def _run(self, ids, pos):
        pkv = self.pkv
        pkv.set_forward_in_place(pos)
        if self.fused:
            pkv.fused_attention = True
            try:  # (no mask: the kernel attends to positions 0 .. pos[r] and nothing else)
                out = self.body(input_ids=ids, position_ids=pos.view(-1, 1).long(), attention_mask=None,
                                past_key_values=pkv, use_cache=True)
            finally:
                pkv.fused_attention = False
                stale = [i for i, ly in enumerate(pkv.layers) if ly._new_k is not None]
                for i in stale:
                    pkv.layers[i]._new_k = pkv.layers[i]._new_v = None
            if stale:  # an attention module that bypassed the attention interface: its token was never appended
                raise RuntimeError(f"glb_slab_attention was not reached in layers {stale}: the new token's K / V were not "
                                   "appended - run this model with SlabForward(fused_attention=False)")
            return out.last_hidden_state[:, 0]
        out = self.body(input_ids=ids, position_ids=pos.view(-1, 1).long(), attention_mask=pkv.attention_mask(pos),
                        past_key_values=pkv, use_cache=True)
        return out.last_hidden_state[:, 0]

    @torch.no_grad()
    def __call__(self, ids, pos):
        """ids: int64 [R, 1], pos: int32 [R] (device).  Returns the last hidden states [R, d] (valid until the next call)."""
        self.calls += 1
        if not self.graph_ok or not ids.is_cuda or self.calls <= 2:  # (allocator growth, library set-up: outside a capture)
            return self._run(ids, pos)
        if self._watched:
            ver = self._weights_version()
            if ver != self._watched_version:  # the caller changed a weight in place: captured launches would read stale copies
                self.graphs.clear()
                self._watched_version = ver
        ep = getattr(self.owner, "weights_epoch", 0)
        if ep != self._owner_epoch:  # AsyncAmdLM.refresh_weights(): writes the version counters cannot see (param.data)
            self.graphs.clear()
            self._owner_epoch = ep
        # a graph belongs to the slab tensors it was captured over: every layer's addresses, shape and dtype make the key,
        # and the entry holds the tensors, so the allocator cannot hand their addresses to another slab set meanwhile
        slabs = self.pkv._tensors(self.pkv.layers)
        key = tuple((t.data_ptr(), tuple(t.shape), t.dtype) for t in slabs)
        ent = self.graphs.get(key)
        if ent is None:
            if len(self.graphs) >= 2:  # slab sets keep changing under this forward: not worth capturing
                return self._run(ids, pos)
            s_ids, s_pos = ids.clone(), pos.clone()
            g = torch.cuda.CUDAGraph()
            # No cyclic garbage collection inside the capture: a collection there can destroy a dead object that holds a
            # captured graph or device memory (an earlier population's SlabForward), whose release is not allowed while a
            # stream is being captured and aborts the process.  What is dead already goes first, outside the capture.
            gc.collect()
            gc_was_on = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(g, capture_error_mode="thread_local"):  # (a collective's watchdog thread may be about)
                    hidden = self._run(s_ids, s_pos)
            except RuntimeError as e:
                # a forward that cannot be captured (a host-side decision on device data, a synchronising call): HIP says
                # so in a RuntimeError that names the capture - eager from now on.  Anything else (shapes, memory, an
                # assertion in kv_append) is a real error of the forward and is the caller's to see.
                msg = str(e).lower()
                if not any(w in msg for w in ("captur", "graph", "hipstreamsynchronize", "cudastreamsynchronize",
                                              "operation not permitted")):
                    raise
                self.graph_ok = False
                self.capture_error = e
                torch.cuda.synchronize()
                return self._run(ids, pos)
            finally:
                if gc_was_on:
                    gc.enable()
            ent = self.graphs[key] = (g, s_ids, s_pos, hidden, slabs)
        g, s_ids, s_pos, hidden, _held = ent
        s_ids.copy_(ids)
        s_pos.copy_(pos)
        self.pkv.set_forward_in_place(s_pos)  # (the captured launches read the static buffers)
        g.replay()
        return hidden


class SlabRunner:
    """The KV slabs of one population (`pkv`: a `SharedSlabKV` made by the first encoding that keeps its KV, or the private
    `SlabKV` its owner puts here), the in-place forward over them, and `run`: the forwards of one glb_kv_plan block table.
    R rows of `cap` positions; `in_place`: the fraction of the R rows from which the one-token forward runs on the slab
    where the rows lie (None: never); `graph`: that forward is replayed from a hipGraph (`SlabForward`)."""

    def __init__(self, llm, rows, cap, in_place=0.75, graph=True):
        self.llm, self.R, self.cap, self.in_place, self.graph = llm, int(rows), int(cap), in_place, graph
        self.pkv = None
        self._slab_fwd = None

    def slab_forward(self):
        """The in-place forward over the slabs as they are now: made again when the slabs were replaced, or the body (set_lora
        makes the backend's shadow after a forward was built over the caller's model)."""
        fwd, body = self._slab_fwd, self.llm._body
        if fwd is None or fwd.pkv is not self.pkv or fwd.body is not body:
            fwd = self._slab_fwd = SlabForward(self.pkv, body, graph=self.graph, owner=self.llm)
        return fwd

    @torch.no_grad()
    def _chunk_fused(self):
        """Whether glb_slab_attention_chunk serves a chunk forward over these slabs (SlabForward.fused's conditions)."""
        pkv, cfg, eng = self.pkv, getattr(self.llm._body, "config", None), self.llm.engine
        k0 = pkv.layers[0].keys if pkv.layers and getattr(pkv.layers[0], "is_initialized", False) else None
        return bool(cfg is not None and k0 is not None and k0.is_cuda and hasattr(eng, "slab_attention_chunk")
                    and eng.slab_attention_chunk_supports(k0.dtype, k0.shape[-1])
                    and getattr(cfg, "_attn_implementation", None) == _ATTN_NAME and getattr(cfg, "_glb_engine", None) is eng)

    def _run_chunk(self, plan, lo, hi, t_max, token_at, pad_id):
        """Forward rows lo .. hi - 1 of the plan, fed up to t_max tokens each (right-padded with pad_id) over the slab rows
        where they lie: never part of the one-token forward, never captured.  Returns the hidden states of every row's last
        new token."""
        llm, pkv, dev = self.llm, self.pkv, self.llm.device
        rows = plan["rows_a"][lo:hi].contiguous()
        pos = plan["pos_a"][lo:hi].contiguous()
        nn = plan["n_new_a"][lo:hi].contiguous()
        ctx = plan["ctx_a"][lo:hi].long()
        ar = torch.arange(t_max, device=dev, dtype=torch.int32)
        valid = ar[None, :] < nn[:, None]
        at = torch.where(valid, pos[:, None] + ar[None, :], pos[:, None]).long()  # (padding: a position the row has, its token unused)
        ids = token_at(ctx[:, None].expand(-1, t_max), at).long()
        ids = torch.where(valid, ids, torch.full_like(ids, pad_id))
        fused = self._chunk_fused()
        pkv.set_forward_chunk(rows, pos, nn, fused)
        try:
            if fused:
                pkv.fused_attention = True
                try:  # (no mask: the kernel attends to positions 0 .. pos + t and nothing else)
                    out = llm._body(input_ids=ids, position_ids=at, attention_mask=None, past_key_values=pkv, use_cache=True)
                finally:
                    pkv.fused_attention = False
                    stale = [i for i, ly in enumerate(pkv.layers) if ly._new_k is not None]
                    for i in stale:
                        pkv.layers[i]._new_k = pkv.layers[i]._new_v = None
                if stale:
                    raise RuntimeError(f"glb_slab_attention_chunk was not reached in layers {stale}: the new tokens' K / V "
                                       "were not appended")
            else:
                impl = getattr(getattr(llm._body, "config", None), "_attn_implementation", None)
                add = None if impl in ("sdpa", _ATTN_NAME) else pkv.layers[0].keys.dtype
                out = llm._body(input_ids=ids, position_ids=at, attention_mask=pkv.attention_mask(pos, nn, t_max, add),
                                past_key_values=pkv, use_cache=True)
        finally:
            pkv.n_new = None
        return out.last_hidden_state[torch.arange(hi - lo, device=dev), (nn - 1).long()]

    @torch.no_grad()
    def run(self, plan, counts, token_at, batch, pad_id=0, row_len=None, chunk=(0, 0)):
        """The forwards of the block table `plan` (engine.kv_plan).  counts: (U, nA, nB, n_copied, n_unkept, l_max_b), the
        head words the caller read with its one D2H copy (nothing is read back here).  Rows of kind A - their prefix sits
        in a slab row - are fed ONE token, `token_at(ctx, pos)` (int64 index tensors -> the tokens at position pos of
        contexts ctx), after the copy-on-append copies; rows of kind B are encoded from the ragged `batch` = (tokens,
        starts, lengths), padded with `pad_id`, and their KV kept where the plan names a row.  row_len: int32 [R], what
        every slab row holds according to the caller's table - given, a row outside an in-place forward takes its dummy
        token BEHIND what it holds (a full row has no such place: its length is zeroed, the table forgets it) and a row
        being filled from an encoding at position 0, which the fill overwrites; absent, `pos_of_row` is taken as it is.
        chunk: (rows fed more than one token, the most tokens fed to a row) of a glb_kv_plan_chunk table - the last `chunk[0]`
        of the nA rows; they run after the copies and the one-token forward, gathered (`_run_chunk`).
        Returns (logits [U, V]: A rows, then B rows; tokens fed to the body; whether the A part ran in place)."""
        llm, R, cap = self.llm, self.R, self.cap
        dev = llm.device
        U, nA_all, nB, n_copied, n_unkept, l_max_b = counts
        n_chunk, t_max = chunk
        nA = nA_all - n_chunk  # rows fed one token
        parts, fed, in_place = [], nB * l_max_b, False
        if nA_all and n_copied:
            self.pkv.copy_rows(plan["copy_src"], plan["copy_len"])
        if nA:
            in_place = self.in_place is not None and nA >= self.in_place * R
            if in_place:
                # most rows are live: the forward runs on the slab rows where they lie (rows outside it ride along with a
                # dummy token) instead of gathering the live rows' prefixes into batch order
                ctx_r, pos_d = plan["ctx_of_row"], plan["pos_of_row"]
                at = pos_d
                if row_len is not None:
                    # (a row that is fed a chunk after this forward - ctx -3 - takes its dummy token at its first new position)
                    is_a, idle = ctx_r >= 0, ctx_r == -1
                    row_len.masked_fill_(idle & (row_len >= cap), 0)
                    zero = torch.zeros_like(ctx_r)
                    pos_d = torch.where(is_a | (ctx_r == -3), pos_d, torch.where(idle, row_len.clamp(max=cap - 1), zero))
                    at = torch.where(is_a, pos_d, zero)
                ids = token_at(ctx_r.clamp_min(0).long(), at.long()).view(-1, 1).long()
                hidden = self.slab_forward()(ids, pos_d)
                parts.append(llm._lm_head(hidden.index_select(0, plan["rows_a"][:nA].long())))
                fed += R
            else:
                pos_a = plan["pos_a"][:nA].contiguous()
                ids = token_at(plan["ctx_a"][:nA].long(), pos_a.long()).view(-1, 1).long()
                self.pkv.set_forward(plan["rows_a"][:nA].contiguous(), pos_a)
                out = llm._body(input_ids=ids, position_ids=pos_a.view(-1, 1).long(),
                                attention_mask=self.pkv.attention_mask(pos_a), past_key_values=self.pkv, use_cache=True)
                parts.append(llm._lm_head(out.last_hidden_state[:, 0]))
                fed += nA
        if n_chunk:
            parts.append(llm._lm_head(self._run_chunk(plan, nA, nA_all, t_max, token_at, pad_id)))
            fed += n_chunk * t_max
        if nB:
            sel = plan["ctx_b"][:nB].contiguous()
            stored = nB > n_unkept  # some row keeps the KV of what is encoded here
            enc = encode_ragged(llm, batch, sel, nB, l_max_b, pad_id=pad_id, keep_kv=stored)
            parts.append(llm._lm_head(enc.last_rows()))
            if stored:
                srcs = enc.kv_layers()
                if self.pkv is None:
                    self.pkv = SharedSlabKV(llm.engine, R, cap, len(srcs))
                rows_b = plan["rows_b"][:nB].long()
                slot = torch.where(rows_b >= 0, rows_b, torch.full_like(rows_b, R))  # (rows nobody keeps: a slot past the end)
                src_full = torch.full((R + 1,), -1, dtype=torch.int32, device=dev)
                len_full = torch.zeros(R + 1, dtype=torch.int32, device=dev)
                src_full[slot] = torch.arange(nB, dtype=torch.int32, device=dev)
                len_full[slot] = batch[2][sel.long()]
                src_full[R] = -1
                self.pkv.fill_rows(srcs, src_full[:R].contiguous(), len_full[:R].contiguous())
        return (parts[0] if len(parts) == 1 else torch.cat(parts)), fed, in_place


def ragged(seqs):
    """Host arrays of a ragged batch of token sequences: (tokens int32 [total], starts int64 [n], lengths int32 [n])."""
    n = len(seqs)
    lens = np.fromiter(map(len, seqs), np.int32, n)
    starts = np.zeros(n, np.int64)
    starts[1:] = np.cumsum(lens[:-1])
    return np.fromiter(itertools.chain.from_iterable(seqs), np.int32, int(lens.sum())), starts, lens


class PrefixTable:
    """Device table of cached prompt prefixes (hf.py:155-164), from [(KVPrefix, its token ids)]: `tokens` / `starts` /
    `lengths` for glb_match_prefixes (left out when the ids are None: a batch that names its prefixes itself) and
    per-layer pointer tables for glb_gather_kv_padded.  Holds the prefixes: the pointers stay valid while it lives."""

    def __init__(self, entries, device):
        self.kvs = kvs = [kv for kv, _ in entries]
        p0 = kvs[0]
        for p in kvs[1:]:  # one gather launch per layer serves every prefix: they must come from one model
            if (p.heads, p.head_dim, p.dtype, len(p.layers)) != (p0.heads, p0.head_dim, p0.dtype, len(p0.layers)):
                raise ValueError("cached prefixes of different KV shapes in one batch")
        self.n = len(kvs)
        self.tokens = self.starts = None
        if entries[0][1] is not None:
            flat, starts, lens = ragged([t for _, t in entries])
            self.tokens, self.starts = torch.from_numpy(flat).to(device), torch.from_numpy(starts).to(device)
        else:
            lens = np.array([len(kv) for kv in kvs], np.int32)
        self.lengths, self.p_max = torch.from_numpy(lens).to(device), int(lens.max())
        self.ptrs = [[torch.tensor([kv.layers[l][j].data_ptr() for kv in kvs], dtype=torch.int64, device=device)
                      for j in range(2)] for l in range(len(p0.layers))]

    def cache_for(self, engine, pref_u):
        """The `DynamicCache` of a batch whose row u continues prefix pref_u[u] (int32 device; -1: none): every layer's K
        and V padded to `p_max` positions, one launch each (glb_gather_kv_padded)."""
        p0 = self.kvs[0]
        return DynamicCache(ddp_cache_data=[tuple(engine.gather_kv_padded(self.ptrs[l][j], self.lengths, pref_u, p0.heads,
                                                                           p0.head_dim, self.p_max, p0.dtype)
                                                  for j in range(2)) for l in range(len(p0.layers))])


class RaggedEncoding:
    """What `encode_ragged` ran: the body's output `out`, `hidden` [n_sel, l_max, d] and every row's `last` position."""

    def __init__(self, out, last):
        self.out, self.hidden, self.last = out, out.last_hidden_state, last

    def last_rows(self):
        """[n_sel, d]: the hidden state at every row's last token."""
        return self.hidden[torch.arange(self.last.numel(), device=self.last.device), self.last.long()]

    def kv_layers(self):
        """[(K, V)] per layer, contiguous [n_sel, heads, p_max + l_max, head_dim] (an encoding with `keep_kv`)."""
        return [(ly.keys.contiguous(), ly.values.contiguous()) for ly in self.out.past_key_values.layers]


def encode_ragged(llm, batch, sel, n_sel, l_max, pad_id=0, base=None, prefixes=None, keep_kv=False):
    """Encode contexts `sel` (int32 device, its first n_sel entries) of the ragged `batch` = (tokens, starts, lengths) in one
    forward of `llm._body` (read here: a call may have swapped it): ragged -> padded gather (glb_gather_padded: masks and
    position ids for the whole batch, hf.py:232-246), then the transformer body (PyTorch-ROCm; the only MFMA work on the
    path).  base: int32 [n] device, the leading tokens of every context that are not fed; prefixes = (PrefixTable, int32
    [n_sel] device: the cached prefix of every selected row, -1 none) serves them from the prefixes' KV (hf.py:247-271,
    glb_gather_kv_padded per layer and K / V).  keep_kv: the layers' K / V are wanted.  Nothing is read back here."""
    table, pref = prefixes or (None, None)
    eng = llm.engine
    ids, am, pos, last = eng.gather_padded(*batch, sel, n_sel, base, pad_id, 0 if table is None else table.p_max, l_max)
    cache = None if table is None else table.cache_for(eng, pref)
    return RaggedEncoding(llm._body(input_ids=ids, attention_mask=am, position_ids=pos, past_key_values=cache,
                                    use_cache=keep_kv or cache is not None), last)


# ---- the row-packed encoding: every shared prompt once per forward ----------------------------------------
PACKED_MAX_KEYS = 32  # glb_short_attention_packed: prompt + tail tokens of a context


class PromptGroups:
    """The G prompts a population was built from, as the packed encoding wants them: `lens` (host ints, each >= 1), their
    tokens and positions as the first rows of every packed batch (int64 [sum P_g], made once), the rows' offsets."""

    def __init__(self, prompts, device):
        if not prompts or any(len(p) < 1 for p in prompts):
            raise ValueError("a prompt group needs at least one token")
        self.lens = [len(p) for p in prompts]
        self.n_rows, self.p_max = sum(self.lens), max(self.lens)
        starts = np.concatenate([[0], np.cumsum(self.lens[:-1])]).astype(np.int32)
        lens = np.asarray(self.lens, np.int32)
        self.ids = torch.tensor([t for p in prompts for t in p], dtype=torch.int64, device=device)
        self.pos = torch.tensor([j for p in prompts for j in range(len(p))], dtype=torch.int64, device=device)
        self.starts_d, self.lens_d = torch.from_numpy(starts).to(device), torch.from_numpy(lens).to(device)
        zero = np.zeros_like(lens)
        self.segments = torch.from_numpy(np.stack([zero, zero, starts, lens], 1)).to(device)  # a prompt: no prefix, causal in itself


def packed_plan(group_lens, grp, lens):
    """The packing plan of contexts u = 0 .. U - 1 (group grp[u], lens[u] tokens = its prompt + a tail of t_u >= 1), in NumPy:
    what `encode_packed` computes on the device, restated for tests and for readers.  Rows: the G prompts, then the tails in
    context order.  Returns (segments int32 [G + U, 4]: (pre_start, pre_len, tail_start, tail_len), the prompts' segments
    first; positions int64 [M]; (context, offset) int64 [M] of every row, context -1 - g for prompt g; last int64 [U]: the
    row of every context's last token)."""
    group_lens, grp, lens = np.asarray(group_lens, np.int64), np.asarray(grp, np.int64), np.asarray(lens, np.int64)
    g_start = np.concatenate([[0], np.cumsum(group_lens[:-1])])
    n_pre = int(group_lens.sum())
    tail = lens - group_lens[grp]
    if (tail < 1).any():
        raise ValueError("every context needs a tail of at least one token behind its prompt")
    t_start = n_pre + np.concatenate([[0], np.cumsum(tail[:-1])])
    zero = np.zeros_like(group_lens)
    seg = np.concatenate([np.stack([zero, zero, g_start, group_lens], 1),
                          np.stack([g_start[grp], group_lens[grp], t_start, tail], 1)]).astype(np.int32)
    ctx = np.concatenate([np.repeat(-1 - np.arange(len(group_lens)), group_lens), np.repeat(np.arange(len(lens)), tail)])
    off = np.concatenate([np.arange(p) for p in group_lens] + [group_lens[grp[u]] + np.arange(tail[u]) for u in range(len(lens))])
    return seg, off.astype(np.int64), np.stack([ctx, off], 1).astype(np.int64), (t_start + tail - 1).astype(np.int64)


class _PackedLayer(CacheLayerMixin):
    """Every layer of `PackedKV`: keeps nothing; hands the keys back tagged with the plan (how the attention entry finds it)."""

    is_compileable = False
    is_sliding = False

    def __init__(self, owner):
        super().__init__()
        self.owner = owner

    def lazy_initialization(self, key_states, value_states):
        self.is_initialized = True

    def update(self, key_states, value_states, *args, **kwargs):
        key_states._glb_packed = self.owner
        return key_states, value_states

    def get_mask_sizes(self, query_length):
        return query_length, 0

    def get_seq_length(self):
        return 0

    def get_max_length(self):
        return -1


class PackedKV(Cache):
    """The side channel of one row-packed forward: a `Cache` that stores nothing (so transformers builds no mask and looks
    for no packed sequences in the position ids) and carries the plan to the "glb" attention entry on the key tensor.
    `segments`: int32 [G + U, 4] device, `n_rows` = M, `max_keys` <= 32; `served` counts the layers that reached the kernel."""

    def __init__(self, engine, segments, n_rows, max_keys, n_layers):
        self.engine, self.segments, self.n_rows, self.max_keys = engine, segments, int(n_rows), int(max_keys)
        self.served = 0
        layer = _PackedLayer(self)
        super().__init__(layers=[layer] * n_layers)


class PackedEncoding:
    """What `encode_packed` ran: `hidden` [M, d] and the row `last` [n_sel] of every context's last token."""

    def __init__(self, out, last, n_rows):
        self.out, self.hidden, self.last, self.n_rows = out, out.last_hidden_state[0], last, n_rows

    def last_rows(self):
        """[n_sel, d]: the hidden state at every context's last token."""
        return self.hidden[self.last]


def packed_supported(llm):
    """Whether `llm._body`'s attention is served by this library's short-context kernels (the shadow points at the "glb"
    entry with the backend's engine, a head width the kernels are built for)."""
    body, eng = llm._body, llm.engine
    cfg = getattr(body, "config", None)
    if cfg is None or getattr(cfg, "_attn_implementation", None) != _ATTN_NAME or getattr(cfg, "_glb_engine", None) is not eng:
        return False
    heads = getattr(cfg, "num_attention_heads", None)
    head_dim = getattr(cfg, "head_dim", None) or (cfg.hidden_size // heads if heads else None)
    return bool(head_dim in (16, 32, 64, 128) and getattr(cfg, "num_hidden_layers", 0) > 0)


def _packed_plan_arrays(llm, batch, sel, n_sel, grp, groups, n_tail_rows, native_plan=True):
    """The plan of `encode_packed` on the device: (segments int32 [G + U, 4], ids int64 [M], pos int64 [M], last int64 [U], M).
    native_plan: glb_packed_plan, two launches; False, or an engine without `packed_plan`: the torch ops below, the
    restatement the kernel is tested against (tests/test_packed_plan_native_gpu.py) - the same arrays for every input."""
    eng, dev = llm.engine, llm.device
    tokens, starts, lengths = batch
    G, n_pre = len(groups.lens), groups.n_rows
    M = n_pre + int(n_tail_rows)
    max_pos = getattr(llm._body.config, "max_position_embeddings", None) or (1 << 30)
    pos_cap = min(PACKED_MAX_KEYS, max_pos)
    native = getattr(eng, "packed_plan", None) if native_plan else None  # (None: an engine without the kernel)
    if native is not None:
        return native(batch, sel, n_sel, grp, groups, n_tail_rows, pos_cap) + (M,)
    sel_l, grp_l = sel[:n_sel].long(), grp[:n_sel].long().clamp(0, G - 1)
    pre_len, pre_start = groups.lens_d[grp_l], groups.starts_d[grp_l]
    tail = lengths[sel_l] - pre_len  # int32 [U]
    ends = torch.cumsum(tail, 0, dtype=torch.int32)
    tail_start = n_pre + ends - tail
    segments = torch.cat([groups.segments, torch.stack([pre_start, pre_len, tail_start, tail], 1)]).contiguous()
    # row -> (context, offset in its tail): the context whose [tail_start, tail_start + t) holds the row
    r = torch.arange(int(n_tail_rows), dtype=torch.int32, device=dev)
    u = torch.searchsorted(ends, r, right=True).clamp_(max=n_sel - 1)
    pos_t = (pre_len[u] + (r - (ends - tail)[u])).long()
    at = (starts[sel_l[u]] + pos_t).clamp_(0, tokens.numel() - 1)
    ids = torch.cat([groups.ids, tokens[at].long()])
    pos = torch.cat([groups.pos, pos_t.clamp_(0, pos_cap - 1)])
    return segments, ids, pos, (tail_start + tail - 1).long().clamp_(0, M - 1), M


def encode_packed(llm, batch, sel, n_sel, grp, groups, n_tail_rows, max_keys=PACKED_MAX_KEYS, native_plan=True):
    """Encode contexts `sel` (int32 device, its first n_sel entries) of the ragged `batch` = (tokens, starts, lengths) in one
    ROW-PACKED forward of `llm._body`: context u is prompt `grp[u]` (int32 [n_sel] device) of `groups` (PromptGroups) plus a
    tail of t_u >= 1 tokens, and the batch is [1, M]: the G prompts once, then the tails in context order - M = sum P_g +
    n_tail_rows, where n_tail_rows = sum t_u is the CALLER's (host) number: nothing is read back here.  The prompts' hidden
    states, K and V are the same for every context behind them (same tokens, same positions, causal), so computing them once
    changes no result; attention is glb_short_attention_packed through `PackedKV`.  max_keys: the most P + t of a context
    (<= 32).  Lengths that do not match n_tail_rows, a tail < 1 or a context longer than max_keys are refused row by row in
    the kernel (engine.error_word / raise_if_failed); every index used here is clamped into range first.  native_plan: the
    plan's four arrays come from glb_packed_plan (`_packed_plan_arrays`); False keeps the torch ops."""
    eng = llm.engine
    if not 1 <= max_keys <= PACKED_MAX_KEYS:
        raise ValueError(f"encode_packed serves contexts of up to {PACKED_MAX_KEYS} tokens")
    if n_sel < 1 or n_tail_rows < n_sel:
        raise ValueError("encode_packed: every context feeds at least one tail row")
    if not packed_supported(llm):
        raise RuntimeError("encode_packed: this model's attention is not served by glb_short_attention")
    segments, ids, pos, last, M = _packed_plan_arrays(llm, batch, sel, n_sel, grp, groups, n_tail_rows, native_plan)
    ids, pos = ids.view(1, M), pos.view(1, M)
    pkv = PackedKV(eng, segments, M, max_keys, llm._body.config.num_hidden_layers)
    out = llm._body(input_ids=ids, position_ids=pos, attention_mask=None, past_key_values=pkv, use_cache=True)
    if pkv.served != len(pkv.layers):
        raise RuntimeError(f"glb_short_attention_packed served {pkv.served} of {len(pkv.layers)} layers: an attention module "
                           "bypassed the attention interface and attended across the packed contexts")
    return PackedEncoding(out, last, M)


class PrefixLRU:
    """Least-recently-used store of cached prompt prefixes under a byte budget.  Keys are trie nodes; evicting an entry
    drops the node's `past_key_values` (the log-prob rows stay), so later queries fall back to re-encoding."""

    def __init__(self, budget_bytes, on_remove=None):
        self.budget = int(budget_bytes)
        self.used = 0
        self._od = OrderedDict()
        self.evictions = 0
        self.on_remove = on_remove  # called with the node whenever an entry leaves the store (evicted or dropped)

    def put(self, node, kv):
        self.drop(node)
        size = kv.nbytes()
        node.past_key_values = kv
        self._od[id(node)] = (node, size)
        self.used += size
        while self.used > self.budget and len(self._od) > 1:
            _, (old, sz) = self._od.popitem(last=False)
            old.past_key_values = None
            self.used -= sz
            self.evictions += 1
            if self.on_remove is not None:
                self.on_remove(old)

    def touch(self, node):
        key = id(node)
        if key in self._od:
            self._od.move_to_end(key)

    def drop(self, node):
        ent = self._od.pop(id(node), None)
        if ent is not None:
            self.used -= ent[1]
            ent[0].past_key_values = None
            if self.on_remove is not None:
                self.on_remove(ent[0])

    def clear(self):
        nodes = [node for node, _ in self._od.values()]
        for node in nodes:
            node.past_key_values = None
        self._od.clear()
        self.used = 0
        if self.on_remove is not None:
            for node in nodes:
                self.on_remove(node)

    def nodes(self):
        return [node for node, _ in self._od.values()]

    def __len__(self):
        return len(self._od)
