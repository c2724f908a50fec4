"""A private view of the caller's HuggingFace model for this backend's forwards.

The reference leaves the model it is handed alone (hf.py:114-140).  Earlier rounds rewrote activation modules of
`hf_model` and re-pointed `hf_model.config._attn_implementation` in place; now `AsyncAmdLM` runs its forwards on a
**shadow** of the module tree: every module is a shallow copy (`copy.copy`) that SHARES its `_parameters` / `_buffers`
dictionaries with the original - the same weights, also after the caller replaces them (`model.to(...)`,
`load_state_dict`) - but has its own `_modules` table and its own copy of the configuration.  Whatever is swapped below
happens in the shadow only; the caller's model, its configuration and its forward are never touched, so two backends over
one model, or a foreign thread running `hf_model(...)`, see exactly the model they built.

What the shadow swaps (PyTorch ops only - no kernels of this library inside the transformer body except attention):
  * GPT-2's `gelu_new` spelled as eight elementwise ops      -> `torch.nn.GELU(approximate="tanh")`     (one kernel)
  * Llama-family RMSNorm spelled as pow / mean / add / rsqrt / mul / two casts / mul (hf modeling_llama.py:52-67)
                                                             -> `torch.nn.functional.rms_norm`          (one kernel)
  * Llama-family rotary embedding spelled as slice / neg / cat / mul / mul / add per tensor (modeling_llama.py:130-160)
                                                             -> roll + mul + addcmul, queries and keys in one pass
  * the q / k / v projections (three GEMMs)                  -> one GEMM on a derived [q; k; v] weight (a copy of those
                                                                rows, rebuilt when the caller's weights change)
  * Llama's gate_proj + up_proj, for few-token forwards       -> one GEMM on a derived [gate; up] weight (a second copy of
                                                                those two matrices: `merge_mlp=False` keeps the memory)
  * GPT-2's Conv1D projections (float32)                     -> `SplitConv1D`: this library's split-bf16 MFMA GEMM
                                                                (glb_gemm_f32_split, on a derived bf16 image of the weight)
                                                                for the batches where it was measured faster; the MLP's
                                                                tanh GELU then runs in that GEMM's epilogue, and a block's
                                                                two residual adds in the epilogues of its `c_proj`s
  * the attention interface                                  -> kv.py's "glb" entry (glb_short_attention /
                                                                glb_slab_attention where they apply, SDPA otherwise)
Same functions, different rounding (float32 inside the fused ops, one rounding at the end; the split GEMM is fp32-accurate
but sums in another order than the library's): the reference's goldens hold
within 1e-4 with identical tokens (tests/test_host_cpu.py, tests/test_host_gpu.py).
"""
import copy
import types

import torch

RMSNORM_CLASSES = ("LlamaRMSNorm", "MistralRMSNorm", "Qwen2RMSNorm", "Qwen3RMSNorm")  # x * rsqrt(mean(x^2) + eps) * weight
ROPE_ATTENTION_CLASSES = ("LlamaAttention",)


def shadow_model(model):
    """Shallow structural copy of a module tree: new module objects and `_modules` tables, shared parameter / buffer
    tables, one private copy of the configuration (modules that referenced the original configuration reference the copy)."""
    cfg = getattr(model, "config", None)
    new_cfg = copy.copy(cfg) if cfg is not None else None
    memo = {}

    def walk(mod):
        got = memo.get(id(mod))
        if got is not None:
            return got
        new = copy.copy(mod)
        memo[id(mod)] = new
        new._modules = {name: (walk(child) if child is not None else None) for name, child in mod._modules.items()}
        if cfg is not None and new.__dict__.get("config") is cfg:
            new.__dict__["config"] = new_cfg
        return new

    return walk(model)


class FusedRMSNorm(torch.nn.Module):
    """`weight * (x * rsqrt(mean(x^2) + eps))` as one `rms_norm` call; shares the original module's parameter table."""

    def __init__(self, src):
        super().__init__()
        self._parameters = src._parameters
        self.eps = float(src.variance_epsilon)

    def forward(self, hidden_states):
        return torch.nn.functional.rms_norm(hidden_states, (hidden_states.shape[-1],), self.weight, self.eps)

    def extra_repr(self):
        return f"{tuple(self.weight.shape)}, eps={self.eps} (fused)"


def _rope(x, rolled, cos, sin_signed):
    """x, rolled [B, T, H, D] (the projection's own layout; rolled = x with the halves of D swapped), cos / sin_signed
    [B, T, 1, D].  x * cos + rotate_half(x) * sin with rotate_half(x) * sin = roll(x, D/2) * (sin with its first half
    negated): three kernels (roll, mul, addcmul) instead of six (slice, neg, cat, mul, mul, add)."""
    return torch.addcmul(x * cos, rolled, sin_signed)


def _merged_qkv(attn):
    """One weight [q; k; v] for the three projections (one GEMM instead of three, two of them a quarter as wide, and the
    rotary embedding applied to queries and keys in ONE pass over the joint output).  A derived copy of the caller's
    weights (q + k + v rows: 12.6 MB a layer at Llama-3.2-1B's shape), rebuilt whenever one of them is replaced or changed
    in place (`Tensor._version`)."""
    ws = (attn.q_proj.weight, attn.k_proj.weight, attn.v_proj.weight)
    bs = (attn.q_proj.bias, attn.k_proj.bias, attn.v_proj.bias)
    key = tuple((id(t), t._version, t.data_ptr()) for t in ws + bs if t is not None)
    ent = attn.__dict__.get("_glb_qkv")
    if ent is None or ent[0] != key:
        with torch.no_grad():
            w = torch.cat(ws, 0)
            b = torch.cat(bs, 0) if bs[0] is not None else None
        # (the entry holds the source tensors: their ids cannot be handed to other tensors while it lives)
        ent = attn.__dict__["_glb_qkv"] = (key, w, b, ws + bs)
    return ent[1], ent[2]


def _row_deltas(x, joint, parts):
    """A call that names adapters per context (lora.RowLora) wraps its targeted projections: the output of a joint GEMM gets
    each wrapped projection's per-row delta on that projection's column slice (module, first column, columns), in place."""
    for mod, first, cols in parts:
        add = getattr(mod, "add_delta", None)
        if add is not None:
            add(x, joint[..., first:first + cols])


MERGE_MLP_MAX_TOKENS = 2048  # up to here one GEMM for gate + up wins (tools/dbg/gemm_merge_probe.py); beyond, two do


def _merged_gate_up(mlp):
    """One weight [gate; up] for a SwiGLU MLP's two input projections, as `_merged_qkv`: a derived copy (at Llama-3.2-1B's
    shape 67 MB a layer), rebuilt when the caller's weights change."""
    ws = (mlp.gate_proj.weight, mlp.up_proj.weight)
    bs = (mlp.gate_proj.bias, mlp.up_proj.bias)
    key = tuple((id(t), t._version, t.data_ptr()) for t in ws + bs if t is not None)
    ent = mlp.__dict__.get("_glb_gate_up")
    if ent is None or ent[0] != key:
        with torch.no_grad():
            w = torch.cat(ws, 0)
            b = torch.cat(bs, 0) if bs[0] is not None else None
        ent = mlp.__dict__["_glb_gate_up"] = (key, w, b, ws + bs)
    return ent[1], ent[2]


def _llama_mlp_forward(self, x):
    """modeling_llama.py:174-176.  For the few-token forwards of the path (one token per KV row: M = 512 to 1024) gate_proj and
    up_proj are ONE GEMM on a derived [gate; up] weight - at M = 512 two GEMMs of N = 8192 leave three quarters of the chip's
    CUs without a tile (65.6 -> 48.3 us a layer at Llama-3.2-1B's shape, 135 -> 114 at Llama-3-8B's); the big re-encoding
    batches keep two GEMMs (the strided halves cost the elementwise ops more than the GEMM gains there)."""
    if (hasattr(self.gate_proj, "weight") and x.shape[:-1].numel() <= MERGE_MLP_MAX_TOKENS  # (no .weight: quant.W4Linear)
            and not (torch.is_grad_enabled() and (x.requires_grad or self.gate_proj.weight.requires_grad))):
        w, b = _merged_gate_up(self)
        n = self.gate_proj.weight.shape[0]
        h = torch.nn.functional.linear(x, w, b)
        _row_deltas(x, h, ((self.gate_proj, 0, n), (self.up_proj, n, h.shape[-1] - n)))  # (before the activation)
        return self.down_proj(self.act_fn(h[..., :n]) * h[..., n:])
    return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))


# The split GEMM's dispatch rule: the fewest rows (tokens of a forward) at which it runs, per (N, K) of a Conv1D, from the
# A/B of profiles/r07/split_gemm_ab.txt (tools/split_gemm_ab.py: native kernel vs torch.addmm in one process, alternating):
# the first measured row count from which the kernel wins at every larger one.  Shapes not listed, and smaller batches -
# the one-token KV forwards (M ~ 1024) among them - keep the library GEMM.
SPLIT_GEMM_MIN_ROWS = {
    (2304, 768): 1536,  # attn.c_attn: 0.73x the library's time at 1536 rows, 0.62-0.89x above
    (768, 768): 6144,  # attn.c_proj: 1.08x at 4096, 0.61-0.82x from 6144
    (3072, 768): 1536,  # mlp.c_fc (with its GELU): 0.85x at 1536, 0.65-0.90x above
    (768, 3072): 8192,  # mlp.c_proj: 1.03x at 6144 (245 us), 0.74x at 9216 (249 us: the kernel's time is flat between the
                        # two, the library's rises with M), 0.68-0.90x above
}


class split_gemm_all_rows:
    """For the duration of one forward, every `SplitConv1D` over `engine` runs the split kernel whatever its row count (the
    table above is not touched).  The row-packed encoding (kv.encode_packed) feeds a fraction of the padded batch's rows; the
    kernel's bits of a row do not depend on the batch around it, the library GEMM's may: with this, a row
    has the bits it has in the padded batch that ran the kernel.  Nests; not for use from two threads over one engine."""

    def __init__(self, engine):
        self.engine = engine

    def __enter__(self):
        self.was = getattr(self.engine, "_split_all_rows", False)
        self.engine._split_all_rows = True
        return self

    def __exit__(self, *exc):
        self.engine._split_all_rows = self.was
        return False


def _is_tanh_gelu(act):
    return isinstance(act, torch.nn.GELU) and act.approximate == "tanh"


class SplitConv1D(torch.nn.Module):
    """GPT-2's Conv1D (`addmm(bias, x, weight)`, weight [K, N]) sharing the original module's parameter table.  A float32
    forward on the engine's device without autograd, of at least `min_rows` rows, runs glb_gemm_f32_split on a derived
    image of the weight (hi / mid / lo bf16 planes, 6 bytes per element, rebuilt when the weight is replaced or changed in
    place: `Tensor._version`, identity, address); everything else - other dtypes, fewer rows, autograd, a bias that is not
    contiguous float32 - runs `torch.addmm` exactly as Conv1D does.  `act`: an activation applied to the result - the tanh
    GELU goes into the GEMM's epilogue.

    On the kernel's path the result is Conv1D's to float32 accuracy for finite operands below 0x1.ffp127 (3.3961775e38), not
    beyond: a NaN, an infinity or a finite value at or above that threshold (+-FLT_MAX included) in x makes its whole output
    row non-finite, in the weight its whole output column, where Conv1D gives +-inf or a finite number; the other rows and
    columns are unaffected (include/glb.h, glb_gemm_f32_split)."""

    def __init__(self, src, engine, min_rows):
        super().__init__()
        self._parameters = src._parameters
        self.nf, self.nx = src.nf, src.nx
        self.min_rows = min_rows
        self.fused_residuals = 0  # calls whose epilogue added a block's residual
        self.__dict__["_glb_engine"] = engine  # (not a submodule)

    def _split(self):
        w = self.weight
        key = (id(w), w._version, w.data_ptr())
        ent = self.__dict__.get("_glb_split")
        if ent is None or ent[0] != key:
            with torch.no_grad():
                img = self._glb_engine.gemm_split_weights(w)
            # (the entry holds the weight: its id cannot be handed to another tensor while it lives)
            ent = self.__dict__["_glb_split"] = (key, img, w)
        return ent[1]

    def _native(self, x):
        w = self.weight
        return (x.dtype == torch.float32 and w.dtype == torch.float32 and x.is_cuda and x.device == w.device
                and x.device == self._glb_engine.device
                and (x.shape[:-1].numel() >= self.min_rows or getattr(self._glb_engine, "_split_all_rows", False))
                and not (torch.is_grad_enabled() and (x.requires_grad or w.requires_grad
                                                      or (self.bias is not None and self.bias.requires_grad))))

    def offer_residual(self, residual):
        """A GPT-2 block hands its residual over for the ONE call that follows (`_gpt2_block_forward`): if that call runs the
        kernel, the add happens in its epilogue.  `residual_taken` tells the block afterwards, and clears the offer."""
        self.__dict__["_glb_residual"] = residual

    def residual_taken(self):
        self.__dict__.pop("_glb_residual", None)  # (an offer no call consumed)
        return self.__dict__.pop("_glb_residual_taken", False)

    def forward(self, x, act=None):
        residual = self.__dict__.pop("_glb_residual", None)
        if self._native(x):
            img = self._split()
            if img is not None:
                gelu = _is_tanh_gelu(act)
                if (residual is not None and act is None and residual.dtype == torch.float32 and residual.device == x.device
                        and residual.shape == x.shape[:-1] + (self.nf,) and residual.is_contiguous()
                        and not (torch.is_grad_enabled() and residual.requires_grad)):
                    y = self._glb_engine.gemm_split(x, img, self.nf, self.bias, residual=residual)
                    if y is not None:
                        self.__dict__["_glb_residual_taken"] = True
                        self.fused_residuals += 1
                        return y
                y = self._glb_engine.gemm_split(x, img, self.nf, self.bias, gelu=gelu)
                if y is not None:
                    return y if gelu or act is None else act(y)
        size_out = x.size()[:-1] + (self.nf,)
        y = torch.addmm(self.bias, x.view(-1, x.size(-1)), self.weight).view(size_out)
        return y if act is None else act(y)

    def extra_repr(self):
        return f"nf={self.nf}, nx={self.nx}, split-bf16 GEMM from {self.min_rows} rows"


def _gpt2_mlp_forward(self, hidden_states):
    """modeling_gpt2.py GPT2MLP.forward with the activation handed to c_fc (SplitConv1D: the tanh GELU in its epilogue)."""
    h = self.c_fc(hidden_states, act=self.act)
    return self.dropout(self.c_proj(h))


RESIDUAL_EPILOGUE = True  # False: every block runs its own adds (the A/B switch of tests/test_packed_fused_forward_gpu.py)


def _gpt2_block_forward(self, hidden_states, past_key_values=None, attention_mask=None, encoder_hidden_states=None,
                        encoder_attention_mask=None, use_cache=False, **kwargs):
    """modeling_gpt2.py GPT2Block.forward with each residual offered to the `c_proj` that precedes its add: a SplitConv1D
    about to run the kernel adds it in the epilogue (the bits of `attn_output + residual` and of `residual +
    feed_forward_hidden_states`: fp32 addition commutes), and the block skips its own add.  Offered only while the dropout
    behind that `c_proj` is the identity (not training); a projection that runs its library GEMM, is wrapped (per-row LoRA)
    or is no SplitConv1D leaves the add to the block, as does a block with cross-attention (the module's own code)."""
    if encoder_hidden_states is not None or not RESIDUAL_EPILOGUE:
        return type(self).forward(self, hidden_states, past_key_values=past_key_values, attention_mask=attention_mask,
                                  encoder_hidden_states=encoder_hidden_states, encoder_attention_mask=encoder_attention_mask,
                                  use_cache=use_cache, **kwargs)
    residual = hidden_states
    proj = self.attn._modules.get("c_proj")
    offered = isinstance(proj, SplitConv1D) and not self.attn.training
    if offered:
        proj.offer_residual(residual)
    try:
        attn_output, _ = self.attn(self.ln_1(hidden_states), past_key_values=past_key_values, attention_mask=attention_mask,
                                   use_cache=use_cache, **kwargs)
    finally:
        taken = offered and proj.residual_taken()
    hidden_states = attn_output if taken else attn_output + residual
    residual = hidden_states
    proj = self.mlp._modules.get("c_proj")
    offered = isinstance(proj, SplitConv1D) and not self.mlp.training
    if offered:
        proj.offer_residual(residual)
    try:
        feed_forward_hidden_states = self.mlp(self.ln_2(hidden_states))
    finally:
        taken = offered and proj.residual_taken()
    return feed_forward_hidden_states if taken else residual + feed_forward_hidden_states


def weights_version(net):
    """A number that changes when a weight the shadow keeps a derived copy of changes (SlabForward drops its hipGraphs then:
    a captured launch would keep reading the stale copy)."""
    v = 0
    for mod in net.modules():
        ent = mod.__dict__.get("_glb_qkv")
        if ent is not None and hasattr(mod.q_proj, "weight"):
            for t in (mod.q_proj.weight, mod.k_proj.weight, mod.v_proj.weight):
                v += t._version + (id(t) & 0xFFFF)
        if mod.__dict__.get("_glb_split") is not None:
            t = mod.weight
            v += t._version + (id(t) & 0xFFFF)
    return v


def _llama_attention_forward(self, hidden_states, position_embeddings=None, attention_mask=None, past_key_values=None,
                             **kwargs):
    """modeling_llama.py:243-281 with q / k / v from one GEMM and the rotary embedding applied to queries and keys together,
    before the head transpose (see `_rope`).  A forward that may be differentiated runs the module's own code."""
    from transformers.modeling_utils import ALL_ATTENTION_FUNCTIONS
    from transformers.models.llama.modeling_llama import eager_attention_forward

    w4 = not hasattr(self.q_proj, "weight")  # quant.W4Linear: 4-bit images, nothing to concatenate or differentiate
    if torch.is_grad_enabled() and (hidden_states.requires_grad or (not w4 and self.q_proj.weight.requires_grad)):
        return type(self).forward(self, hidden_states, position_embeddings=position_embeddings, attention_mask=attention_mask,
                                  past_key_values=past_key_values, **kwargs)
    input_shape = hidden_states.shape[:-1]
    D = self.head_dim
    if w4:  # three projections, one joint tensor: the rotary pass below stays the fused one
        qkv = torch.cat((self.q_proj(hidden_states), self.k_proj(hidden_states), self.v_proj(hidden_states)), -1)
        qkv = qkv.view(*input_shape, -1, D)
        n_kv = self.k_proj.out_features // D
    else:
        w, b = _merged_qkv(self)
        qkv = torch.nn.functional.linear(hidden_states, w, b)
        nq, nk = self.q_proj.weight.shape[0], self.k_proj.weight.shape[0]
        _row_deltas(hidden_states, qkv, ((self.q_proj, 0, nq), (self.k_proj, nq, nk),
                                         (self.v_proj, nq + nk, qkv.shape[-1] - nq - nk)))  # (before the rotary pass)
        qkv = qkv.view(*input_shape, -1, D)  # [B, T, Hq + 2 Hkv, D]
        n_kv = nk // D
    n_q = qkv.shape[-2] - 2 * n_kv
    cos, sin = position_embeddings
    ss = getattr(sin, "_glb_signed", None)
    half = D // 2
    if ss is None:
        ss = torch.cat((-sin[..., :half], sin[..., half:]), dim=-1)
    rolled = torch.roll(qkv, half, -1)  # (the whole joint tensor: a roll of a strided slice would copy it first)
    qk = _rope(qkv[..., :n_q + n_kv, :], rolled[..., :n_q + n_kv, :], cos.unsqueeze(2), ss.unsqueeze(2))
    q = qk[..., :n_q, :].transpose(1, 2)
    k = qk[..., n_q:, :].transpose(1, 2)
    v = qkv[..., n_q + n_kv:, :].transpose(1, 2)
    if past_key_values is not None:
        k, v = past_key_values.update(k, v, self.layer_idx)
    attention_interface = ALL_ATTENTION_FUNCTIONS.get_interface(self.config._attn_implementation, eager_attention_forward)
    attn_output, attn_weights = attention_interface(self, q, k, v, attention_mask,
                                                    dropout=0.0 if not self.training else self.attention_dropout,
                                                    scaling=self.scaling, **kwargs)
    attn_output = attn_output.reshape(*input_shape, -1).contiguous()
    return self.o_proj(attn_output), attn_weights


def _rotary_forward_signed(self, x, position_ids):
    """The rotary module's own forward, its sine tagged with the half-negated copy `_rope` multiplies the rolled tensor
    by (made once per forward instead of once per layer)."""
    cos, sin = type(self).forward(self, x, position_ids)
    half = sin.shape[-1] // 2
    sin._glb_signed = torch.cat((-sin[..., :half], sin[..., half:]), dim=-1)
    return cos, sin


def fuse_shadow(shadow, activations=True, merge_mlp=True, split_engine=None):
    """Swap the decomposed activations / norms / rotary embedding of a SHADOW tree (never call this on a caller's model).
    split_engine: a HipEngine - GPT-2's float32 Conv1D projections of the shapes in SPLIT_GEMM_MIN_ROWS become
    SplitConv1D (None: not swapped).  Returns the names of what was swapped."""
    done = []
    if split_engine is not None:
        done += _split_conv1d(shadow, split_engine)
    if not activations:
        return done
    for mod in list(shadow.modules()):
        for name, child in list(mod._modules.items()):
            kind = type(child).__name__
            if kind == "NewGELUActivation":
                mod._modules[name] = torch.nn.GELU(approximate="tanh")
                done.append("gelu_new")
            elif kind in RMSNORM_CLASSES and hasattr(child, "variance_epsilon") and "weight" in child._parameters:
                mod._modules[name] = FusedRMSNorm(child)
                done.append("rms_norm")
            elif kind in ROPE_ATTENTION_CLASSES:
                child.forward = types.MethodType(_llama_attention_forward, child)
                done.append("rope")
            elif kind == "LlamaRotaryEmbedding":
                child.forward = types.MethodType(_rotary_forward_signed, child)
            elif kind == "LlamaMLP" and merge_mlp:
                child.forward = types.MethodType(_llama_mlp_forward, child)
                done.append("gate_up")
    return done


def _split_conv1d(shadow, engine):
    done = []
    for mod in list(shadow.modules()):
        for name, child in list(mod._modules.items()):
            if type(child).__name__ != "Conv1D" or child.weight.dtype != torch.float32:
                continue
            min_rows = SPLIT_GEMM_MIN_ROWS.get((child.nf, child.nx))
            if min_rows is None or not engine.gemm_split_supports(child.nx, child.nf):
                continue
            mod._modules[name] = SplitConv1D(child, engine, min_rows)
            done.append("split_gemm")
        if type(mod).__name__ == "GPT2MLP" and isinstance(mod._modules.get("c_fc"), SplitConv1D):
            mod.forward = types.MethodType(_gpt2_mlp_forward, mod)
    for mod in shadow.modules():  # (after the swaps: a block is listed before its children)
        if type(mod).__name__ == "GPT2Block" and any(
                isinstance(getattr(mod, part)._modules.get("c_proj"), SplitConv1D) for part in ("attn", "mlp") if hasattr(mod, part)):
            mod.forward = types.MethodType(_gpt2_block_forward, mod)
    return done
