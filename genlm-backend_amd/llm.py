"""AsyncLM interface and the MI355X backend behind it.

Mirrors, name for name, the surface of the reference that the hot path exposes:
  * `AsyncLM`                       genlm/backend/llm/base.py:9-179
  * `AsyncAmdLM` (= AsyncTransformer of genlm/backend/llm/hf.py:73-422 with the per-step work moved
    to the HIP library): `from_name`, `next_token_logprobs[_sync|_uncached]`,
    `batch_next_token_logprobs[_sync]`, `sample`, `batch_sample`, `cache_kv`, `clear_cache`,
    `clear_kv_cache`, `reset_async_queries`, `walk_cache`, `add_query`, `batch_evaluate_queries`,
    attributes `model tokenizer device cache queries batch_size timeout timer byte_vocab str_vocab`
  * `load_model_by_name`            genlm/backend/llm/__init__.py:10-43 (extra backend value "amd")
plus one addition the reference leaves to user code (README.md:82-91): `next_token_step`, the fused
log-softmax + mask + logsumexp + categorical draw, autobatched through the same queue.

All device arithmetic after the transformer's final hidden state goes through `HipEngine`
(C ABI, include/glb.h).  There is no CPU fallback: without the built library and a HIP device the
constructor raises.
"""
import asyncio
from abc import ABC, abstractmethod

import numpy as np
import torch

from .cache import KVPrefix, RowLRU, TokenTrie
from .kv import PrefixLRU, PrefixTable, encode_ragged, ragged
from .masks import MASK_BITS, MASK_F32, MASK_NONE, RegisteredMasks  # noqa: F401 (the kinds stay importable from here)
from .tokenization import decode_vocab

RNG_NONE, RNG_PHILOX, RNG_NOISE = 0, 1, 2


class AsyncLM(ABC):
    """base.py:9-179."""

    def __init__(self, tokenizer):
        self.tokenizer = tokenizer
        self.byte_vocab, self.str_vocab = decode_vocab(self.tokenizer)

    @abstractmethod
    async def next_token_logprobs(self, token_ids):
        pass

    @abstractmethod
    def next_token_logprobs_sync(self, token_ids):
        pass

    async def batch_next_token_logprobs(self, token_ids_list):
        """base.py:47-60"""
        logprobs = await asyncio.gather(*[self.next_token_logprobs(t) for t in token_ids_list])
        return torch.stack(logprobs)

    def batch_next_token_logprobs_sync(self, token_ids_list):
        """base.py:62-73"""
        return torch.stack([self.next_token_logprobs_sync(t) for t in token_ids_list])

    def add_new_lora(self, lora_path, lora_name):
        raise NotImplementedError("add_new_lora must be implemented by subclasses")

    def set_lora(self, lora_path, lora_name):
        raise NotImplementedError("set_lora must be implemented by subclasses")

    def clear_lora(self):
        raise NotImplementedError("clear_lora must be implemented by subclasses")

    def clear_cache(self):
        pass

    def _draw(self, logprobs, temperature, generator_state):
        """One categorical draw from softmax(logprobs / temperature); subclasses override."""
        probs = torch.softmax(logprobs / temperature, dim=-1)
        return torch.multinomial(probs.cpu(), num_samples=1, generator=generator_state).item()

    def _make_generator(self, seed):
        if seed is None:
            return None
        g = torch.Generator()
        g.manual_seed(seed)
        return g

    async def sample(self, prompt_token_ids, max_tokens, eos_token_ids, temperature=1.0, seed=None):
        """base.py:110-146"""
        gen = self._make_generator(seed)
        generated = []
        for _ in range(max_tokens):
            logprobs = await self.next_token_logprobs(prompt_token_ids + generated)
            tok = self._draw(logprobs, temperature, gen)
            if tok in eos_token_ids:
                break
            generated.append(tok)
        return generated

    async def batch_sample(self, prompt_token_ids_list, max_tokens, eos_token_ids, temperature=1.0, seed=None):
        """base.py:148-179 (every sequence gets its own generator seeded with `seed`)"""
        return await asyncio.gather(*[
            self.sample(prompt_token_ids=p, max_tokens=max_tokens, eos_token_ids=eos_token_ids,
                        temperature=temperature, seed=seed)
            for p in prompt_token_ids_list
        ])


class Query:
    """A pending request (hf.py:14-70).  Padding, masks and position ids are no longer built per query in
    Python: the gather kernel produces them for the whole batch (glb_gather_padded)."""

    __slots__ = ("prompt", "future", "past", "past_len", "first_new", "kind", "mask_id")

    def __init__(self, prompt, future, past=None, first_new=0, kind="logprobs", mask_id=0):
        self.prompt = prompt
        self.future = future
        self.past = past
        self.past_len = len(past) if past is not None else 0
        self.first_new = first_new  # first prompt position whose next-token row the caller needs
        self.kind = kind            # "logprobs" | "step"
        self.mask_id = mask_id


class _Slot:
    """Stand-in for a query's future on the synchronous paths.  reraise: an exception handed over is raised where it is
    set instead of being kept in `exc`."""

    __slots__ = ("value", "exc", "reraise")

    def __init__(self, reraise=False):
        self.value, self.exc, self.reraise = None, None, reraise

    def done(self):
        return self.value is not None or self.exc is not None

    def set_result(self, v):
        self.value = v

    def set_exception(self, e):
        if self.reraise:
            raise e
        self.exc = e


class SequenceScores:
    """What `batch_sequence_logprobs*` return, all float32 device tensors: `token_logprobs` [total] = log p(token | what
    precedes it) of every scored token, sequence after sequence (sequence i's are token_logprobs[starts[i]:starts[i + 1]],
    `starts` int64 [N + 1]); `logprobs` [N], their sums per sequence (0 for an empty continuation).  Under a constraint
    also `token_logZ` / `logZ` (log of the probability mass the constraint allowed at each position: what the fused step
    adds to a particle's log-weight - a pushed constraint's `start_logw` is not added) and `token_logprobs_masked` /
    `logprobs_masked` (log-probabilities under the constrained, renormalised distribution: -inf from a sequence's first
    forbidden token on); None without one."""

    FIELDS = ("token_logprobs", "token_logZ", "token_logprobs_masked")

    def __init__(self, starts, token_logprobs, logprobs, token_logZ=None, logZ=None, token_logprobs_masked=None,
                 logprobs_masked=None):
        self.starts, self.token_logprobs, self.logprobs = starts, token_logprobs, logprobs
        self.token_logZ, self.logZ = token_logZ, logZ
        self.token_logprobs_masked, self.logprobs_masked = token_logprobs_masked, logprobs_masked

    def __len__(self):
        return self.starts.numel() - 1

    def tolist(self, field="token_logprobs"):
        """Per-sequence Python lists of one per-token field (one D2H copy of it and of `starts`)."""
        if field not in self.FIELDS or getattr(self, field) is None:
            raise ValueError(f"no per-token field {field!r} in these scores")
        st, v = self.starts.tolist(), getattr(self, field).tolist()
        return [v[st[i]:st[i + 1]] for i in range(len(st) - 1)]


class AsyncAmdLM(AsyncLM):
    """Autobatching wrapper around a HuggingFace causal LM on one MI355X (hf.py:73-422)."""

    @classmethod
    def from_name(cls, model_id, bitsandbytes_opts=None, hf_opts=None, **kwargs):
        """hf.py:80-112.  bitsandbytes_opts: the dict the reference hands to transformers.BitsAndBytesConfig; the model is
        loaded as without it and its linear layers are then quantised to 4-bit NF4 / FP4 blocks by this library's own
        kernels (quant.py, DESIGN.md §14: `bitsandbytes` is not needed).  Served: load_in_4bit, bnb_4bit_quant_type "fp4"
        (default) / "nf4", bnb_4bit_compute_dtype, llm_int8_skip_modules; load_in_8bit, double quantisation, another
        quant storage and pre-quantised checkpoints raise NotImplementedError.  `self.quantization` holds the report."""
        from transformers import AutoModelForCausalLM, AutoTokenizer

        w4 = None
        if bitsandbytes_opts:
            from .quant import parse_opts

            w4 = parse_opts(bitsandbytes_opts)
        _hf_opts = {"torch_dtype": "auto"}
        if hf_opts:
            _hf_opts.update(hf_opts)
        device = _hf_opts.pop("device", None) or _hf_opts.pop("device_map", None) or "cuda:0"
        if device == "auto":
            device = "cuda:0"
        tok = AutoTokenizer.from_pretrained(model_id)
        mod = AutoModelForCausalLM.from_pretrained(model_id, **_hf_opts).to(device)
        if w4 is not None:
            kwargs = cls._quantize_own(mod, w4, kwargs)
        return cls(mod, tok, **kwargs)

    @staticmethod
    def _quantize_own(mod, w4, kwargs):
        """4-bit weights for a model this backend has just made (a model handed to the constructor is never rewritten)."""
        from .quant import quantize_model

        if getattr(mod.config, "quantization_config", None) is not None:
            raise NotImplementedError("a pre-quantised checkpoint (quantization_config in its config.json) is not served")
        kwargs = dict(kwargs)
        if kwargs.get("engine") is None:
            from .engine import HipEngine  # raises without the library / a HIP device

            kwargs["engine"] = HipEngine(mod.device, contract=kwargs.get("contract") or "auto")
        mod.eval()
        quantize_model(mod, w4, kwargs["engine"])
        return kwargs

    @classmethod
    def from_config(cls, config, tokenizer, device="cuda:0", dtype=torch.float32, seed=0, bitsandbytes_opts=None, **kwargs):
        """Random-init model of a given architecture (no hub access needed; synthetic benchmarks/tests).
        bitsandbytes_opts: as `from_name` (the model is quantised after it is made)."""
        from transformers import AutoModelForCausalLM

        w4 = None
        if bitsandbytes_opts:
            from .quant import parse_opts

            w4 = parse_opts(bitsandbytes_opts)

        torch.manual_seed(seed)
        n_params = getattr(config, "num_hidden_layers", 0) * getattr(config, "hidden_size", 0) ** 2 * 12
        if n_params > 2e9 and torch.device(device).type == "cuda":
            # a model of several billion parameters: made on the device in its own dtype (on the host it would first be
            # tens of GB of float32 and minutes of initialisation)
            old = torch.get_default_dtype()
            torch.set_default_dtype(dtype)
            try:
                with torch.device(device):
                    mod = AutoModelForCausalLM.from_config(config)
            finally:
                torch.set_default_dtype(old)
            mod = mod.to(dtype)
        else:
            mod = AutoModelForCausalLM.from_config(config).to(dtype).to(device)
        if w4 is not None:
            kwargs = cls._quantize_own(mod, w4, kwargs)
        return cls(mod, tokenizer, **kwargs)

    @staticmethod
    def _post_head(config):
        """What the model's own forward applies to `lm_head(hidden)` (the reference reads `model(...).logits`, hf.py:275):
        Cohere `logit_scale`, Granite `logits_scaling`, Gemma-2 `final_logit_softcapping`.  Returned as
        (multiplier, softcap); other families leave the head's output alone."""
        mult, cap = 1.0, None
        mt = getattr(config, "model_type", "")
        if mt.startswith("cohere") and getattr(config, "logit_scale", None) is not None:
            mult *= float(config.logit_scale)
        if mt.startswith("granite") and getattr(config, "logits_scaling", None):
            mult /= float(config.logits_scaling)
        if getattr(config, "final_logit_softcapping", None):
            cap = float(config.final_logit_softcapping)
        return mult, cap

    def _log_softmax(self, logits):
        """log-prob rows of `logits` in the dtype this backend returns (glb_log_softmax_rows)"""
        return self.engine.log_softmax_rows(logits, out_dtype=logits.dtype if self._lp_model_dtype else torch.float32)

    def _lm_head(self, hidden):
        """Logits of the given hidden rows exactly as `model(...).logits` has them: output embedding, then the
        family's post-head scaling / soft-capping."""
        x = self._head(hidden)
        if self._head_mult != 1.0:
            x = x * self._head_mult
        if self._head_cap is not None:
            x = torch.tanh(x / self._head_cap) * self._head_cap
        return x

    @torch.no_grad()
    def __init__(self, hf_model, hf_tokenizer, batch_size=20, timeout=0.02, engine=None, fuse_activations=True,
                 kv_budget_bytes=8 << 30, logprob_budget_bytes=16 << 30, auto_kv_rows=0, auto_kv_cap=64,
                 auto_kv_chunk=1, logprob_dtype="float32", glb_attention=True, merge_mlp=True, contract=None, gemms="library",
                 split_gemms=True, w4_gemm="auto", score_chunk_bytes=1 << 30):
        """The caller's `hf_model` is never modified (hf.py:114-140 leaves it alone too): with `fuse_activations` or
        `glb_attention` the forwards of this backend run on a private SHADOW of its module tree that shares every weight
        (fuse.shadow_model); `self.model` stays the caller's object.
        fuse_activations: in the shadow, GPT-2's eight-op `gelu_new` becomes one GELU kernel, Llama-family RMSNorm one
        `rms_norm` call, the rotary embedding three elementwise ops per tensor instead of six (same functions, different
        rounding); `merge_mlp` (Llama family): for few-token forwards gate_proj and up_proj are one GEMM on a derived
        [gate; up] weight - a second copy of those two matrices in device memory (False: not made).  glb_attention: the
        shadow's attention goes through this library's kernels where they apply (padded
        batches of short contexts: glb_short_attention; the in-place one-token forward over KV rows: glb_slab_attention),
        everything else still runs the SDPA path.  Both False: the forwards run on `hf_model` itself.
        logprob_dtype: "float32" (default: every row `next_token_logprobs` returns is float32, whatever the checkpoint's
        dtype) or "model" - rows in the model's own dtype, what the reference returns (cache.py:96 keeps the dtype; for a
        bfloat16 checkpoint a third fewer bytes per materialised row: glb_log_softmax_rows' out_dtype).
        auto_kv_rows > 0: `batch_next_token_step` keeps the KV of the contexts it evaluates in that many slab rows of
        `auto_kv_cap` positions and feeds one token to every context whose first L - 1 tokens it finds there
        (autokv.AutoKV; off by default: the reference re-encodes, hf.py:202-288).
        auto_kv_chunk = K, 1 .. 16 (needs auto_kv_rows): with K > 1 a context is served by ANY row it shares a prefix of
        `keep` >= 1 tokens with, provided the L - keep tokens behind it are at most K - they are fed in ONE forward and the
        row ends up holding the whole context (contexts that grew by several tokens, shrank and grew, or fork off a longer
        one; the reference's per-token KV, cache.py:103-191).  Everything else is encoded as before; 1 (default) is the
        one-token behaviour in every respect.  `_auto_kv.stats` counts `chunk_rows` / `chunk_tokens`.
        contract: "poly" / "hw" / "auto" - the arithmetic of the fused step's terms (HipEngine; None: the engine's own, "auto"
        for an engine made here: the hardware exponential for 16-bit logits, the polynomial for float32).
        gemms: "library" (default: PyTorch picks the GEMM kernels as it always does) or "recorded" - the forward's GEMM
        shapes run by the rocBLAS / hipBLASLt solution recorded for them in tuned/<arch>.csv (gemm_tuning: PyTorch TunableOp,
        a PROCESS-WIDE switch that also reaches the caller's other GEMMs; 8-10 % of a step at 1024 particles; silently the
        library's defaults when the file was made by another build of the libraries - `self.gemm_shapes` says how many
        shapes were taken over).  `close()` gives the switch back.
        split_gemms: in the shadow, GPT-2's float32 Conv1D projections run this library's split-bf16 MFMA GEMM (fuse.py
        SplitConv1D: fp32-accurate, the MLP's tanh GELU in its epilogue) for the batch sizes where it was measured faster
        than the library; it keeps a derived bf16 image of each such weight (6 bytes per element: 510 MB for GPT-2 small).
        `gemms` still decides every GEMM this path does not take.  False: not swapped.
        w4_gemm: how the 4-bit layers of a quantised model (quant.W4Linear) multiply - "auto": glb_w4_gemm on the 4-bit image
        for the row counts where it was measured faster (quant.MIN_ROWS_FUSED), dequantise + library GEMM otherwise;
        "fused" / "dequant": one path wherever it is able to serve the call (tests, A/Bs).
        score_chunk_bytes: the most logits bytes `batch_sequence_logprobs*` hold at a time (never above logprob_budget_bytes;
        always at least one row)."""
        if score_chunk_bytes <= 0:
            raise ValueError(f"score_chunk_bytes must be positive, got {score_chunk_bytes!r}")
        self.score_chunk_bytes = min(int(score_chunk_bytes), int(logprob_budget_bytes))
        self.model = hf_model
        self.tokenizer = hf_tokenizer
        self.device = hf_model.device
        if gemms not in ("library", "recorded"):
            raise ValueError(f"gemms must be 'library' or 'recorded', got {gemms!r}")
        self.gemms, self.gemm_shapes = gemms, 0
        if gemms == "recorded" and self.device.type == "cuda":
            from . import gemm_tuning

            self.gemm_shapes = gemm_tuning.acquire(self.device)
            self._gemms_held = True
        if engine is None:
            from .engine import HipEngine  # raises without the library / a HIP device

            engine = HipEngine(self.device, contract=contract or "auto")
        elif contract is not None:
            if contract not in engine.CONTRACTS:
                raise ValueError(f"contract must be one of {engine.CONTRACTS}, got {contract!r}")
            engine.contract = contract
        self.engine = engine
        from .quant import W4_GEMM_MODES

        if w4_gemm not in W4_GEMM_MODES:
            raise ValueError(f"w4_gemm must be one of {W4_GEMM_MODES}, got {w4_gemm!r}")
        self.w4_gemm = w4_gemm
        self.quantization = hf_model.__dict__.get("_glb_quantization")  # quantize_model's report; None: not quantised
        if logprob_dtype not in ("float32", "model"):
            raise ValueError(f"logprob_dtype must be 'float32' or 'model', got {logprob_dtype!r}")
        self._lp_model_dtype = logprob_dtype == "model"
        self.cache = TokenTrie()
        self.queries = []
        self._sq = None  # pending `next_token_step` requests without a cached prefix: [contexts, mask ids, ONE future]
        self.batch_size = batch_size
        self.timeout = timeout
        self.timer = None
        self.model.eval()
        self.glb_attention = False
        self.fused = []
        self._net = self.model  # what this backend's forwards run on: the caller's model, or its shadow
        want_attention = bool(glb_attention) and self.device.type == "cuda"
        if fuse_activations or want_attention:
            from .fuse import fuse_shadow, shadow_model

            self._net = shadow_model(self.model)
            split_engine = self.engine if split_gemms and self.device.type == "cuda" else None
            self.fused = fuse_shadow(self._net, activations=bool(fuse_activations), merge_mlp=bool(merge_mlp),
                                     split_engine=split_engine)
            if want_attention:
                from .kv import use_glb_attention

                self.glb_attention = use_glb_attention(self._net, self.engine)
        from .quant import bind as _bind_w4

        _bind_w4(self._net, self.engine, w4_gemm)
        self._head = self._net.get_output_embeddings()
        if self._head is None:
            raise NotImplementedError(f"{type(hf_model).__name__} has no output embedding (get_output_embeddings() is None)")
        self._head_mult, self._head_cap = self._post_head(self.model.config)
        self._body = self._net.base_model
        self._kv_tokens = {}  # id(trie node) -> the prefix's token ids (for the device prefix table)
        self._ptab = None
        # prompt prefixes pinned by cache_kv, least recently used out first; an entry that leaves the store takes its
        # token tuple and the device prefix table (which holds pointers into its slabs) with it
        self._kv_lru = PrefixLRU(kv_budget_bytes, on_remove=self._forget_prefix)
        # log-prob rows on trie nodes: views into their batch's [R, V] slab, least recently used slab out first
        self._rows = RowLRU(logprob_budget_bytes)
        # KV rows that follow the contexts handed to batch_next_token_step (off unless auto_kv_rows > 0)
        self._auto_kv = None
        if isinstance(auto_kv_chunk, bool) or not isinstance(auto_kv_chunk, int) or not 1 <= auto_kv_chunk <= 16:
            raise ValueError(f"auto_kv_chunk must be an integer from 1 to 16, got {auto_kv_chunk!r}")
        if auto_kv_chunk > 1 and not auto_kv_rows:
            raise ValueError("auto_kv_chunk > 1 needs auto_kv_rows: there are no KV rows to share prefixes in")
        if auto_kv_rows:
            from .autokv import AutoKV

            self._auto_kv = AutoKV(self, auto_kv_rows, auto_kv_cap, chunk=auto_kv_chunk)
        # fused-step state
        self.masks = RegisteredMasks(self.engine)  # what register_masks was given (masks.py)
        self._rng_mode = RNG_PHILOX
        self._rng_seed = 0
        self._noise_src = None  # "torch" draws: the CPU generator's stream on the device, made at the first evaluation
        self._batch_counter = 0
        self.stats = {"batches": 0, "queries": 0, "unique": 0, "rows": 0, "lora_rows_calls": 0}
        self._loras = {}  # name -> lora.LoraAdapter (loaded, validated)
        self._row_lora = None  # lora.RowLora over the loaded adapters (made at the first call that names adapters per context)
        self._lora = None  # lora.MergedLora of the active adapter
        self.lora_epoch = 0  # moves at every set_lora / clear_lora
        if hf_tokenizer is not None:
            super().__init__(tokenizer=self.tokenizer)
        else:  # model-only use (synthetic benchmarks): no vocabulary to decode
            self.byte_vocab, self.str_vocab = None, None

    def refresh_weights(self):
        """Call after changing the model's weights in a way PyTorch's version counters do not see.  The shadow keeps derived
        copies of some weights ([q; k; v] and [gate; up] as one matrix each, the split GEMM's bf16 images: fuse.py) and captured hipGraphs of the
        one-token forward read the copies they were captured with; both notice `param.copy_()` / `param.mul_()` and replaced
        parameters by themselves (`Tensor._version`, identity, address), but NOT writes through `param.data` (EMA and
        weight-merging code does that: `p.data.copy_(...)` bumps no counter and moves no address).  This drops every
        derived copy and every captured graph - they are rebuilt from the current weights at the next forward -, merges an
        active LoRA adapter again, and drops the cached log-prob rows and KV (made with the old weights: clear_cache())."""
        for mod in self._net.modules():
            mod.__dict__.pop("_glb_qkv", None)
            mod.__dict__.pop("_glb_gate_up", None)
            mod.__dict__.pop("_glb_split", None)
        if self._lora is not None:  # an active adapter is merged again from the current base weights
            self._lora.uninstall()
            from .lora import MergedLora

            self._lora = MergedLora(self._lora.adapter, self._net, self.engine)
        self.weights_epoch = getattr(self, "weights_epoch", 0) + 1  # SlabForward drops its graphs when this moves
        self.clear_cache()

    def close(self):
        """Give back what this backend holds of the process's state: the recorded GEMM solutions (gemms="recorded").  The
        object stays usable (its GEMMs then run by the library's defaults); safe to call more than once."""
        if getattr(self, "_gemms_held", False):
            from . import gemm_tuning

            self._gemms_held = False
            self.gemm_shapes = 0
            gemm_tuning.release()

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    @property
    def _pad_id(self):
        pad_id = getattr(self.tokenizer, "pad_token_id", None) if self.tokenizer is not None else None
        return 0 if pad_id is None else pad_id

    def _forget_prefix(self, node):
        self._kv_tokens.pop(id(node), None)
        self._ptab = None

    # ---- cache management (hf.py:142-164) ---------------------------------------------------------
    def clear_cache(self):
        self._kv_lru.clear()
        self._kv_tokens.clear()
        self._rows.clear()
        self.cache = TokenTrie()
        if self._auto_kv is not None:
            self._auto_kv.reset()

    def clear_kv_cache(self):
        self._kv_lru.clear()
        self.cache.clear_kv_cache()
        if self._auto_kv is not None:
            self._auto_kv.reset()

    def reset_async_queries(self):
        self.queries = []
        self._sq = None

    @torch.no_grad()
    def cache_kv(self, prompt_tokens):
        """hf.py:155-164: run the prompt once, cache every position's log-probs and keep the KV states
        on the prompt's last node so later queries only feed their new tokens."""
        self._lora_sync()
        key = tuple(int(t) for t in prompt_tokens)
        # extend_cache makes fresh nodes, so caching the same prompt again (or one that shares leading tokens) orphans
        # the node that held the KV so far: its entry leaves the store instead of lingering under the budget
        for old in [n for n in self._kv_lru.nodes() if self._kv_tokens.get(id(n)) == key]:
            self._kv_lru.drop(old)
        ids = torch.tensor([prompt_tokens], device=self.device)
        out = self._body(input_ids=ids, use_cache=True)
        logits = self._lm_head(out.last_hidden_state[0])
        node = self.cache.extend_cache(0, prompt_tokens, logits, 0, engine=self.engine, store=self._rows,
                                       out_dtype=logits.dtype if self._lp_model_dtype else None)
        # (re-created ancestors: an older, shorter prefix whose node was replaced on the way is unreachable from the
        # trie now and would only hold memory)
        reach = set()
        walk = self.cache
        for t in prompt_tokens:
            if not walk.has_token(t):
                break
            walk = walk.get_token(t)
            reach.add(id(walk))
        for old in self._kv_lru.nodes():
            toks = self._kv_tokens.get(id(old))
            if toks is not None and len(toks) <= len(key) and key[:len(toks)] == toks and id(old) not in reach:
                self._kv_lru.drop(old)
        # pinned under a byte budget: the least recently used prefix loses its KV (its log-prob rows stay), the policy
        # of cache.py:103-191 applied to whole prefix slabs
        self._kv_lru.put(node, KVPrefix.from_hf_cache(out.past_key_values))
        self._kv_tokens[id(node)] = key
        self._ptab = None

    # ---- LoRA adapters (hf.py:166-200): merged into private weights of the shadow (lora.py) ----------
    def add_new_lora(self, lora_path, lora_name="lora_1"):
        """Load a peft LoRA adapter (a local directory or a hub id) and check it against the model; it is not activated
        (`set_lora` does that).  A name that is already loaded raises ValueError, as transformers' load_adapter does."""
        from .lora import load_adapter

        if lora_name in self._loras:
            raise ValueError(f"Adapter with name {lora_name} already exists. Please use a different name.")
        self._loras[lora_name] = load_adapter(lora_path, self.model, lora_name)
        self._row_lora = None  # (its table lists the loaded adapters)
        self._lora_stats()

    def set_lora(self, lora_path=None, lora_name="lora_1"):
        """Activate a loaded adapter: its targeted weights become W + s * B . A (one glb_lora_merge call into private
        tensors of the shadow; the caller's model is not touched), every cache made with other weights is dropped, and
        DeviceSIS / DeviceSampler objects made before refuse to step."""
        if lora_name not in self._loras:
            raise ValueError(
                f"A LoRA adapter named '{lora_name}' has not been loaded yet. Please call add_new_lora() first to load and "
                "name your LoRA adapters."
            )
        try:
            self._drop_lora()
            self._ensure_shadow()  # (fuse_activations=False, glb_attention=False: one to merge into)
            from .lora import MergedLora

            self._lora = MergedLora(self._loras[lora_name], self._net, self.engine)
        finally:  # (also when the merge fails: the old adapter is gone, and what was made with it must go too)
            self._weights_switched()

    def _ensure_shadow(self):
        if self._net is self.model:
            from .fuse import shadow_model

            self._net = shadow_model(self.model)
            self._head = self._net.get_output_embeddings()
            self._body = self._net.base_model
            self._row_lora = None

    def clear_lora(self):
        """Back to the base weights: the shared parameter tables return and the merged tensors are freed, so results are
        bit-identical to a backend that never saw an adapter.  Clears the caches also when no adapter is active."""
        self._drop_lora()
        self._weights_switched()

    @property
    def active_lora(self):
        """Name of the active adapter, or None."""
        return None if self._lora is None else self._lora.adapter.name

    def _drop_lora(self):
        if self._lora is not None:
            self._lora.uninstall()
            self._lora = None
            for mod in self._net.modules():  # derived copies of merged weights go with them (rebuilt from the base)
                mod.__dict__.pop("_glb_qkv", None)
                mod.__dict__.pop("_glb_gate_up", None)
                mod.__dict__.pop("_glb_split", None)

    def _weights_switched(self):
        self.lora_epoch += 1  # DeviceSIS objects made before refuse to step
        self.weights_epoch = getattr(self, "weights_epoch", 0) + 1  # SlabForward drops its graphs
        self.clear_kv_cache()
        self.clear_cache()
        self._lora_stats()

    def _lora_stats(self):
        self.stats["lora_merged_bytes"] = 0 if self._lora is None else self._lora.nbytes()
        self.stats["lora_adapter_bytes"] = sum(a.nbytes() for a in self._loras.values())

    def _lora_sync(self, epoch=None):
        """Before a batch evaluates: an object made under other weights (`epoch`: the lora_epoch it was made at) raises;
        an active adapter whose base weights changed since the merge is merged again (SlabForward's graphs are dropped)."""
        if epoch is not None and epoch != self.lora_epoch:
            raise RuntimeError("the LoRA adapter changed (set_lora / clear_lora) after this object was made: its KV was "
                               "computed with other weights - make a new one")
        if self._lora is not None and self._lora.sync():
            self.weights_epoch = getattr(self, "weights_epoch", 0) + 1
            self._lora_stats()

    # ---- fused-step configuration -------------------------------------------------------------------
    def register_masks(self, masks):
        """masks: float tensor [K, V] (or list of [V]) of additive log-masks (README.md:57-70).  {0,-inf}
        masks are packed to bit rows on the device; anything else is kept as float."""
        if isinstance(masks, (list, tuple)):
            masks = torch.stack([m.to(torch.float32) for m in masks])
        masks = masks.to(self.device, torch.float32).contiguous()
        self.masks.register(masks)
        return masks.shape[0]

    def step_masks(self, logits_dtype):
        """Mask arguments of `HipEngine.step` for logits of `logits_dtype`: bit masks are brought into the kernels'
        layout once per element width (glb_mask_prepare) and reused by every step."""
        return self.masks.tables(logits_dtype)

    _mask_kind = property(lambda self: self.masks.kind)

    def _fused_step(self, logits, row_of, ids, by_row, n, noise_groups, constraint=None):
        """The fused step over logits rows for n contexts (row_of: the logits row of each): the masks of `constraint`, else
        the registered ones, by `ids` (per logits row when `by_row`, else per context); in parity mode the Exp(1) rows in the
        reference's resolution order - by dedup group `noise_groups`, duplicates contiguous (hf.py:285-288); None: the
        contexts are in that order already.  Returns (logZ, token) device tensors."""
        eng, V, parity = self.engine, logits.shape[-1], self._rng_mode == RNG_NOISE
        kw, _ = (self.masks if constraint is None else constraint).step_masks(logits, ids, by_row, n, parity=parity)
        if parity:
            slot = None
            if noise_groups is not None:
                order = torch.argsort(noise_groups.to(torch.int64), stable=True)
                slot = torch.empty(n, dtype=torch.int32, device=self.device)
                slot[order] = torch.arange(n, dtype=torch.int32, device=self.device)
            kw["noise"] = self._noise_rows(V).rows(n, row_slot=slot)
        logZ, _, tok = eng.step(logits, vocab=V, row_of=row_of, rng_mode=self._rng_mode, seed=self._rng_seed,
                                offset=self._batch_counter, want_lse=False, **kw)
        return logZ, tok

    def set_rng(self, mode="philox", seed=0):
        """"philox": in-kernel counter RNG (fast).  "torch": parity with the reference's CPU
        torch.multinomial under torch.manual_seed(seed) (README.md:87): the exponentials come from the same MT19937
        stream, in the reference's particle order - generated on the device (engine.DeviceRng)."""
        if mode == "philox":
            self._rng_mode, self._rng_seed, self._noise_src = RNG_PHILOX, int(seed), None
        elif mode == "torch":
            self._rng_mode, self._rng_seed, self._noise_src = RNG_NOISE, int(seed), None
        else:
            raise ValueError(f"unknown rng mode {mode!r}")
        self._batch_counter = 0

    def _noise_rows(self, V):
        if self._noise_src is None:
            self._noise_src = self.engine.noise_rng(self._rng_seed, V)
        return self._noise_src

    # ---- the batched evaluation (hf.py:202-288) -------------------------------------------------------
    @torch.no_grad()
    def batch_evaluate_queries(self):
        self._fire_step_batch()
        queries, self.queries = self.queries, []
        if len(queries) == 0:
            return
        try:
            self._evaluate(queries)
        except Exception as e:  # vllm.py:396-400 behaviour: nobody is left waiting
            stranded = [q.future for q in queries if q.future is not None and not q.future.done()]
            for f in stranded:
                f.set_exception(e)
            if not stranded:
                raise

    def _evaluate(self, queries):
        self._lora_sync()
        if all(q.kind == "step" and q.past is None for q in queries):
            return self._evaluate_steps(queries)
        if (self._auto_kv is not None and not self._kv_tokens
                and all(q.kind == "logprobs" and q.past is None and q.first_new == len(q.prompt) - 1 for q in queries)):
            return self._evaluate_last_rows(queries)
        return self._evaluate_encoded(queries)

    def _count(self, n, unique, rows):
        """One evaluated batch of n requests in `stats`; the fused step's draws move on with it (`_batch_counter`)."""
        self._batch_counter += 1
        self.stats["batches"] += 1
        self.stats["queries"] += n
        self.stats["unique"] += unique
        self.stats["rows"] += rows

    def _evaluate_steps(self, queries):
        # a population of README particles (README.md:82-91) and no cached prefix: the whole batch goes through the
        # vectorised pipeline of batch_next_token_step_sync - three host arrays in, two out, one loop to resolve
        logZ, tok = self.batch_next_token_step_sync([q.prompt for q in queries], [q.mask_id for q in queries])
        for q, z, t in zip(queries, logZ.tolist(), tok.tolist()):
            if q.future is not None and not q.future.done():
                q.future.set_result((z, t))

    def _evaluate_last_rows(self, queries):
        # every request wants the row after its LAST token only (its shorter prefixes are in the trie - a population
        # that grew by one token): the contexts find their KV rows (autokv.AutoKV) and one token each is fed
        eng, dev = self.engine, self.device
        tok_d, st_d, ln_d = (torch.from_numpy(a).to(dev) for a in ragged([q.prompt for q in queries]))
        group_of, rep, ng = eng.group_contexts(tok_d, st_d, ln_d)
        logits, row_of_group, _, U, _ = self._auto_kv.logits(tok_d, st_d, ln_d, group_of, rep, ng)
        lp = self._log_softmax(logits)
        rows = torch.cat([row_of_group[group_of.long()], eng.error_word()]).cpu().tolist()
        eng.raise_if_failed(rows.pop(), what="glb_log_softmax_rows")  # no NaN row may reach the trie
        self._count(len(queries), U, U)
        for q, r in zip(queries, rows):
            if q.future is not None and not q.future.done():
                q.future.set_result((lp, r, q.first_new))

    def _evaluate_encoded(self, queries):
        """The re-encoding path (hf.py:202-288): requests of both kinds, with or without a `cache_kv` prefix."""
        eng, dev = self.engine, self.device
        n = len(queries)
        # -- flatten: context i = [prefix slot, past_len, prompt...]; two header words make the dedup key
        #    (hf.py:216 keys on the prompt only; adding the prefix identity cannot merge unequal requests)
        prefixes, prefix_slot = [], {}
        lens = np.fromiter((len(q.prompt) + 2 for q in queries), np.int32, n)
        starts = np.zeros(n, np.int64)
        starts[1:] = np.cumsum(lens[:-1])
        flat = np.empty(int(lens.sum()), np.int32)
        for i, q in enumerate(queries):
            slot = 0
            if q.past is not None:
                key = id(q.past)
                if key not in prefix_slot:
                    prefix_slot[key] = len(prefixes) + 1
                    prefixes.append(q.past)
                slot = prefix_slot[key]
            s = starts[i]
            flat[s] = slot
            flat[s + 1] = q.past_len
            flat[s + 2:s + lens[i]] = q.prompt
        tok_d, st_d, ln_d = (torch.from_numpy(a).to(dev) for a in (flat, starts, lens))

        # -- shared-prefix dedup on the device, first-appearance order (glb_group_contexts)
        group_of_d, rep_d, ng_d = eng.group_contexts(tok_d, st_d, ln_d)
        U = int(ng_d.item())
        group_of = group_of_d.cpu().numpy()
        rep = rep_d[:U].cpu().numpy()
        uniq = [queries[r] for r in rep]
        members = [[] for _ in range(U)]
        for i, g in enumerate(group_of):
            members[g].append(queries[i])

        p_max = max(q.past_len for q in uniq)
        l_max = max(len(q.prompt) for q in uniq)

        # -- the ragged batch as the gather takes it: starts/lengths are shifted so that
        #    tokens[start + base + t] is prompt token t, with base = past_len.
        past_len = np.array([q.past_len for q in queries], np.int32)
        base_d = torch.from_numpy(past_len).to(dev)
        st_adj = st_d + 2 - base_d.to(torch.int64)
        ln_adj = ln_d - 2 + base_d

        # -- batched prefix KV: a table of this batch's prefixes alone (it checks that they share one KV shape).  Every
        #    prefix is some unique query's: the table's longest is p_max
        prefixes_u = None
        if p_max > 0:
            slot_of_u = np.array([prefix_slot[id(q.past)] - 1 if q.past is not None else -1 for q in uniq], np.int32)
            prefixes_u = (PrefixTable([(p, None) for p in prefixes], dev), torch.from_numpy(slot_of_u).to(dev))

        # -- padded gather, prefix KV, transformer body (kv.encode_ragged)
        hidden = encode_ragged(self, (tok_d, st_adj, ln_adj), rep_d, U, l_max, pad_id=self._pad_id, base=base_d,
                               prefixes=prefixes_u).hidden  # [U, l_max, d]

        # -- which (unique, position) rows are needed: log-prob queries want every new position,
        #    step queries only the last one
        row_u, row_t, lp_rows, step_row = [], [], {}, {}
        for u, q in enumerate(uniq):
            L = len(q.prompt)
            lp_first = min((m.first_new for m in members[u] if m.kind == "logprobs"), default=None)
            if lp_first is not None:
                lp_rows[u] = (len(row_u), lp_first)
                for t in range(lp_first, L):
                    row_u.append(u)
                    row_t.append(t)
                step_row[u] = len(row_u) - 1
            elif any(m.kind == "step" for m in members[u]):
                step_row[u] = len(row_u)
                row_u.append(u)
                row_t.append(L - 1)
        ru = torch.from_numpy(np.asarray(row_u, np.int64)).to(dev)
        rt = torch.from_numpy(np.asarray(row_t, np.int64)).to(dev)
        logits = self._lm_head(hidden[ru, rt])  # [R, V] plain library GEMM on the gathered rows
        R, V = logits.shape

        # -- log-prob rows in one launch (glb_log_softmax_rows; replaces cache.py:93-98)
        lp_slab, slab_row = None, None
        if lp_rows:
            need = sorted(r for u, (r0, f) in lp_rows.items() for r in range(r0, r0 + len(uniq[u].prompt) - f))
            if len(need) == R:
                lp_slab = self._log_softmax(logits)
            else:
                idx = torch.from_numpy(np.asarray(need, np.int64)).to(dev)
                lp_slab = self._log_softmax(logits[idx].contiguous())
                slab_row = {r: i for i, r in enumerate(need)}

        # -- fused step for every step query, in resolution order (group order, duplicates contiguous)
        step_q = [(u, m) for u in range(U) for m in members[u] if m.kind == "step"]
        step_out = None
        if step_q:
            row_of = torch.from_numpy(np.fromiter((step_row[u] for u, _ in step_q), np.int32, len(step_q))).to(dev)
            mask_id = torch.from_numpy(np.fromiter((m.mask_id for _, m in step_q), np.int32, len(step_q))).to(dev)
            # (step_q is in resolution order already: by group, duplicates contiguous)
            logZ, tok = self._fused_step(logits, row_of, mask_id, False, len(step_q), None)
            step_out = (logZ.cpu().tolist(), tok.cpu().tolist())
            eng.raise_if_failed(tokens=step_out[1])
        if lp_slab is not None:  # no NaN row may reach the trie: the error word of the log-softmax launch (one small copy)
            eng.raise_if_failed(int(eng.error_word().item()), what="glb_log_softmax_rows")
        self._count(n, U, R)

        # -- fan out (hf.py:285-288 order)
        si = 0
        for u in range(U):
            rows = None
            if u in lp_rows:
                r0, first = lp_rows[u]
                # (slab, index of the row of position `first`, first): no view per query
                rows = (lp_slab, r0 if slab_row is None else slab_row[r0], first)
            for m in members[u]:
                if m.kind == "step":
                    res = (step_out[0][si], step_out[1][si])
                    si += 1
                else:
                    res = rows
                if m.future is not None and not m.future.done():
                    m.future.set_result(res)

    # ---- queueing (hf.py:290-312) -----------------------------------------------------------------------
    def add_query(self, query, future, past, first_new=0, kind="logprobs", mask_id=0):
        """hf.py:290-312: queue the request; evaluate when the batch is full or `timeout` after the LAST request.
        (The reference cancels and re-arms its timer on every request; here one timer re-checks a moving deadline,
        which fires at the same moment without 2 x batch_size timer operations per batch.)"""
        self.queries.append(Query(query, future, past, first_new=first_new, kind=kind, mask_id=mask_id))
        if len(self.queries) >= self.batch_size:
            if self.timer:
                self.timer.cancel()
                self.timer = None
            self.batch_evaluate_queries()
        else:
            loop = asyncio.get_running_loop()
            self._deadline = loop.time() + self.timeout
            if self.timer is None:
                self.timer = loop.call_later(self.timeout, self._on_timer)

    def _on_timer(self):
        self.timer = None
        if not self.queries and self._sq is None:
            return
        loop = asyncio.get_running_loop()
        remaining = self._deadline - loop.time()
        if remaining > 1e-4:
            self.timer = loop.call_later(remaining, self._on_timer)
        else:
            self.batch_evaluate_queries()

    def walk_cache(self, token_ids):
        """hf.py:314-344: deepest matching node, tokens matched, deepest KV on the way and its depth."""
        node = self.cache
        prev = None
        next_token_index = 0
        past = None
        base = 0
        while next_token_index < len(token_ids):
            if node.past_key_values is not None:
                past = node.past_key_values
                base = next_token_index
                self._kv_lru.touch(node)
            if node.has_token(token_ids[next_token_index]):
                prev, node = node, node.get_token(token_ids[next_token_index])
                next_token_index += 1
            else:
                break
        if next_token_index == len(token_ids) and prev is not None:
            if not node.has_row():  # the row was evicted under the byte budget (RowLRU): a miss on the last position
                node, next_token_index = prev, next_token_index - 1
            else:
                self._rows.touch(node)
        return node, next_token_index, past, base

    async def next_token_logprobs(self, token_ids):
        """hf.py:346-373.  Returns a float32 [V] tensor on the model's device."""
        if not token_ids:
            raise ValueError("Token ids must not be empty")
        node, next_token_index, past, base = self.walk_cache(token_ids)
        if next_token_index == len(token_ids):
            return node.logprobs
        future = asyncio.get_running_loop().create_future()
        self.add_query(token_ids[base:], future, past, first_new=next_token_index - base)
        slab, row0, first = await future  # slab[row0 + t - first]: the row after prompt position t (= context position base + t)
        t, i = node.extend_cache_lazy(next_token_index, token_ids, slab, base + first - row0, store=self._rows)
        return t[i]

    def _evaluate_one(self, prompt, past, first_new):
        """Synchronous single-query evaluation through the same batched machinery."""
        slot = _Slot()
        self._evaluate([Query(prompt, slot, past, first_new=first_new)])
        return slot.value

    @torch.no_grad()
    def next_token_logprobs_sync(self, token_ids):
        """hf.py:375-402 (uses the walked KV prefix; the reference passes the matched node's, hf.py:396)."""
        if not token_ids:
            raise ValueError("Token ids must not be empty")
        node, next_token_index, past, base = self.walk_cache(token_ids)
        if next_token_index == len(token_ids):
            return node.logprobs
        slab, row0, first = self._evaluate_one(token_ids[base:], past, next_token_index - base)
        t, i = node.extend_cache_lazy(next_token_index, token_ids, slab, base + first - row0, store=self._rows)
        return t[i]

    @torch.no_grad()
    def next_token_logprobs_uncached(self, token_ids):
        """hf.py:404-422: no KV, no output cache, no batching."""
        if not token_ids:
            raise ValueError("Token ids must not be empty")
        self._lora_sync()
        ids = torch.tensor([token_ids], device=self.device)
        h = self._body(input_ids=ids, use_cache=False).last_hidden_state[0, -1:]
        return self._log_softmax(self._lm_head(h))[0]  # (a single row: the three-launch form, no waits inside)

    # ---- fused particle step (README.md:82-91 moved behind the queue) ------------------------------------
    async def next_token_step(self, token_ids, mask_id=0):
        """Returns (logZ, token): logZ = logsumexp(next_token_logprobs + mask[mask_id]) and a categorical
        draw from the masked, renormalised distribution; token is -1 if the mask forbids everything."""
        if not token_ids:
            raise ValueError("Token ids must not be empty")
        if len(self._kv_lru):  # a cached KV prefix may serve this request: the trie walk finds it, the request is queued on its own
            _node, _n, past, base = self.walk_cache(token_ids)
            future = asyncio.get_running_loop().create_future()
            self.add_query(token_ids[base:] if base else token_ids, future, past, kind="step", mask_id=mask_id)
            return await future
        # No prefix is cached, so there is nothing to walk and nothing per-request to keep: the requests of a batch share
        # ONE future (a population of README particles awaits the same evaluation, hf.py:290-312's queue without a future,
        # a Query object and a timer operation per particle) and pick their slot out of its result.
        sq = self._sq
        if sq is None:
            sq = self._sq = ([], [], asyncio.get_running_loop().create_future())
        slot = len(sq[0])
        sq[0].append(token_ids)
        sq[1].append(mask_id)
        if slot + 1 + len(self.queries) >= self.batch_size:
            if self.timer:
                self.timer.cancel()
                self.timer = None
            self.batch_evaluate_queries()
        else:
            loop = asyncio.get_running_loop()
            self._deadline = loop.time() + self.timeout
            if self.timer is None:
                self.timer = loop.call_later(self.timeout, self._on_timer)
        logZ, tok = await sq[2]
        return logZ[slot], tok[slot]

    async def gather(self, *coros, return_exceptions=False):
        """`asyncio.gather` for coroutines that spend their time awaiting THIS backend (a population of README particles:
        `await llm.gather(*[p.extend() for p in particles])`), without a Task per coroutine.  asyncio.gather wraps every
        coroutine in a Task: creating it, one trip through the event loop to start it, one to wake it when the shared
        future resolves and one done-callback cost CPython ~15 us per particle and step - at 1024 particles more than
        the step on the GPU takes.  Here the coroutines are advanced by hand (`send`): each runs to the point where it
        awaits this backend, the queued requests are evaluated as one batch, each is resumed with the result.  A
        coroutine that awaits something else (a foreign future, `asyncio.sleep`) is simply awaited from here, so any
        coroutine works - only slower.  Results in argument order; the first exception closes the other coroutines and
        propagates (with `return_exceptions` it takes the failed coroutine's place in the results, as in asyncio).
        No counterpart in the reference (its callers use asyncio.gather, README.md:96)."""
        n = len(coros)
        results = [None] * n
        live = list(range(n))   # coroutines that have not finished
        blocked = [None] * n    # what coroutine i is waiting for: a future, or None = ready to be resumed
        try:
            while live:
                nxt = []
                for i in live:
                    fut = blocked[i]
                    if fut is not None and not fut.done():
                        nxt.append(i)
                        continue
                    blocked[i] = None
                    try:
                        y = coros[i].send(None)
                    except StopIteration as e:
                        results[i] = e.value
                        continue
                    except Exception as e:
                        if not return_exceptions:
                            raise
                        results[i] = e
                        continue
                    if y is not None:  # `await future`: the future itself comes out (asyncio's protocol), flagged as awaited
                        if getattr(y, "_asyncio_future_blocking", None) is None:
                            raise RuntimeError(f"coroutine yielded {y!r}: not an asyncio awaitable")
                        y._asyncio_future_blocking = False
                        blocked[i] = y
                    nxt.append(i)
                live = nxt
                if not live:
                    break
                did_batch = bool(self.queries or self._sq is not None)
                if did_batch:
                    if self.timer:
                        self.timer.cancel()
                        self.timer = None
                    self.batch_evaluate_queries()  # everything queued so far is one batch: its futures resolve here
                waiting = [blocked[i] for i in live if blocked[i] is not None and not blocked[i].done()]
                if waiting and len(waiting) == len(live):
                    await asyncio.wait(waiting, return_when=asyncio.FIRST_COMPLETED)  # (foreign futures: the event loop's business)
                elif not did_batch:
                    # nothing of this pass was this backend's to resolve - coroutines polling with bare yields, possibly
                    # next to others blocked on foreign futures: the event loop (its timers, the futures' owners) gets its turn
                    await asyncio.sleep(0)
        except BaseException as exc:
            for i in live:
                coros[i].close()
            # what the closed coroutines had queued must not ride into somebody else's next batch: fail it (nobody is left
            # waiting on a future that would never resolve)
            self._fail_pending(exc if isinstance(exc, Exception) else asyncio.CancelledError())
            raise
        return results

    def _fail_pending(self, exc):
        """Drop everything queued and not yet evaluated; its futures get `exc`."""
        sq, self._sq = self._sq, None
        if sq is not None and not sq[2].done():
            sq[2].set_exception(exc)
            sq[2].exception()  # (marked retrieved: a gather that was abandoned has nobody left to read it)
        queries, self.queries = self.queries, []
        for q in queries:
            if q.future is not None and not q.future.done():
                q.future.set_exception(exc)
        if self.timer:
            self.timer.cancel()
            self.timer = None

    def _fire_step_batch(self):
        """Evaluate the pending `next_token_step` requests (one vectorised call) and resolve their shared future."""
        sq, self._sq = self._sq, None
        if sq is None:
            return
        contexts, mask_ids, future = sq
        try:
            logZ, tok = self.batch_next_token_step_sync(contexts, mask_ids)
        except Exception as e:  # vllm.py:396-400 behaviour: nobody is left waiting
            if not future.done():
                future.set_exception(e)
            return
        if not future.done():
            future.set_result((logZ.tolist(), tok.tolist()))

    # ---- batched submit: a whole population per call (no per-query futures, no per-query Python) ----------------------
    def _prefix_table(self):
        """The prompts whose KV `cache_kv` holds: their device table (kv.PrefixTable; None when there are none), their
        trie nodes and their number; rebuilt when the set of cached prefixes changed."""
        entries = [(node, self._kv_tokens.get(id(node))) for node, _ in self._kv_lru._od.values()]
        entries = [(n, t) for n, t in entries if t is not None and n.past_key_values is not None]
        key = tuple(id(n) for n, _ in entries)
        if self._ptab is not None and self._ptab["key"] == key:
            return self._ptab
        table = PrefixTable([(n.past_key_values, t) for n, t in entries], self.device) if entries else None
        self._ptab = dict(key=key, n=len(entries), nodes=[n for n, _ in entries], table=table)
        return self._ptab

    @torch.no_grad()
    def batch_next_token_step_sync(self, contexts, mask_ids=None, lora_names=None):
        """README.md:82-87 for a whole population in ONE call: for every context, logZ = logsumexp(next-token
        log-probs + mask[mask_id]) and a draw from the masked, renormalised distribution (-1 if nothing is allowed).
        Same pipeline as the queued `next_token_step` - dedup (hf.py:214-220), cached-prefix match (hf.py:334-342),
        ragged-to-padded gather, forward, lm_head on the last position, fused step - but the ragged batch is built
        once (three host arrays) and nothing is done per query in Python.  Returns (logZ float32 [n], token int32 [n])
        as NumPy arrays.
        lora_names: one entry per context - a name given to `add_new_lora`, or None for the base model; the contexts are
        then evaluated in ONE forward with each context's adapter applied unmerged (`_lora_rows_logits`)."""
        dev = self.device
        n = len(contexts)
        if lora_names is not None:
            slots = self._lora_slots(lora_names, n)
        if n == 0:
            return np.zeros(0, np.float32), np.zeros(0, np.int32)
        if lora_names is not None:
            if any(len(c) == 0 for c in contexts):
                raise ValueError("Token ids must not be empty")
            mid_d = self._mask_ids_device(mask_ids, n)
            logits, group_of, U, row_mid, by_row = self._lora_rows_logits(contexts, slots, mid_d)
            return self._step_to_host(*self._finish_batch_step(logits, group_of, group_of, U, n, mid_d, row_mid, by_row))
        flat, starts, lens = ragged(contexts)
        if int(lens.min()) == 0:
            raise ValueError("Token ids must not be empty")
        mid_d = self._mask_ids_device(mask_ids, n)
        return self._step_to_host(*self._batch_step(torch.from_numpy(flat).to(dev), torch.from_numpy(starts).to(dev),
                                                    torch.from_numpy(lens).to(dev), n, mid_d, l_max=int(lens.max())))

    def _mask_ids_device(self, mask_ids, n):
        """The mask ids of a call's n contexts as an int32 device tensor (absent: mask 0); None when no masks are registered."""
        if self._mask_kind == MASK_NONE:
            return None
        mid = np.zeros(n, np.int32) if mask_ids is None else np.ascontiguousarray(mask_ids, dtype=np.int32)
        return torch.from_numpy(mid).to(self.device)

    @staticmethod
    def _row_mask_ids(mid_d, rep, group_of, n, head):
        """The mask id of every dedup group's representative (None without masks); `head`, the words of the call's D2H copy,
        gets one more: may the mask ids go per logits row? (they do when the mask is a function of the context)."""
        if mid_d is None:
            return None
        row_mid = mid_d[rep.long().clamp(0, n - 1)]  # entries of `rep` past the group count are unspecified
        head.append((row_mid[group_of.long()] == mid_d).all().to(torch.int32))
        return row_mid

    def _step_to_host(self, logZ, tok):
        """(logZ float32 [n], token int32 [n]) as NumPy arrays, in one D2H copy; raises if a step launch failed."""
        out = torch.stack([logZ, tok.to(torch.float32)]).cpu().numpy()  # token ids < 2^24: exact in float32
        toks = out[1].astype(np.int32)
        self.engine.raise_if_failed(tokens=toks)  # a finishing wave of the one-launch step gave up waiting (include/glb.h)
        return out[0], toks

    @torch.no_grad()
    def batch_next_token_step_device(self, tokens, lengths, mask_ids=None, constraint=None, prompt_lengths=None):
        """`batch_next_token_step` for a population that LIVES ON THE DEVICE: `tokens` int32 [n, cap] (row i's first
        lengths[i] entries are context i - the padded particle matrix a device-resident loop keeps), `lengths` int32 [n],
        `mask_ids` int32 [n] or None, all device tensors.  Returns (logZ float32 [n], token int32 [n]) as device tensors:
        nothing of the population crosses the host in either direction (the call's only D2H copy is the handful of counts
        the host needs to size the forward; a failed launch shows as token -2 and raises at the next call / `engine.check()`).
        No counterpart in the reference (its API takes Python lists, hf.py:346-373); this is the same evaluation.
        `constraint` (a `constraints.DeviceConstraint`, exclusive with `mask_ids`): context i's mask is that of the automaton
        state after tokens[i, prompt_lengths[i]:lengths[i]) (`prompt_lengths` int32 [n], None: zeros), recomputed here - the
        call keeps no state; the registered masks are not used.  Over a `constraints.ByteWFSA` the state's row of token
        log-weights is added to the log-probabilities (the bank handed over as float masks).  Under a constraint with
        pushed weights (`push="log"` / `"max"`) the rows are the pushed ones and so is the logZ returned: the call is
        stateless and adds no constant - a caller that accumulates weights starts them at `constraint.start_logw`."""
        if constraint is not None and mask_ids is not None:
            raise ValueError("give mask_ids (registered masks) or constraint (masks made on the device), not both")
        if tokens.dim() != 2 or tokens.dtype != torch.int32 or lengths.dtype != torch.int32 or lengths.numel() != tokens.shape[0]:
            raise ValueError("tokens must be int32 [n, cap] and lengths int32 [n]")
        if not tokens.is_contiguous():
            tokens = tokens.contiguous()
        n, cap = tokens.shape
        if n == 0:
            return (torch.zeros(0, dtype=torch.float32, device=self.device), torch.zeros(0, dtype=torch.int32, device=self.device))
        key = (n, cap)
        if getattr(self, "_row_starts", (None,))[0] != key:
            self._row_starts = (key, torch.arange(n, device=self.device, dtype=torch.int64) * cap)
        mid_d = None
        if constraint is not None:
            frm = torch.zeros_like(lengths) if prompt_lengths is None else prompt_lengths
            mid_d = constraint.mask_rows(constraint.advance(None, tokens, frm, lengths))
        elif self._mask_kind != MASK_NONE:
            mid_d = torch.zeros(n, dtype=torch.int32, device=self.device) if mask_ids is None else mask_ids
        return self._batch_step(tokens.view(-1), self._row_starts[1], lengths, n, mid_d, l_max=None, constraint=constraint)

    def _batch_step(self, tok_d, st_d, ln_d, n, mid_d, l_max, constraint=None, finish=None):
        """The batched step on a ragged batch that is on the device already.  l_max: the longest context if the host
        knows it (else it rides on the call's D2H copy).  Returns device tensors.  finish: what is made of the logits rows in
        place of the fused step (`_finish_batch_step`'s arguments: `_topk_finisher`)."""
        eng, dev = self.engine, self.device
        finish = finish or self._finish_batch_step
        self._lora_sync()
        group_of, rep, ng = eng.group_contexts(tok_d, st_d, ln_d)
        P = self._prefix_table()
        T = P["table"]
        base, pref, used_d = None, None, None
        head = [ng[0]]
        auto = self._auto_kv if (self._auto_kv is not None and not P["n"]) else None
        if P["n"]:
            pref, base = eng.match_prefixes(tok_d, st_d, ln_d, T.tokens, T.starts, T.lengths)
            head.append((ln_d - base).max().to(torch.int32))
            # which cached prefixes this call uses (they count as recently used, like walk_cache's touch)
            used_d = torch.zeros(P["n"] + 1, dtype=torch.int32, device=dev).index_fill_(0, (pref + 1).long(), 1)[1:]
        elif l_max is None and auto is None:
            head.append(ln_d.max().to(torch.int32))
        row_mid = self._row_mask_ids(mid_d, rep, group_of, n, head)
        if auto is not None:
            # contexts find the KV rows of their first L - 1 tokens (autokv.AutoKV): one token per context is fed; the error
            # word of the calls so far rides on the call's one D2H copy
            logits, row_of_group, group_of_row, U, extra = auto.logits(tok_d, st_d, ln_d, group_of, rep, ng,
                                                                       head[1:] + [eng.error_word()[0]])
            eng.raise_if_failed(extra[-1])
            by_row = bool(extra[-2]) if mid_d is not None else False
            if mid_d is not None:
                row_mid = row_mid[group_of_row]
            return finish(logits, row_of_group[group_of.long()], group_of, U, n, mid_d, row_mid, by_row, constraint)
        n_head = len(head)
        head = torch.stack(head) if used_d is None else torch.cat([torch.stack(head), used_d])
        head = head.cpu().tolist()  # the call's one D2H copy before the forward
        if used_d is not None:
            for node, u in zip(P["nodes"], head[n_head:]):
                if u:
                    self._kv_lru.touch(node)
            head = head[:n_head]
        U = head[0]
        l_max = head[1] if (P["n"] or l_max is None) else l_max
        by_row = bool(head[-1]) if mid_d is not None else False
        prefixes = (T, pref[rep[:U].long()].contiguous()) if P["n"] else None
        enc = encode_ragged(self, (tok_d, st_d, ln_d), rep, U, l_max, pad_id=self._pad_id, base=base, prefixes=prefixes)
        logits = self._lm_head(enc.last_rows())  # [U, V]
        return finish(logits, group_of, group_of, U, n, mid_d, row_mid, by_row, constraint)

    def _finish_batch_step(self, logits, row_of, group_of, U, n, mid_d, row_mid, by_row, constraint=None):
        """The fused step over a batch's logits rows (row_of: logits row of every context; group_of: its dedup group -
        the order parity-mode noise is dealt in).  Returns (logZ, token) device tensors."""
        # (under a constraint the ids are bank rows: the bank itself or the units' rows gathered out of it, DeviceConstraint.step_masks)
        logZ, tok = self._fused_step(logits, row_of, row_mid[:U].contiguous() if by_row else mid_d, by_row, n, group_of, constraint)
        self._count(n, U, U)
        return logZ, tok

    async def batch_next_token_step(self, contexts, mask_ids=None, lora_names=None):
        """Awaitable form of `batch_next_token_step_sync` (the evaluation itself blocks the loop, like
        `batch_evaluate_queries` does in the reference, hf.py:307-308)."""
        return self.batch_next_token_step_sync(contexts, mask_ids, lora_names=lora_names)

    # ---- the k most probable next tokens (glb_topk_rows: DESIGN.md §30) ------------------------------------------------------
    def _topk_finisher(self, k, scale):
        """`_batch_step`'s `finish` for the top-k calls: `topk_rows` on the distinct logits rows, under the constraint's mask
        rows, and a gather of the [U, k] results to the contexts.  Returns (token int32 [n, k], logp float32 [n, k])."""
        def finish(logits, row_of, group_of, U, n, mid_d, row_mid, by_row, constraint=None):
            rows, kw = logits[:U], {}
            if constraint is not None:
                if not by_row:  # contexts that share a logits row under different masks: a row per context
                    rows, row_mid, row_of = logits[row_of.long()], mid_d, None
                kw, _ = constraint.step_masks(rows, row_mid[:rows.shape[0]].contiguous(), True, n, parity=False)
            got = self.engine.topk_rows(rows, k, vocab=logits.shape[-1], logit_scale=scale, want=("logp",), **kw)
            self._count(n, U, U)
            if row_of is None:
                return got["token"], got["logp"]
            idx = row_of.long()
            return got["token"][idx], got["logp"][idx]

        return finish

    @staticmethod
    def _topk_scale(k, temperature):
        if not isinstance(k, int) or not 1 <= k <= 64:
            raise ValueError(f"k must be an integer in 1..64, got {k!r}")
        if not float(temperature) > 0.0:
            raise ValueError(f"temperature must be > 0, got {temperature!r}")
        return 1.0 / float(temperature)

    @torch.no_grad()
    def batch_next_token_topk_sync(self, token_ids_list, k, temperature=1.0):
        """The k most probable next tokens of every context and their log-probabilities under softmax(logits /
        temperature): (tokens int32 [n, k], logprobs float32 [n, k]) as device tensors, most probable first, equal
        log-probabilities by lower token id.  The pipeline of `batch_next_token_step_sync` - dedup, cached-prefix match,
        one forward - with `HipEngine.topk_rows` on the distinct rows: no [n, V] log-softmax is written."""
        scale = self._topk_scale(k, temperature)
        n = len(token_ids_list)
        if n == 0:
            return (torch.zeros((0, k), dtype=torch.int32, device=self.device), torch.zeros((0, k), dtype=torch.float32, device=self.device))
        flat, starts, lens = ragged(token_ids_list)
        if int(lens.min()) == 0:
            raise ValueError("Token ids must not be empty")
        dev = self.device
        return self._batch_step(torch.from_numpy(flat).to(dev), torch.from_numpy(starts).to(dev), torch.from_numpy(lens).to(dev), n,
                                None, l_max=int(lens.max()), finish=self._topk_finisher(k, scale))

    async def batch_next_token_topk(self, token_ids_list, k, temperature=1.0):
        """Awaitable form of `batch_next_token_topk_sync` (the evaluation itself blocks the loop)."""
        return self.batch_next_token_topk_sync(token_ids_list, k, temperature)

    @torch.no_grad()
    def batch_next_token_topk_device(self, tokens, lengths, k, constraint=None, prompt_lengths=None, *, temperature=1.0, mask_rows=None):
        """`batch_next_token_topk_sync` for contexts that live on the device: `tokens` int32 [n, cap], `lengths` int32 [n] as
        `batch_next_token_step_device` takes them.  `constraint`: context i's candidates are those its automaton state after
        tokens[i, prompt_lengths[i]:lengths[i]) allows, and `logprobs` is the model's log-probability of the token (over a
        `constraints.ByteWFSA`: plus the token's weight) - not renormalised: what a search adds up.  mask_rows: the
        constraint's bank rows of the contexts when the caller keeps the states itself (`DeviceBeam`); else recomputed here."""
        scale = self._topk_scale(k, temperature)
        if tokens.dim() != 2 or tokens.dtype != torch.int32 or lengths.dtype != torch.int32 or lengths.numel() != tokens.shape[0]:
            raise ValueError("tokens must be int32 [n, cap] and lengths int32 [n]")
        if mask_rows is not None and constraint is None:
            raise ValueError("mask_rows given without the constraint whose bank they index")
        if not tokens.is_contiguous():
            tokens = tokens.contiguous()
        n, cap = tokens.shape
        if n == 0:
            return (torch.zeros((0, k), dtype=torch.int32, device=self.device), torch.zeros((0, k), dtype=torch.float32, device=self.device))
        key = (n, cap)
        if getattr(self, "_row_starts", (None,))[0] != key:
            self._row_starts = (key, torch.arange(n, device=self.device, dtype=torch.int64) * cap)
        mid_d = mask_rows
        if constraint is not None and mid_d is None:
            frm = torch.zeros_like(lengths) if prompt_lengths is None else prompt_lengths
            mid_d = constraint.mask_rows(constraint.advance(None, tokens, frm, lengths))
        return self._batch_step(tokens.view(-1), self._row_starts[1], lengths, n, mid_d, l_max=None, constraint=constraint,
                                finish=self._topk_finisher(k, scale))

    # ---- one adapter per context in one forward (lora.RowLora, glb_lora_rows: DESIGN.md §15) --------------------------------
    def _lora_slots(self, lora_names, n):
        """The table slot of every context (-1: the base model) for a call's `lora_names`; ValueError for a wrong length,
        an unknown name, an active merged adapter (the shadow's weights are then not the base's) or too many adapters."""
        from .lora import MAX_ROW_SLOTS

        names = list(lora_names)
        if len(names) != n:
            raise ValueError(f"lora_names has {len(names)} entries for {n} contexts")
        if self._lora is not None:
            raise ValueError(f"lora_names cannot be used while the merged adapter {self.active_lora!r} is active: "
                             "call clear_lora() first")
        order = {name: i for i, name in enumerate(self._loras)}  # (`add_new_lora` order)
        for name in names:
            if name is not None and name not in order:
                raise ValueError(f"A LoRA adapter named '{name}' has not been loaded yet. Please call add_new_lora() first "
                                 "to load and name your LoRA adapters.")
        if len(order) > MAX_ROW_SLOTS:
            raise ValueError(f"{len(order)} adapters are loaded; a call with lora_names serves at most {MAX_ROW_SLOTS}")
        return np.fromiter((-1 if name is None else order[name] for name in names), np.int32, n)

    def _lora_rows_logits(self, contexts, slots, mid_d=None):
        """The last-position logits of `contexts` under their adapters (`slots`: int32 [n], -1 the base), in one forward on
        the re-encoding path: dedup on (adapter, context) - every context is grouped with a leading pseudo-token V + 1 + slot
        -, ragged-to-padded gather without it, the body and the head with every targeted module wrapped for this call
        (lora.RowLora).  Neither reads nor writes the output trie, the prefix KV or the auto-KV rows (keyed by tokens alone).
        Returns (logits [U, V'], group_of, U, row mask ids, mask ids go per row)."""
        from .lora import RowLora

        eng, dev = self.engine, self.device
        n = len(contexts)
        self._ensure_shadow()
        if self._row_lora is None:
            self._row_lora = RowLora(list(self._loras.values()), self._net, eng)
        vocab = int(self.model.config.vocab_size)
        flat, starts, lens = ragged([[vocab + 1 + int(s)] + list(c) for s, c in zip(slots, contexts)])
        tok_d, st_d, ln_d = (torch.from_numpy(a).to(dev) for a in (flat, starts, lens))
        slots_d = torch.from_numpy(slots).to(dev)
        group_of, rep, ng = eng.group_contexts(tok_d, st_d, ln_d)
        head = [ng[0]]
        row_mid = self._row_mask_ids(mid_d, rep, group_of, n, head)
        head = torch.stack(head).cpu().tolist()
        U = head[0]
        by_row = bool(head[-1]) if mid_d is not None else False
        seq_slots = slots_d[rep[:U].long()].contiguous()
        head_was, body_was = self._head, self._body
        with self._row_lora(seq_slots) as rl:
            try:
                self._head, self._body = self._net.get_output_embeddings(), self._net.base_model
                # (the gather leaves the pseudo-token out)
                enc = encode_ragged(self, (tok_d, st_d + 1, ln_d - 1), rep, U, int(lens.max()) - 1, pad_id=self._pad_id)
                logits = self._lm_head(enc.last_rows())  # [U, V]: per-sequence slots
            finally:
                self._head, self._body = head_was, body_was
            self.stats["lora_rows_calls"] += rl.calls
        return logits, group_of, U, row_mid, by_row

    @torch.no_grad()
    def _batch_lora_logprobs(self, token_ids_list, lora_names):
        n = len(token_ids_list)
        slots = self._lora_slots(lora_names, n)
        if any(len(c) == 0 for c in token_ids_list):
            raise ValueError("Token ids must not be empty")
        if n == 0:
            return torch.zeros((0, int(self.model.config.vocab_size)), device=self.device)
        logits, group_of, U, _, _ = self._lora_rows_logits(token_ids_list, slots)
        lp = self._log_softmax(logits)
        out = lp.index_select(0, group_of.long())
        self.engine.raise_if_failed(int(self.engine.error_word().item()), what="glb_log_softmax_rows")
        self._count(n, U, U)
        return out

    @torch.no_grad()
    def _batch_logprobs(self, token_ids_list):
        """`batch_next_token_logprobs` without one coroutine / future per context: cache walk per context, ONE batched
        evaluation of the misses, trie update, rows stacked on the device."""
        pending, refs = [], [None] * len(token_ids_list)  # refs[i]: (tensor, index) of context i's row (held: the budget may evict)
        for i, token_ids in enumerate(token_ids_list):
            if not token_ids:
                raise ValueError("Token ids must not be empty")
            node, nti, past, base = self.walk_cache(token_ids)
            if nti == len(token_ids):
                refs[i] = node.row_ref()
            else:
                pending.append((i, node, nti, base, Query(token_ids[base:], _Slot(reraise=True), past, first_new=nti - base)))
        if pending:
            self._evaluate([q for *_, q in pending])
            for i, node, nti, base, q in pending:
                slab, row0, first = q.future.value
                refs[i] = node.extend_cache_lazy(nti, token_ids_list[i], slab, base + first - row0, store=self._rows)
        # rows of one slab leave in one gather
        by_slab = {}
        for i, (t, idx) in enumerate(refs):
            ent = by_slab.get(id(t))
            if ent is None:
                ent = by_slab[id(t)] = (t, [], [])
            ent[1].append(i)
            ent[2].append(idx)
        dev = self.device
        out = None
        for t, pos, idx in by_slab.values():
            if idx[0] < 0:  # a row of its own
                got = t[None].expand(len(pos), -1)
            else:
                got = t.index_select(0, torch.from_numpy(np.asarray(idx, np.int64)).to(dev))
            if len(by_slab) == 1:
                return got  # positions 0 .. n-1 in order
            if out is None:
                out = torch.empty((len(refs), got.shape[-1]), dtype=got.dtype, device=dev)
            out[torch.from_numpy(np.asarray(pos, np.int64)).to(dev)] = got
        return out

    async def batch_next_token_logprobs(self, token_ids_list, lora_names=None):
        """base.py:47-60 (one batched evaluation instead of a gather over per-context coroutines).  lora_names: as
        `batch_next_token_step_sync`."""
        if lora_names is not None:
            return self._batch_lora_logprobs(token_ids_list, lora_names)
        return self._batch_logprobs(token_ids_list)

    def batch_next_token_logprobs_sync(self, token_ids_list, lora_names=None):
        """base.py:62-73.  lora_names: one entry per context - a name given to `add_new_lora`, or None for the base model;
        all contexts are evaluated in one forward, each under its adapter (unmerged: DESIGN.md §15).  Such a call leaves
        the output trie and the KV caches alone."""
        if lora_names is not None:
            return self._batch_lora_logprobs(token_ids_list, lora_names)
        return self._batch_logprobs(token_ids_list)

    # ---- scoring given sequences (glb_score_rows: DESIGN.md §29) -----------------------------------------------------------
    def batch_sequence_logprobs_sync(self, prompts, continuations, *, temperature=1.0, constraint=None):
        """log p(continuation token | prompt, earlier continuation tokens) for every token of every pair, in ONE forward over
        prompt + continuation[:-1] and without a log-softmax of any row: `SequenceScores`.  prompts, continuations: lists of
        token-id lists of equal count; a prompt needs at least one token, a continuation may be empty.  temperature: the
        scores are those of softmax(logits / temperature).  constraint (any constraint of `constraints`): the continuation
        is also walked through it from its start state - `SequenceScores`' logZ and masked fields."""
        prompts, continuations = [list(p) for p in prompts], [list(c) for c in continuations]
        if len(prompts) != len(continuations):
            raise ValueError(f"{len(prompts)} prompts for {len(continuations)} continuations")
        if any(len(p) == 0 for p in prompts):
            raise ValueError("a prompt needs at least one token: the first scored token needs a position before it")
        n = len(prompts)
        cap = max((len(p) + len(c) for p, c in zip(prompts, continuations)), default=1)
        tok = np.zeros((n, cap), np.int32)
        for i, (p, c) in enumerate(zip(prompts, continuations)):
            tok[i, :len(p) + len(c)] = p + c
        plen = np.fromiter(map(len, prompts), np.int32, n)
        lens = plen + np.fromiter(map(len, continuations), np.int32, n)
        dev = self.device
        return self.batch_sequence_logprobs_device(torch.from_numpy(tok).to(dev), torch.from_numpy(lens).to(dev),
                                                   torch.from_numpy(plen).to(dev), temperature=temperature, constraint=constraint)

    async def batch_sequence_logprobs(self, prompts, continuations, *, temperature=1.0, constraint=None):
        """Awaitable form of `batch_sequence_logprobs_sync` (the evaluation itself blocks the loop)."""
        return self.batch_sequence_logprobs_sync(prompts, continuations, temperature=temperature, constraint=constraint)

    async def sequence_logprobs(self, prompt, continuation, *, temperature=1.0, constraint=None):
        """`batch_sequence_logprobs` of one pair."""
        return self.batch_sequence_logprobs_sync([prompt], [continuation], temperature=temperature, constraint=constraint)

    @torch.no_grad()
    def batch_sequence_logprobs_device(self, tokens, lengths, prompt_lengths, *, temperature=1.0, constraint=None, forced_at=None):
        """`batch_sequence_logprobs_sync` for sequences that live on the device, as `batch_next_token_step_device` takes
        them: `tokens` int32 [N, cap] (row i's first lengths[i] entries: prompt, then continuation), `lengths` and
        `prompt_lengths` int32 [N].  No token and no score crosses the host, but the call is not asynchronous: it copies back
        six counts to size the forward and the score buffers (and, under a constraint, how many sequences have a token at each
        position), and each copy waits for the stream - a caller that queues work behind a population stalls here.
        forced_at (needs a constraint): int32 [N] device, the place in its continuation at which sequence i was MADE to end
        (negative: nowhere) - that token is scored against the row a finished sequence is served (EOS alone if its state
        accepts, else nothing), as a `DeviceSIS` particle out of tokens is."""
        if tokens.dim() != 2 or tokens.dtype != torch.int32 or lengths.dtype != torch.int32 or lengths.shape != (tokens.shape[0],):
            raise ValueError("tokens must be int32 [n, cap] and lengths int32 [n]")
        if prompt_lengths.dtype != torch.int32 or prompt_lengths.shape != lengths.shape:
            raise ValueError("prompt_lengths must be int32 [n]")
        if not 0 < temperature < float("inf"):
            raise ValueError(f"temperature must be positive and finite, got {temperature!r}")
        if forced_at is not None and (constraint is None or forced_at.dtype != torch.int32 or forced_at.shape != lengths.shape):
            raise ValueError("forced_at must be int32 [n] and needs a constraint")
        eng, dev = self.engine, self.device
        tokens = tokens.contiguous()
        N, cap = tokens.shape
        f32 = lambda k: torch.zeros(k, dtype=torch.float32, device=dev)
        if N == 0:
            return SequenceScores(torch.zeros(1, dtype=torch.int64, device=dev), f32(0), f32(0),
                                  *([f32(0)] * 4 if constraint is not None else []))
        self._lora_sync()
        P, T = prompt_lengths.long(), (lengths - prompt_lengths).long()
        starts = torch.zeros(N + 1, dtype=torch.int64, device=dev)
        torch.cumsum(T.clamp(min=0), 0, out=starts[1:])
        enc_len = (lengths - 1).clamp(min=1)  # prompt + continuation[:-1]; a lone prompt token stands for itself
        R, l_max, t_max, p_min, t_min, len_max = torch.stack([starts[-1], enc_len.max().long(), T.max(), P.min(), T.min(),
                                                              lengths.max().long()]).tolist()  # the call's D2H copy
        if p_min < 1:
            raise ValueError("a prompt needs at least one token: the first scored token needs a position before it")
        if t_min < 0 or len_max > cap:
            raise ValueError("prompt_lengths must not exceed lengths, nor lengths the width of tokens")
        names = ("logp",) if constraint is None else ("logp", "logZ", "logp_masked")
        tok_out = {w: torch.empty(R, dtype=torch.float32, device=dev) for w in names}
        if R:
            row_start = torch.arange(N, dtype=torch.int64, device=dev) * cap
            enc = encode_ragged(self, (tokens.view(-1), row_start, enc_len), torch.arange(N, dtype=torch.int32, device=dev), N,
                                l_max, pad_id=self._pad_id)
            hidden = enc.hidden.reshape(N * l_max, -1)  # (right-padded: position j of sequence i is row i * l_max + j)
            rows_per = self._score_rows_per_chunk(hidden)
            scale = 1.0 / temperature
            if constraint is None:
                seq = torch.repeat_interleave(torch.arange(N, device=dev), T, output_size=R)
                k = torch.arange(R, device=dev) - starts[seq]  # the token's place in its continuation
                h_idx, tgt = seq * l_max + P[seq] - 1 + k, tokens.view(-1)[seq * cap + P[seq] + k]
                for a in range(0, R, rows_per):  # (a chunk boundary may fall inside a sequence)
                    logits = self._lm_head(hidden[h_idx[a:a + rows_per]])
                    got = eng.score_rows(logits, tgt[a:a + rows_per].contiguous(), vocab=logits.shape[-1], logit_scale=scale,
                                         want=names)
                    tok_out["logp"][a:a + rows_per] = got["logp"]
            else:
                self._score_constrained(constraint, tokens, lengths, P, T, starts, hidden, l_max, t_max, rows_per, scale, tok_out,
                                        forced_at)
        sums = {w: eng.score_seq_sums(v, starts) for w, v in tok_out.items()}
        if constraint is None:
            return SequenceScores(starts, tok_out["logp"], sums["logp"])
        constraint.check()
        return SequenceScores(starts, tok_out["logp"], sums["logp"], tok_out["logZ"], sums["logZ"], tok_out["logp_masked"],
                              sums["logp_masked"])

    def _score_rows_per_chunk(self, hidden):
        """Logits rows a scoring chunk may hold: `score_chunk_bytes` over the bytes of a row as `_lm_head` returns it (the
        head's own width and dtype, found by running it on one row), a third of that where the head soft-caps its logits
        (x / cap and tanh(.) are temporaries of the logits' size)."""
        one = self._lm_head(hidden[:1])
        per_row = one.shape[-1] * one.element_size() * (3 if self._head_cap is not None else 1)
        return max(1, self.score_chunk_bytes // per_row)

    def _score_constrained(self, constraint, tokens, lengths, P, T, starts, hidden, l_max, t_max, rows_per, scale, tok_out,
                           forced_at=None):
        """Position by position: the sequences that have a token at position t are scored against the mask rows of their
        current states, then every state moves over its token.  Row ids are asked for afresh at each position (an evicting
        bank may recycle rows between two `mask_rows` calls)."""
        eng, dev = self.engine, self.device
        N, cap = tokens.shape
        order = torch.argsort(T, descending=True, stable=True)  # the sequences with a token at position t: a prefix of it
        counts = (T[:, None] > torch.arange(t_max, device=dev)[None]).sum(0).tolist()  # (D2H: t_max counts)
        states = constraint.states0(N)
        P32 = P.to(torch.int32)
        flat = tokens.view(-1)
        for t in range(t_max):
            done = T <= t
            if forced_at is not None:  # (a sequence made to end here: the row of a finished one)
                done = done | (forced_at == t)
            ids = constraint.mask_rows(states, done.to(torch.int32))
            for a in range(0, counts[t], rows_per):
                act = order[a:min(a + rows_per, counts[t])]
                logits = self._lm_head(hidden[act * l_max + P[act] - 1 + t])
                kw, _ = constraint.step_masks(logits, ids[act].contiguous(), True, act.numel())
                got = eng.score_rows(logits, flat[act * cap + P[act] + t].contiguous(), vocab=logits.shape[-1], logit_scale=scale,
                                     want=tuple(tok_out), **kw)
                for w, v in tok_out.items():
                    v[starts[act] + t] = got[w]
            frm = torch.minimum(P32 + t, lengths)
            states = constraint.advance(states, tokens, frm.contiguous(), torch.minimum(P32 + t + 1, lengths).contiguous())

    # ---- sampling (base.py:110-179): a device-resident multi-token loop -----------------------------------------------
    @torch.no_grad()
    def batch_sample_sync(self, prompt_token_ids_list, max_tokens, eos_token_ids, temperature=1.0, seed=None,
                          sync_every=4, top_k=0, top_p=1.0, min_p=0.0):
        """base.py:148-179.  All sequences advance together on the device (sis.DeviceSampler): per-sequence KV slabs,
        softmax(logits / temperature) -> one draw per sequence per forward by the fused step, stop on `eos_token_ids`.
        With a seed every sequence reproduces torch.multinomial under its own torch.Generator().manual_seed(seed)
        (base.py:125-141); without one the draws come from the in-kernel Philox stream.  `sync_every`: how often the
        loop reads the number of unfinished sequences back (the reference reads every token of every sequence).
        top_k (0: off), top_p (1: off), min_p (0: off): every step draws from the distribution truncated after the temperature
        - top-k, then the nucleus among those, and min-p against the largest probability, ties at the boundary kept
        (HipEngine.truncate_rows) - and renormalised; with a seed, torch.multinomial of exactly that."""
        from .engine import check_truncation
        from .sis import DeviceSampler

        check_truncation(top_k, top_p, min_p)
        if not prompt_token_ids_list:
            return []
        if any(len(p) == 0 for p in prompt_token_ids_list):
            raise ValueError("Token ids must not be empty")
        if max_tokens <= 0:
            return [[] for _ in prompt_token_ids_list]
        smp = DeviceSampler(self, prompt_token_ids_list, max_tokens, eos_token_ids, temperature, seed, sync_every=sync_every,
                            top_k=top_k, top_p=top_p, min_p=min_p)
        return [[int(t) for t in row] for row in smp.generate()]

    async def batch_sample(self, prompt_token_ids_list, max_tokens, eos_token_ids, temperature=1.0, seed=None, top_k=0, top_p=1.0,
                           min_p=0.0):
        """base.py:148-179; top_k, top_p, min_p as `batch_sample_sync` takes them"""
        return self.batch_sample_sync(prompt_token_ids_list, max_tokens, eos_token_ids, temperature, seed, top_k=top_k, top_p=top_p,
                                      min_p=min_p)

    async def sample(self, prompt_token_ids, max_tokens, eos_token_ids, temperature=1.0, seed=None, top_k=0, top_p=1.0, min_p=0.0):
        """base.py:110-146; top_k, top_p, min_p as `batch_sample_sync` takes them"""
        return self.batch_sample_sync([prompt_token_ids], max_tokens, eos_token_ids, temperature, seed, top_k=top_k, top_p=top_p,
                                      min_p=min_p)[0]


def load_model_by_name(name, backend=None, llm_opts=None):
    """llm/__init__.py:10-43.  `backend` may be None / "amd" / "hf" (all served by AsyncAmdLM on the
    MI355X); the CUDA / Apple engines of the reference ("vllm", "sgl", "mlx") do not exist here."""
    if llm_opts is None:
        llm_opts = {}
    if backend in (None, "amd", "hf"):
        return AsyncAmdLM.from_name(name, **llm_opts)
    if backend in ("vllm", "sgl", "mlx", "mock"):
        raise ValueError(f"Backend {backend!r} is not part of the MI355X hot-path build")
    raise ValueError(f"Invalid backend: {backend}")
