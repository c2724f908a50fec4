"""LoRA adapters in peft's on-disk format, served by MERGING.

The reference loads an adapter with transformers' `load_adapter` and runs peft's unmerged form: two extra skinny GEMMs and
an add per targeted projection on every forward (hf.py:166-200).  This backend instead gives every targeted module of its
private shadow (fuse.shadow_model) a private weight W + s * B . A, made by ONE glb_lora_merge call per adapter switch; the
forward then runs exactly the kernels (and the tuned shapes) of the base model.

  * `load_adapter` reads adapter_config.json and adapter_model.safetensors (or adapter_model.bin) without peft, checks every
    (lora_A, lora_B) pair against the caller's module and its weight's shape, and keeps A and B on the model's device in
    their stored dtype.  What merging cannot serve is rejected with a ValueError: DoRA, trained biases, modules_to_save,
    embedding adapters, other peft types, keys without a module, shape mismatches, ranks above 256.
  * `MergedLora` installs an adapter in a shadow: each targeted shadow module gets a NEW `_parameters` dict (the merged
    weight plus the caller's other parameters).  Shadow modules share their `_parameters` dict with the caller's module,
    so the shared dict is never written; `uninstall` puts the shared dicts back and lets the merged tensors go.  `sync`
    re-merges the modules whose base weight changed since the merge (`Tensor._version`, identity, address).
  * `RowLora` serves SEVERAL adapters in one forward, one per context, UNMERGED: every loaded adapter is a
    slot of a device table, and for the duration of one call each targeted shadow module is wrapped by a `RowLoraModule`
    that runs the base module and then glb_lora_rows on its output with the call's row slots.  It reads only a module's
    input and output, so the base may be a 4-bit `W4Linear`.
"""
import json
import math
import os
import re

import numpy as np
import torch

MAX_RANK = 256  # glb_lora_merge and glb_lora_rows serve r = 1 .. 256
MAX_ROW_SLOTS = 64  # adapters that may be loaded when a call names adapters per context (glb_lora_rows' table)
_KEY = re.compile(r"^(?:base_model\.model\.)?(?P<path>.+)\.(?P<which>lora_A|lora_B)(?:\.(?P<name>[^.]+))?\.weight$")
_SERVED = (torch.float32, torch.bfloat16, torch.float16)


def _pattern_value(patterns, path, default):
    """peft's rank_pattern / alpha_pattern lookup: the first key that matches the end of the module path
    (`(.*\\.)?key$`, peft tuners_utils)."""
    for key, val in (patterns or {}).items():
        if re.match(rf"(.*\.)?{key}$", path):
            return val
    return default


def _module_kind(mod):
    if isinstance(mod, torch.nn.Linear):
        return "linear"
    if type(mod).__name__ in ("Conv1D", "SplitConv1D") and hasattr(mod, "nf"):
        return "conv1d"
    if type(mod).__name__ == "W4Linear":
        return "w4"  # (quant.py: loadable and checked for shape, but `set_lora` cannot merge into 4-bit codes)
    return None


def resolve_path(lora_path):
    """A local adapter directory as it is; anything else is a Hugging Face hub id, resolved through the hub cache the way
    `from_name` resolves model ids."""
    if os.path.isdir(lora_path):
        return lora_path
    from huggingface_hub import snapshot_download

    return snapshot_download(lora_path, allow_patterns=["adapter_config.json", "adapter_model.*"])


def _read_weights(path):
    st = os.path.join(path, "adapter_model.safetensors")
    if os.path.exists(st):
        from safetensors.torch import load_file

        return load_file(st)
    bn = os.path.join(path, "adapter_model.bin")
    if os.path.exists(bn):
        return torch.load(bn, map_location="cpu", weights_only=True)
    raise ValueError(f"no adapter_model.safetensors or adapter_model.bin in {path}")


class LoraModule:
    """One targeted module: `a` = lora_A [r, k_in], `b` = lora_B [n_out, r] (device, stored dtype), `scale` (float32 value),
    `transposed` (GPT-2 Conv1D: the weight is [k_in, n_out])."""

    def __init__(self, path, a, b, scale, transposed):
        self.path, self.a, self.b, self.scale, self.transposed = path, a, b, scale, transposed

    @property
    def rank(self):
        return self.a.shape[0]


class LoraAdapter:
    def __init__(self, name, path, config, modules):
        self.name, self.path, self.config, self.modules = name, path, config, modules

    def nbytes(self):
        return sum(m.a.numel() * m.a.element_size() + m.b.numel() * m.b.element_size() for m in self.modules.values())


def load_adapter(lora_path, model, name):
    """Read and validate a peft LoRA adapter against the caller's `model` (module paths are the paths inside it)."""
    path = resolve_path(lora_path)
    cfg_file = os.path.join(path, "adapter_config.json")
    if not os.path.exists(cfg_file):
        raise ValueError(f"no adapter_config.json in {path}")
    with open(cfg_file) as f:
        cfg = json.load(f)
    if cfg.get("peft_type") != "LORA":
        raise ValueError(f"adapter {path}: peft_type {cfg.get('peft_type')!r} is not LORA")
    if cfg.get("use_dora"):
        raise ValueError(f"adapter {path}: DoRA (use_dora) is not supported")
    if cfg.get("bias", "none") != "none":
        raise ValueError(f"adapter {path}: bias {cfg.get('bias')!r} is not supported (only 'none')")
    if cfg.get("modules_to_save"):
        raise ValueError(f"adapter {path}: modules_to_save {cfg['modules_to_save']} is not supported")
    r0, alpha0 = int(cfg.get("r", 8)), float(cfg.get("lora_alpha", 8))
    rslora = bool(cfg.get("use_rslora", False))
    rank_pattern, alpha_pattern = cfg.get("rank_pattern") or {}, cfg.get("alpha_pattern") or {}

    pairs = {}
    for key, t in _read_weights(path).items():
        if "lora_embedding_A" in key or "lora_embedding_B" in key:
            raise ValueError(f"adapter {path}: embedding LoRA ({key}) is not supported")
        m = _KEY.match(key)
        if m is None:
            raise ValueError(f"adapter {path}: key {key!r} is not a lora_A / lora_B weight")
        pairs.setdefault(m.group("path"), {})[m.group("which")] = t
    if not pairs:
        raise ValueError(f"adapter {path}: no lora_A / lora_B weights")

    device = next(model.parameters()).device
    modules = {}
    for mpath, ab in sorted(pairs.items()):
        if set(ab) != {"lora_A", "lora_B"}:
            raise ValueError(f"adapter {path}: module {mpath} has {sorted(ab)} only")
        try:
            mod = model.get_submodule(mpath)
        except AttributeError:
            raise ValueError(f"adapter {path}: key for {mpath!r}, which is no module of {type(model).__name__}") from None
        kind = _module_kind(mod)
        if kind is None:
            raise ValueError(f"adapter {path}: {mpath} is a {type(mod).__name__}, not nn.Linear or Conv1D")
        if kind == "w4":
            k_in, n_out = mod.in_features, mod.out_features
            w = torch.empty((n_out, k_in), device="meta")  # (for the messages below: a 4-bit module has no weight)
        else:
            w = mod.weight
            k_in, n_out = (w.shape[0], w.shape[1]) if kind == "conv1d" else (w.shape[1], w.shape[0])
        a, b = ab["lora_A"], ab["lora_B"]
        r = int(_pattern_value(rank_pattern, mpath, r0))
        alpha = float(_pattern_value(alpha_pattern, mpath, alpha0))
        if a.dim() != 2 or b.dim() != 2 or tuple(a.shape) != (a.shape[0], k_in) or tuple(b.shape) != (n_out, a.shape[0]):
            raise ValueError(f"adapter {path}: {mpath} lora_A {tuple(a.shape)} / lora_B {tuple(b.shape)} do not fit the weight "
                             f"{tuple(w.shape)} (k_in {k_in}, n_out {n_out})")
        if a.shape[0] != r:
            raise ValueError(f"adapter {path}: {mpath} has rank {a.shape[0]}, the config says {r}")
        if r > MAX_RANK:
            raise ValueError(f"adapter {path}: {mpath} has rank {r} > {MAX_RANK}")
        scale = alpha / math.sqrt(r) if rslora else alpha / r  # (double, rounded to float once)
        dt = a.dtype if a.dtype in _SERVED and b.dtype == a.dtype else torch.float32
        modules[mpath] = LoraModule(mpath, a.to(device, dt).contiguous(), b.to(device, dt).contiguous(),
                                    float(np.float32(scale)), kind == "conv1d")
    info = {k: cfg.get(k) for k in ("r", "lora_alpha", "target_modules", "fan_in_fan_out", "use_rslora", "rank_pattern",
                                     "alpha_pattern")}
    return LoraAdapter(name, path, info, modules)


def _base_key(t):
    return (id(t), t._version, t.data_ptr())


class MergedLora:
    """An adapter installed in a shadow module tree `net`: merged private weights on the targeted modules."""

    def __init__(self, adapter, net, engine):
        self.adapter, self.net, self.engine = adapter, net, engine
        self.slots = {}  # path -> [module, shared dict, private dict, base key]
        quantised = [p for p in adapter.modules if type(net.get_submodule(p)).__name__ == "W4Linear"]
        if quantised:
            raise ValueError(f"adapter {adapter.name}: {quantised[0]} (and {len(quantised) - 1} more) are 4-bit quantised "
                             "modules (W4Linear); LoRA is served by merging into the weight, which a quantised base does not "
                             "allow - load the model without bitsandbytes_opts")
        for p in adapter.modules:
            mod = net.get_submodule(p)
            self.slots[p] = [mod, mod._parameters, None, None]
        self._merge(list(adapter.modules))

    def _merge(self, paths):
        jobs = []
        for p in paths:
            lm = self.adapter.modules[p]
            mod, shared = self.slots[p][0], self.slots[p][1]
            base = shared["weight"]
            w = base.detach()
            if w.stride(-1) != 1:
                w = w.contiguous()
            out = torch.empty(w.shape, dtype=w.dtype, device=w.device)
            jobs.append(dict(w=w, a=lm.a, b=lm.b, scale=lm.scale, transposed=lm.transposed, out=out))
            private = type(shared)(shared)
            private["weight"] = torch.nn.Parameter(out, requires_grad=False)
            self.slots[p][2:] = [private, _base_key(base)]
        with torch.no_grad():
            self.engine.lora_merge(jobs)
        for p in paths:
            mod, _, private, _ = self.slots[p]
            mod.__dict__["_parameters"] = private

    def sync(self):
        """Re-merge the modules whose base weight was replaced or changed in place since their merge; the other entries
        of a private dict follow the shared one (a replaced bias).  Returns True if anything was re-merged."""
        stale = []
        for p, (mod, shared, private, key) in self.slots.items():
            if _base_key(shared["weight"]) != key:
                stale.append(p)
            for k, v in shared.items():
                if k != "weight" and private.get(k) is not v:
                    private[k] = v
        if stale:
            self._merge(stale)
        return bool(stale)

    def uninstall(self):
        for mod, shared, _, _ in self.slots.values():
            mod.__dict__["_parameters"] = shared
        self.slots = {}

    def nbytes(self):
        return sum(s[2]["weight"].numel() * s[2]["weight"].element_size() for s in self.slots.values())


class RowLoraModule(torch.nn.Module):
    """A targeted shadow module for the duration of one call that names adapters per context: the base module's output plus,
    per row, its adapter's s (x A^T) B^T (HipEngine.lora_rows, in place).  Everything else about the module (`weight`,
    `out_features`, `nf`, ...) is the base module's."""

    def __init__(self, base, owner, index):
        super().__init__()
        self.__dict__["_glb_base"] = base  # (not a submodule: the shadow's parameter walk must not see it twice)
        self.__dict__["_glb_owner"] = owner
        self.__dict__["_glb_index"] = index

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            return getattr(self.__dict__["_glb_base"], name)

    def add_delta(self, x, y):
        """y (this module's output for input x, or the column slice of a joint GEMM's output that is) += the rows' deltas."""
        return self._glb_owner.apply(self._glb_index, x, y)

    def forward(self, x, act=None):
        y = self._glb_base(x)  # (a SplitConv1D runs without its GELU epilogue: the activation follows the delta)
        self.add_delta(x, y)
        return y if act is None else act(y)


class RowLora:
    """The loaded adapters as slots (in `add_new_lora` order) over the shadow `net`: the device table of glb_lora_rows and
    the per-call wrappers."""

    def __init__(self, adapters, net, engine):
        if len(adapters) > MAX_ROW_SLOTS:
            raise ValueError(f"{len(adapters)} adapters are loaded; a call with lora_names serves at most {MAX_ROW_SLOTS}")
        self.net, self.engine = net, engine
        self.slot_of = {ad.name: i for i, ad in enumerate(adapters)}
        self.paths = sorted({p for ad in adapters for p in ad.modules})
        self.index_of = {p: i for i, p in enumerate(self.paths)}
        slots = []
        for ad in adapters:
            row = []
            for p in self.paths:
                lm = ad.modules.get(p)
                row.append(None if lm is None else dict(a=lm.a, b=lm.b, scale=lm.scale))
            slots.append(row)
        self.table = engine.lora_rows_table(slots) if self.paths else None
        self._seq = None      # int32 [U] device: the slot of every sequence of the running call
        self._by_rows = {}    # rows of a module's input -> its row slots
        self.calls = 0        # lora_rows launches of the running call

    def apply(self, index, x, y):
        seq = self._seq
        if seq is None:
            raise RuntimeError("RowLoraModule outside a call with lora_names")
        k = x.shape[-1]
        rows = x.numel() // k
        slots = self._by_rows.get(rows)
        if slots is None:
            u = seq.numel()
            if rows % u:
                raise RuntimeError(f"a targeted module saw {rows} rows for {u} sequences")
            # body modules see [U, L] tokens: a sequence's slot for each of its L positions
            slots = self._by_rows[rows] = seq.repeat_interleave(rows // u).contiguous()
        self.engine.lora_rows(x, y, slots, self.table, index)
        self.calls += 1
        return y

    def __call__(self, seq_slots):
        return _RowLoraCall(self, seq_slots)


class _RowLoraCall:
    """Context of one call: wrappers installed on entry and gone on exit (base results stay bit-identical)."""

    def __init__(self, owner, seq_slots):
        self.owner, self.seq = owner, seq_slots
        self.saved = []

    def __enter__(self):
        o = self.owner
        o._seq, o._by_rows, o.calls = self.seq.to(torch.int32).contiguous(), {}, 0
        o._by_rows[o._seq.numel()] = o._seq
        for p, i in o.index_of.items():
            parent_path, _, name = p.rpartition(".")
            parent = o.net.get_submodule(parent_path) if parent_path else o.net
            base = parent._modules[name]
            self.saved.append((parent, name, base))
            parent._modules[name] = RowLoraModule(base, o, i)
        return o

    def __exit__(self, *exc):
        for parent, name, base in self.saved:
            parent._modules[name] = base
        self.saved = []
        self.owner._seq, self.owner._by_rows = None, {}
        return False
