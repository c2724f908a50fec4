"""4-bit NF4 / FP4 weights (`bitsandbytes_opts={"load_in_4bit": True, ...}`), served by this library's kernels.

`bitsandbytes` itself is not needed: the block format is restated here (blocks of 64 along the input features, one float32
absmax and 64 four-bit codes into a 16-entry codebook each, no double quantisation) and everything hot about it is
glb_w4_quantize / glb_w4_dequantize / glb_w4_gemm (csrc/glb_quant.hip).

  * `parse_opts` builds `transformers.BitsAndBytesConfig(**opts)` as the reference does (hf.py:80-112) and turns it into a
    `W4Config`; what this backend does not serve raises NotImplementedError naming the option.
  * `quantize_model` replaces the `nn.Linear` / `Conv1D` modules of a model by `W4Linear`, one glb_w4_quantize launch each,
    and lets the full-precision weight go as it does.  The peak is still the full-precision model: loading shard by shard is
    out of scope.
  * `W4Linear.forward`: few rows go through glb_w4_gemm, which reads the 4-bit image directly; everything else dequantises the
    layer into a scratch buffer shared by all layers of the model and runs `torch.nn.functional.linear` on it.

The codebooks below are written from the published description of the format; equality with bitsandbytes' own tables has not
been checked against an installation of it.
"""
import numpy as np
import torch

BLOCK = 64

NF4 = (-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635, -0.18477343022823334,
       -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
       0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0)
_FP4_HALF = tuple(float(np.float32(v) / np.float32(12.0)) for v in (0.0, 0.0625, 8.0, 12.0, 4.0, 6.0, 2.0, 3.0))
FP4 = _FP4_HALF + tuple(-v for v in _FP4_HALF)  # bit 3 is the sign
CODEBOOKS = {"nf4": NF4, "fp4": FP4}

W4_GEMM_MODES = ("auto", "fused", "dequant")

# The fused kernel's dispatch rule: per (N, K) of a projection, the most rows (tokens of a forward) at which glb_w4_gemm
# runs under w4_gemm="auto", from the A/B of profiles/r09/w4_gemm_ab.txt (tools/w4_gemm_ab.py: fused kernel vs dequantise +
# F.linear in one process, alternating): the last measured M below which the fused kernel wins at every smaller M.  Shapes
# that were not measured, and larger batches, dequantise and run the library's GEMM.
MIN_ROWS_FUSED = {
    (2048, 2048): 128,   # Llama-3.2-1B q / o: 0.51-0.56x the time of (b) up to 64 rows, 0.85x at 128
    (512, 2048): 128,    # 1B k / v: 0.52-0.54x throughout
    (8192, 2048): 64,    # 1B gate / up: 0.50-0.60x up to 32, 0.88x at 64, 1.47x at 128
    (2048, 8192): 64,    # 1B down: 0.41-0.62x up to 32, 0.84x at 64, 1.34x at 128
    (4096, 4096): 64,    # Llama-3-8B q / o: 0.43-0.64x up to 32, 0.84x at 64, 1.22x at 128
    (1024, 4096): 128,   # 8B k / v: 0.50-0.64x up to 64, 0.89x at 128
    (14336, 4096): 64,   # 8B gate / up: 0.21-0.46x up to 32, 0.81x at 64, 1.53x at 128
    (4096, 14336): 64,   # 8B down: 0.24-0.44x up to 32, 0.64x at 64; 0.98x at 128 is inside the noise and left to (b)
}
min_rows_fused = MIN_ROWS_FUSED


def w4_bytes(n, k):
    """Bytes of the packed image of a [n, k] weight: codes + absmax."""
    return n * k // 2 + 4 * (n * k // BLOCK)


class W4Config:
    def __init__(self, quant_type, compute_dtype, skip_modules):
        self.quant_type = quant_type        # "nf4" | "fp4"
        self.compute_dtype = compute_dtype  # torch dtype, or None: the activations' own
        self.skip_modules = skip_modules    # module names left in full precision, or None: the output embedding

    def __repr__(self):
        return f"W4Config({self.quant_type}, compute_dtype={self.compute_dtype}, skip_modules={self.skip_modules})"


_DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16, "float32": torch.float32,
           "fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32, "half": torch.float16, "float": torch.float32}


def parse_opts(bitsandbytes_opts):
    """`bitsandbytes_opts` (the dict the reference hands to transformers.BitsAndBytesConfig) -> W4Config."""
    from transformers import BitsAndBytesConfig

    opts = dict(bitsandbytes_opts)
    cfg = BitsAndBytesConfig(**opts)
    if getattr(cfg, "load_in_8bit", False):
        raise NotImplementedError("bitsandbytes_opts: load_in_8bit (LLM.int8) is not served; use load_in_4bit")
    if not getattr(cfg, "load_in_4bit", False):
        raise NotImplementedError("bitsandbytes_opts: only load_in_4bit=True is served")
    if getattr(cfg, "bnb_4bit_use_double_quant", False):
        raise NotImplementedError("bitsandbytes_opts: bnb_4bit_use_double_quant=True is not served")
    storage = getattr(cfg, "bnb_4bit_quant_storage", torch.uint8)
    if storage not in (torch.uint8, "uint8"):
        raise NotImplementedError(f"bitsandbytes_opts: bnb_4bit_quant_storage {storage} is not served (uint8 only)")
    qt = cfg.bnb_4bit_quant_type
    if qt not in CODEBOOKS:
        raise NotImplementedError(f"bitsandbytes_opts: bnb_4bit_quant_type {qt!r} is not served (fp4 or nf4)")
    cd = None
    if opts.get("bnb_4bit_compute_dtype") is not None:  # (the config object reports float32 for "unset": look at the dict)
        cd = cfg.bnb_4bit_compute_dtype
        if isinstance(cd, str):
            cd = _DTYPES.get(cd.replace("torch.", ""))
        if cd not in (torch.float16, torch.bfloat16, torch.float32):
            raise NotImplementedError(f"bitsandbytes_opts: bnb_4bit_compute_dtype {opts['bnb_4bit_compute_dtype']!r} is not "
                                      "served (float16, bfloat16 or float32)")
    skip = cfg.llm_int8_skip_modules
    return W4Config(qt, cd, list(skip) if skip is not None else None)


class W4Scratch:
    """One dequantisation buffer for all W4Linear modules of a model, sized for the largest of them and allocated when the
    model is quantised (its address is stable under hipGraph capture).  One buffer per compute dtype that is used."""

    def __init__(self, device):
        self.device = device
        self.numel = 0
        self._bufs = {}

    def reserve(self, numel, dtype=None):
        self.numel = max(self.numel, numel)
        if dtype is not None:
            self.get(dtype)

    def get(self, dtype):
        buf = self._bufs.get(dtype)
        if buf is None or buf.numel() < self.numel:
            buf = self._bufs[dtype] = torch.empty(self.numel, dtype=dtype, device=self.device)
        return buf

    def nbytes(self):
        return sum(b.numel() * b.element_size() for b in self._bufs.values())


class W4Linear(torch.nn.Module):
    """y = x . W'^T + bias over a 4-bit image of W [out_features, in_features] (a quantised `Conv1D` is stored the same way:
    its transposed weight is read by glb_w4_quantize's `transposed` flag).  Inference only; there is no `.weight`."""

    def __init__(self, image, bias, in_features, out_features, quant_type, compute_dtype, engine, scratch):
        super().__init__()
        self.register_buffer("image", image)
        self.register_buffer("bias", bias)
        self.in_features, self.out_features = in_features, out_features
        self.quant_type, self.compute_dtype = quant_type, compute_dtype
        self.mode = "auto"
        self.__dict__["_glb_engine"] = engine  # (not submodules / buffers)
        self.__dict__["_glb_scratch"] = scratch

    @property
    def codebook(self):
        return CODEBOOKS[self.quant_type]

    def dequantize(self, dtype=torch.float32, out=None):
        """W' [out_features, in_features] in `dtype` (glb_w4_dequantize)."""
        return self._glb_engine.w4_dequantize(self.image, self.out_features, self.in_features, self.codebook, dtype=dtype,
                                              out=out)

    def _bias(self, dtype):
        b = self.bias
        return b if b is None or b.dtype == dtype else b.to(dtype)

    def forward(self, x):
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("W4Linear is inference only: run it under torch.no_grad() (4-bit weights have no gradient)")
        eng = self._glb_engine
        n, k = self.out_features, self.in_features
        cd = self.compute_dtype or x.dtype
        rows = x.shape[:-1].numel()
        with torch.no_grad():
            if (self.mode != "dequant" and cd in (torch.bfloat16, torch.float16) and x.device == eng.device
                    and (self.mode == "fused" or rows <= min_rows_fused.get((n, k), 0))):
                y = eng.w4_gemm(x if x.dtype == cd else x.to(cd), self.image, n, self.codebook, self._bias(cd))
                if y is not None:
                    return y if y.dtype == x.dtype else y.to(x.dtype)
            w = self._glb_scratch.get(cd)[:n * k].view(n, k)
            eng.w4_dequantize(self.image, n, k, self.codebook, out=w)
            y = torch.nn.functional.linear(x if x.dtype == cd else x.to(cd), w, self._bias(cd))
            return y if y.dtype == x.dtype else y.to(x.dtype)

    def extra_repr(self):
        return (f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, "
                f"{self.quant_type}, compute_dtype={self.compute_dtype}, w4_gemm={self.mode}")


def _skipped_by_name(name, skip):
    """A skip entry names a module, a path prefix or any run of path components (transformers matches substrings)."""
    return any(f".{s}." in f".{name}." for s in skip)


def quantize_model(model, cfg, engine):
    """Replace every `nn.Linear` / `Conv1D` of `model` whose input features are a multiple of 64 by a W4Linear (in place: only
    for a model this backend made itself).  Left alone, with the reason in the report: the output embedding and whatever
    is tied to it (or `cfg.skip_modules` when given), other input widths, weights off the engine's device.  Raises ValueError
    for a weight that is not finite.  Returns {"quant_type", "compute_dtype", "modules", "skipped", "bytes", "bytes_before"}."""
    head = model.get_output_embeddings() if hasattr(model, "get_output_embeddings") else None
    tied = set()
    if head is not None and getattr(head, "weight", None) is not None:
        tied.add(head.weight.data_ptr())
    scratch = W4Scratch(engine.device)
    report = {"quant_type": cfg.quant_type, "compute_dtype": cfg.compute_dtype, "modules": [], "skipped": {}, "bytes": 0,
              "bytes_before": 0}
    codebook = CODEBOOKS[cfg.quant_type]
    todo = []
    for pname, parent in model.named_modules():
        for cname, child in parent._modules.items():
            if child is None:
                continue
            conv = type(child).__name__ == "Conv1D" and hasattr(child, "nf")
            if not (isinstance(child, torch.nn.Linear) or conv):
                continue
            name = f"{pname}.{cname}" if pname else cname
            w = child.weight
            n, k = (w.shape[1], w.shape[0]) if conv else (w.shape[0], w.shape[1])
            if cfg.skip_modules is not None:
                if _skipped_by_name(name, cfg.skip_modules):
                    report["skipped"][name] = "llm_int8_skip_modules"
                    continue
            elif child is head or w.data_ptr() in tied:
                report["skipped"][name] = "output embedding (or tied to it)"
                continue
            if k % BLOCK != 0 or engine.w4_bytes(n, k) == 0:
                report["skipped"][name] = f"in_features {k} is not a multiple of {BLOCK}"
                continue
            if w.device != engine.device:
                report["skipped"][name] = f"weight on {w.device}, engine on {engine.device}"
                continue
            if w.dtype not in (torch.float32, torch.bfloat16, torch.float16):
                report["skipped"][name] = f"weight dtype {w.dtype}"
                continue
            todo.append((name, parent, cname, child, conv, n, k))
    todo.reverse()
    while todo:  # (popped as it goes: nothing but `parent` holds a replaced module afterwards)
        name, parent, cname, child, conv, n, k = todo.pop()
        w = child.weight.detach()
        if not bool(torch.isfinite(w).all()):
            raise ValueError(f"quantize_model: {name} has weights that are not finite")
        if w.stride(-1) != 1:
            w = w.contiguous()
        with torch.no_grad():
            image = engine.w4_quantize(w, codebook, transposed=conv)
        bias = child.bias.detach() if getattr(child, "bias", None) is not None else None
        cd = cfg.compute_dtype
        q = W4Linear(image, bias, k, n, cfg.quant_type, cd, engine, scratch)
        q.train(child.training)
        report["bytes_before"] += w.numel() * w.element_size()
        report["bytes"] += image.numel()
        report["modules"].append(name)
        scratch.reserve(n * k, cd if cd is not None else w.dtype)
        parent._modules[cname] = q  # (the full-precision weight goes with the last reference to `child`)
        del child, w
    report["scratch_bytes"] = scratch.nbytes()
    model.__dict__["_glb_quantization"] = report
    return report


def bind(net, engine, mode):
    """Point the W4Linear modules of a backend's module tree at its engine and GEMM path (`w4_gemm`)."""
    if mode not in W4_GEMM_MODES:
        raise ValueError(f"w4_gemm must be one of {W4_GEMM_MODES}, got {mode!r}")
    found = 0
    for mod in net.modules():
        if isinstance(mod, W4Linear):
            mod.mode = mode
            if mod.__dict__.get("_glb_engine") is None or mod._glb_engine.device == engine.device:
                mod.__dict__["_glb_engine"] = engine
            found += 1
    return found
