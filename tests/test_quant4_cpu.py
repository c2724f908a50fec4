"""4-bit NF4 / FP4 weights without a GPU: the codebooks, the format's three properties on the restatement
(tests/quant4_engine.py), `parse_opts`, the C ABI's argument checks, and the structure `quantize_model` / `W4Linear` give a
tiny Llama and a tiny GPT-2 (the HIP engine replaced by the restatement)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import quant4_engine as Q
from tests.cpu_engine import CpuOracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 96
HALF_GAP = {"nf4": 0.1519, "fp4": 0.1667}  # half the widest codebook gap (issue §1), as a fraction of absmax


class Engine(Q.StubW4Engine, CpuOracleEngine):
    pass


class Tok:
    pad_token_id = None
    eos_token_id = 0


def _llama(tie=True):
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(12)
    return LlamaForCausalLM(LlamaConfig(vocab_size=V, hidden_size=64, intermediate_size=128, num_hidden_layers=2,
                                        num_attention_heads=4, num_key_value_heads=2, head_dim=16, max_position_embeddings=64,
                                        bos_token_id=1, eos_token_id=2, tie_word_embeddings=tie)).eval()


def _gpt2():
    from transformers import GPT2Config, GPT2LMHeadModel

    torch.manual_seed(11)
    return GPT2LMHeadModel(GPT2Config(vocab_size=V, n_embd=64, n_layer=2, n_head=4, n_positions=64)).eval()


LLAMA_LINEARS = [f"model.layers.{i}.{m}" for i in range(2) for m in (
    "self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
    "mlp.down_proj")]
GPT2_LINEARS = [f"transformer.h.{i}.{m}" for i in range(2) for m in ("attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj")]


# ---- the tables ------------------------------------------------------------------------------------------------------------
def test_codebooks():
    from genlm_backend_amd import quant

    for name in ("nf4", "fp4"):
        cb = quant.CODEBOOKS[name]
        assert len(cb) == 16
        assert all(float(np.float32(v)) == v for v in cb), name  # float32-exact
        assert np.array_equal(np.array(cb, np.float64), Q.TABLES[name])  # the product's table is the restatement's
    nf4 = quant.CODEBOOKS["nf4"]
    assert list(nf4) == sorted(nf4) and len(set(nf4)) == 16
    assert 0.0 in nf4 and nf4[0] == -1.0 and nf4[-1] == 1.0
    fp4 = quant.CODEBOOKS["fp4"]
    assert [-v for v in fp4[:8]] == list(fp4[8:])
    want = (np.array([0, 0.0625, 8, 12, 4, 6, 2, 3], np.float32) / np.float32(12)).astype(np.float32)
    assert np.array_equal(np.array(fp4[:8], np.float32), want)
    assert max(abs(v) for v in fp4) == 1.0


# ---- the three properties of the format ------------------------------------------------------------------------------------
def _blocks(seed, n_blocks):
    rng = np.random.default_rng(seed)
    scale = np.exp(rng.uniform(-8, 8, (n_blocks, 1))).astype(np.float32)
    return (rng.standard_normal((n_blocks, 64)).astype(np.float32) * scale).astype(np.float32)


@pytest.mark.parametrize("name", ["nf4", "fp4"])
def test_roundtrip_properties(name):
    cb = Q.codebook(name)
    w = _blocks(5, 4096)
    w[7] = 0.0  # an all-zero block
    w[9] = 0.0
    w[9, 13] = -3.25  # a block with one non-zero element
    codes, absmax = Q.quantize(w, cb)
    deq = Q.dequantize_f32(codes, absmax, cb)
    assert np.isfinite(deq).all()
    assert np.array_equal(absmax[:, 0], np.abs(w).max(-1))
    # per element: within half the widest gap of the codebook, times absmax
    assert (np.abs(deq - w) <= HALF_GAP[name] * absmax).all()
    # quantise -> dequantise -> quantise: absmax survives, the dequantised VALUES are a fixed point
    codes2, absmax2 = Q.quantize(deq, cb)
    assert np.array_equal(absmax2, absmax)
    deq2 = Q.dequantize_f32(codes2, absmax2, cb)
    assert np.array_equal(deq2.view(np.uint32) & 0x7fffffff, deq.view(np.uint32) & 0x7fffffff)  # (+0 / -0 in FP4)
    assert np.array_equal(deq2, deq)
    if name == "nf4":
        assert np.array_equal(codes2, codes)
    else:  # codes too, except the two zeros
        differ = codes2 != codes
        assert (cb[codes[differ]] == 0).all() and (cb[codes2[differ]] == 0).all()
    # the zero block: absmax 0, zeros out, no NaN; the one-element block: that element exactly, zeros elsewhere
    assert absmax[7, 0] == 0 and (deq[7] == 0).all()
    assert deq[9, 13] == np.float32(-3.25) and (np.delete(deq[9], 13) == 0).all()


def test_code_is_the_nearest_entry():
    """The midpoint rule picks a nearest codebook entry (checked in float64 against brute force, ties aside)."""
    for name in ("nf4", "fp4"):
        cb = Q.codebook(name)
        w = _blocks(6, 256)
        codes, absmax = Q.quantize(w, cb)
        x = w.astype(np.float64) / absmax.astype(np.float64)
        dist = np.abs(x[..., None] - cb.astype(np.float64)[None, None, :])
        got = np.take_along_axis(dist, codes[..., None].astype(np.int64), -1)[..., 0]
        assert (got <= dist.min(-1) + 1e-6).all()


# ---- parse_opts ------------------------------------------------------------------------------------------------------------
def test_parse_opts_served():
    from genlm_backend_amd.quant import parse_opts

    c = parse_opts({"load_in_4bit": True})
    assert (c.quant_type, c.compute_dtype, c.skip_modules) == ("fp4", None, None)  # unset compute dtype: the activations'
    for qt in ("fp4", "nf4"):
        for cd in (torch.float16, torch.bfloat16, torch.float32):
            c = parse_opts({"load_in_4bit": True, "bnb_4bit_quant_type": qt, "bnb_4bit_compute_dtype": cd})
            assert (c.quant_type, c.compute_dtype) == (qt, cd)
    assert parse_opts({"load_in_4bit": True, "bnb_4bit_compute_dtype": "bfloat16"}).compute_dtype == torch.bfloat16
    c = parse_opts({"load_in_4bit": True, "llm_int8_skip_modules": ["lm_head", "q_proj"]})
    assert c.skip_modules == ["lm_head", "q_proj"]
    assert parse_opts({"load_in_4bit": True, "bnb_4bit_use_double_quant": False,
                       "bnb_4bit_quant_storage": torch.uint8}).quant_type == "fp4"


@pytest.mark.parametrize("opts, word", [
    ({"load_in_8bit": True}, "load_in_8bit"),
    ({"load_in_4bit": True, "bnb_4bit_use_double_quant": True}, "bnb_4bit_use_double_quant"),
    ({"load_in_4bit": True, "bnb_4bit_quant_storage": torch.bfloat16}, "bnb_4bit_quant_storage"),
    ({"load_in_4bit": True, "bnb_4bit_quant_storage": "float16"}, "bnb_4bit_quant_storage"),
])
def test_parse_opts_rejected(opts, word):
    from genlm_backend_amd.quant import parse_opts

    with pytest.raises(NotImplementedError, match=word):
        parse_opts(opts)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_abi_symbols_bytes_and_argument_errors():
    from genlm_backend_amd import _lib

    lib = _lib.load()
    for name in ("glb_w4_bytes", "glb_w4_quantize", "glb_w4_dequantize", "glb_w4_gemm", "glb_w4_gemm_workspace_bytes",
                 "glb_w4_gemm_max_rows"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    for n, k in [(2048, 2048), (512, 2048), (8192, 2048), (2048, 8192), (2304, 768), (768, 3072), (1, 64), (17, 64), (3, 192)]:
        assert lib.glb_w4_bytes(n, k) == n * k // 2 + 4 * (n * k // 64)
    for n, k in [(16, 32), (16, 65), (16, 100), (0, 64), (16, 0), (-1, 64)]:
        assert lib.glb_w4_bytes(n, k) == 0
    assert 1 <= lib.glb_w4_gemm_max_rows() <= 128 and lib.glb_w4_gemm_max_rows() % 16 == 0
    mx = lib.glb_w4_gemm_max_rows()
    assert lib.glb_w4_gemm_workspace_bytes(mx, 2048, 2048) > 0
    assert lib.glb_w4_gemm_workspace_bytes(mx + 1, 2048, 2048) == 0
    assert lib.glb_w4_gemm_workspace_bytes(1, 2040, 2048) == 0

    cb = (C.c_float * 16)(*Q.codebook("nf4"))
    buf = (C.c_char * 4096)()  # never dereferenced: every call below fails its argument check first
    ptr = C.addressof(buf) + (-C.addressof(buf)) % 16
    for fn in (lib.glb_w4_quantize, lib.glb_w4_dequantize):
        assert fn(None, None) == _lib.GLB_EINVAL
        a = _lib.W4Args()
        a.struct_size = 1
        assert fn(C.byref(a), None) == _lib.GLB_EINVAL and "struct_size" in _lib.last_error()
        a.struct_size = C.sizeof(_lib.W4Args)
        a.n, a.k, a.ldw = 16, 64, 64
        assert fn(C.byref(a), None) == _lib.GLB_EINVAL  # null pointers
        a.w, a.image, a.image_bytes, a.codebook = ptr, ptr + 2048, 16 * 32 + 64, cb
        a.dtype = 7
        assert fn(C.byref(a), None) == _lib.GLB_EINVAL and "dtype" in _lib.last_error()
        a.dtype, a.transposed = _lib.F32, 2
        assert fn(C.byref(a), None) == _lib.GLB_EINVAL
        a.transposed, a.ldw = 0, 63
        assert fn(C.byref(a), None) == _lib.GLB_EINVAL  # row pitch below the row
        a.ldw, a.k = 100, 100
        assert fn(C.byref(a), None) == _lib.GLB_EUNSUPPORTED  # k % 64 != 0
        a.k, a.image_bytes = 64, 16
        assert fn(C.byref(a), None) == _lib.GLB_ENOSPC
    assert lib.glb_w4_gemm(None, None) == _lib.GLB_EINVAL
    g = _lib.W4GemmArgs()
    g.struct_size = 3
    assert lib.glb_w4_gemm(C.byref(g), None) == _lib.GLB_EINVAL and "struct_size" in _lib.last_error()
    g.struct_size = C.sizeof(_lib.W4GemmArgs)
    g.m, g.n, g.k, g.ldx, g.ldy = 1, 16, 64, 64, 16
    g.dtype = _lib.F32
    assert lib.glb_w4_gemm(C.byref(g), None) == _lib.GLB_EINVAL and "dtype" in _lib.last_error()
    g.dtype = _lib.BF16
    assert lib.glb_w4_gemm(C.byref(g), None) == _lib.GLB_EINVAL  # null pointers
    g.x, g.image, g.y, g.workspace, g.workspace_bytes, g.codebook = ptr, ptr + 1024, ptr + 2048, ptr + 3072, 1024, cb
    g.ldx = 32
    assert lib.glb_w4_gemm(C.byref(g), None) == _lib.GLB_EINVAL  # row pitch below the row
    g.ldx, g.m = 64, mx + 1
    assert lib.glb_w4_gemm(C.byref(g), None) == _lib.GLB_EUNSUPPORTED
    g.m, g.n, g.ldy = 1, 24, 24
    assert lib.glb_w4_gemm(C.byref(g), None) == _lib.GLB_EUNSUPPORTED  # n % 16 != 0


def test_argument_blocks_have_the_headers_size(tmp_path):
    from genlm_backend_amd import _lib

    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "glb.h"\nint main(void) { printf("%zu %zu\\n", sizeof(glb_w4_args), '
                   'sizeof(glb_w4_gemm_args)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = tuple(int(v) for v in subprocess.check_output([str(exe)]).split())
    assert got == (C.sizeof(_lib.W4Args), C.sizeof(_lib.W4GemmArgs)) == (72, 104)


# ---- quantize_model / W4Linear ----------------------------------------------------------------------------------------------
def _formula(model_fp, names):
    total = before = 0
    for p in names:
        w = model_fp.get_submodule(p).weight
        total += w.numel() // 2 + 4 * (w.numel() // 64)
        before += w.numel() * w.element_size()
    return total, before


@pytest.mark.parametrize("kind", ["llama", "gpt2"])
def test_quantize_model_structure(kind):
    import copy

    from genlm_backend_amd.quant import W4Config, W4Linear, quantize_model

    model = _llama() if kind == "llama" else _gpt2()
    names = LLAMA_LINEARS if kind == "llama" else GPT2_LINEARS
    ref = copy.deepcopy(model)
    head_ptr = model.get_output_embeddings().weight.data_ptr()
    rep = quantize_model(model, W4Config("nf4", None, None), Engine())
    assert sorted(rep["modules"]) == sorted(names)
    assert list(rep["skipped"]) == ["lm_head"]
    for p in names:
        q = model.get_submodule(p)
        assert isinstance(q, W4Linear) and not hasattr(q, "weight")
        w = ref.get_submodule(p).weight
        n, k = (w.shape[1], w.shape[0]) if kind == "gpt2" else w.shape
        assert (q.out_features, q.in_features) == (n, k) and q.image.numel() == n * k // 2 + 4 * (n * k // 64)
        # the module computes x . W'^T + b with W' the restatement's round trip of the layer's weight
        wq = Q.roundtrip(w.T if kind == "gpt2" else w, Q.codebook("nf4"))
        assert torch.equal(q.dequantize(torch.float32), wq)
        x = torch.randn(3, 5, k)
        b = ref.get_submodule(p).bias
        with torch.no_grad():
            assert torch.allclose(q(x), torch.nn.functional.linear(x, wq, b), atol=1e-6)
    # the output embedding (tied to the input embedding in both) is untouched
    assert isinstance(model.get_output_embeddings(), torch.nn.Linear)
    assert model.get_output_embeddings().weight.data_ptr() == head_ptr
    assert torch.equal(model.get_output_embeddings().weight, ref.get_output_embeddings().weight)
    assert (rep["bytes"], rep["bytes_before"]) == _formula(ref, names)
    assert rep["quant_type"] == "nf4" and rep["compute_dtype"] is None
    with pytest.raises(RuntimeError, match="inference only"):
        model.get_submodule(names[0])(torch.randn(2, model.get_submodule(names[0]).in_features, requires_grad=True))


def test_skip_list_and_other_widths():
    from genlm_backend_amd.quant import W4Config, W4Linear, quantize_model

    model = _llama(tie=False)
    rep = quantize_model(model, W4Config("fp4", torch.float32, ["q_proj", "model.layers.1.mlp"]), Engine())
    for p in LLAMA_LINEARS:
        skipped = p.endswith("q_proj") or p.startswith("model.layers.1.mlp")
        assert isinstance(model.get_submodule(p), W4Linear) != skipped, p
        assert (p in rep["skipped"]) == skipped
    # a skip list REPLACES the default (transformers does the same): the untied head, K = 64, is quantised
    assert isinstance(model.lm_head, W4Linear) and "lm_head" in rep["modules"]
    # without a list an untied head is still the output embedding and stays
    model = _llama(tie=False)
    rep = quantize_model(model, W4Config("fp4", None, None), Engine())
    assert isinstance(model.lm_head, torch.nn.Linear) and "lm_head" in rep["skipped"]
    # input widths that are no multiple of 64 stay, with the reason
    from transformers import LlamaConfig, LlamaForCausalLM

    small = LlamaForCausalLM(LlamaConfig(vocab_size=V, hidden_size=32, intermediate_size=64, num_hidden_layers=1,
                                         num_attention_heads=4, num_key_value_heads=2, head_dim=8)).eval()
    rep = quantize_model(small, W4Config("nf4", None, None), Engine())
    assert rep["modules"] == ["model.layers.0.mlp.down_proj"]
    assert "multiple of 64" in rep["skipped"]["model.layers.0.self_attn.q_proj"]
    # weights must be finite
    bad = _llama()
    with torch.no_grad():
        bad.model.layers[0].mlp.up_proj.weight[3, 5] = float("inf")
    with pytest.raises(ValueError, match="not finite"):
        quantize_model(bad, W4Config("nf4", None, None), Engine())


def _snapshot(model):
    return {k: (id(m), type(m), {n: (id(p), p._version) for n, p in m._parameters.items() if p is not None},
                {n: id(b) for n, b in m._buffers.items() if b is not None}) for k, m in model.named_modules()}


@pytest.mark.parametrize("kind", ["llama", "gpt2"])
def test_backend_over_a_quantised_model(kind, tmp_path):
    """A model that already holds W4Linear modules is served by the constructor and not modified; its log-probs are those of
    the same architecture holding the dequantised weights; set_lora refuses, the other LoRA calls and the caches work."""
    import copy

    from genlm_backend_amd.llm import AsyncAmdLM
    from genlm_backend_amd.quant import W4Config, quantize_model
    from tests.test_lora_cpu import write_adapter

    model = _llama() if kind == "llama" else _gpt2()
    names = LLAMA_LINEARS if kind == "llama" else GPT2_LINEARS
    ref = copy.deepcopy(model)
    with torch.no_grad():
        for p in names:
            w = ref.get_submodule(p).weight
            wq = Q.roundtrip(w.T if kind == "gpt2" else w, Q.codebook("fp4"))
            w.copy_(wq.T if kind == "gpt2" else wq)
    eng = Engine()
    rep = quantize_model(model, W4Config("fp4", None, None), eng)
    before = _snapshot(model)
    llm = AsyncAmdLM(model, None, batch_size=64, timeout=0.02, engine=eng, w4_gemm="dequant")
    llm.tokenizer = Tok()
    assert llm.quantization is rep and llm.w4_gemm == "dequant"
    ctxs = [[3, 1, 4, 1, 5], [9, 2, 6, 5, 3, 5], [8, 9], [7]]
    got = llm.batch_next_token_logprobs_sync(ctxs)
    for ctx, row in zip(ctxs, got):
        with torch.no_grad():
            want = torch.log_softmax(ref(torch.tensor([ctx])).logits[0, -1].float(), -1)
        assert torch.allclose(row.float().cpu(), want, atol=1e-4)
    assert _snapshot(model) == before
    write_adapter(str(tmp_path / "ad"), ref, names[:2])
    llm.add_new_lora(str(tmp_path / "ad"), "a")
    with pytest.raises(ValueError, match="quantised"):
        llm.set_lora(lora_name="a")
    llm.clear_lora()
    llm.refresh_weights()
    llm.clear_cache()
    again = llm.batch_next_token_logprobs_sync(ctxs)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    with pytest.raises(ValueError, match="w4_gemm"):
        AsyncAmdLM(model, None, engine=eng, w4_gemm="sometimes")
    plain = AsyncAmdLM(ref, None, engine=eng)
    assert plain.quantization is None
