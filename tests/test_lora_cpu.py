"""LoRA adapters on the CPU (the HIP engine replaced by tests/lora_engine.py, which merges by the kernel's contract restated
bit for bit): peft-format adapters load without peft and are validated, results under an adapter match two independent
references - a model merged in float64 and the caller's model with peft's unmerged hooks -, adapter swaps are bit-identical
to unswapped runs, the caller's model is never modified, base-weight edits reach the merge, stale populations refuse to step."""
import asyncio
import copy
import ctypes
import ctypes.util
import json
import math
import os

import numpy as np
import pytest
import torch

from tests.lora_engine import LoraOracleEngine, fmaf

TOL = 1e-4
V = 96


class Tok:
    pad_token_id = None
    eos_token_id = 0


def _gpt2():
    from transformers import GPT2Config, GPT2LMHeadModel

    torch.manual_seed(11)
    return GPT2LMHeadModel(GPT2Config(vocab_size=V, n_embd=32, n_layer=2, n_head=4, n_positions=64)).eval()


def _llama():
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(12)
    return LlamaForCausalLM(LlamaConfig(vocab_size=V, hidden_size=32, intermediate_size=64, num_hidden_layers=2,
                                        num_attention_heads=4, num_key_value_heads=2, head_dim=8, max_position_embeddings=64,
                                        bos_token_id=1, eos_token_id=2, tie_word_embeddings=True)).eval()


GPT2_TARGETS = [f"transformer.h.{i}.{m}" for i in range(2) for m in ("attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj")]
LLAMA_TARGETS = [f"model.layers.{i}.{m}" for i in range(2) for m in (
    "self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
    "mlp.down_proj")] + ["lm_head"]


def _pattern(patterns, path, default):
    import re

    for k, v in (patterns or {}).items():
        if re.match(rf"(.*\.)?{k}$", path):
            return v
    return default


def write_adapter(d, model, targets, r=4, alpha=8.0, seed=0, fan_in_fan_out=False, rank_pattern=None, alpha_pattern=None,
                  rslora=False, dtype=torch.float32, name_segment=False, cfg_extra=None, keys_extra=None, shape_off=0):
    """A peft-format LoRA adapter for `model` in directory d; returns {path: (A, B, scale as float64, conv1d)}."""
    from safetensors.torch import save_file

    os.makedirs(d, exist_ok=True)
    g = torch.Generator().manual_seed(seed)
    tensors, spec = {}, {}
    for p in targets:
        mod = model.get_submodule(p)
        conv = type(mod).__name__ == "Conv1D"
        k_in, n_out = (mod.weight.shape[0], mod.weight.shape[1]) if conv else (mod.weight.shape[1], mod.weight.shape[0])
        rr = _pattern(rank_pattern, p, r)
        al = _pattern(alpha_pattern, p, alpha)
        a = (torch.randn(rr, k_in + shape_off, generator=g) * 0.04).to(dtype)
        b = (torch.randn(n_out, rr, generator=g) * 0.04).to(dtype)
        seg = ".default" if name_segment else ""
        tensors[f"base_model.model.{p}.lora_A{seg}.weight"] = a
        tensors[f"base_model.model.{p}.lora_B{seg}.weight"] = b
        spec[p] = (a, b, al / math.sqrt(rr) if rslora else al / rr, conv)
    tensors.update(keys_extra or {})
    save_file(tensors, os.path.join(d, "adapter_model.safetensors"))
    cfg = dict(peft_type="LORA", r=r, lora_alpha=alpha, target_modules=sorted({p.split(".")[-1] for p in targets}),
               fan_in_fan_out=fan_in_fan_out, use_rslora=rslora, rank_pattern=rank_pattern or {},
               alpha_pattern=alpha_pattern or {}, lora_dropout=0.05, bias="none", modules_to_save=None, use_dora=False)
    cfg.update(cfg_extra or {})
    with open(os.path.join(d, "adapter_config.json"), "w") as f:
        json.dump(cfg, f)
    return spec


def merged_reference(model, spec):
    """A second model whose targeted weights were merged in float64 (a tied lm_head gets its own weight)."""
    ref = copy.deepcopy(model)
    with torch.no_grad():
        for p, (a, b, s, conv) in spec.items():
            mod = ref.get_submodule(p)
            delta = s * (b.double() @ a.double())
            w = mod.weight.double() + (delta.T if conv else delta)
            mod.weight = torch.nn.Parameter(w.to(mod.weight.dtype))
    return ref


def hooked_reference(model, spec):
    """The caller's model (a copy) with peft's unmerged semantics: every targeted module's output + s (x A^T) B^T."""
    ref = copy.deepcopy(model)
    for p, (a, b, s, conv) in spec.items():
        def hook(mod, args, out, a=a.float(), b=b.float(), s=s):
            return out + s * ((args[0] @ a.T) @ b.T)

        ref.get_submodule(p).register_forward_hook(hook)
    return ref


def ref_logprobs(ref, ctx):
    with torch.no_grad():
        return torch.log_softmax(ref(torch.tensor([ctx])).logits[0, -1].float(), -1).numpy()


def make_llm(model, **kw):
    from genlm_backend_amd.llm import AsyncAmdLM

    m = AsyncAmdLM(model, None, batch_size=64, timeout=0.02, engine=LoraOracleEngine(), **kw)
    m.tokenizer = Tok()
    return m


CTXS = [[3, 1, 4, 1, 5], [9, 2, 6, 5, 3, 5], [8, 9], [7], [3, 1, 4, 1, 5, 9, 2]]


# ---- the contract's arithmetic -----------------------------------------------------------------------------------------
def test_numpy_fmaf_is_libm_fmaf():
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    rs = np.random.default_rng(0)
    n = 4000
    cases = [
        tuple(rs.standard_normal(n).astype(np.float32) for _ in range(3)),
        # products with few bits plus addends on the float32 grid: many exact ties of the final rounding
        ((1 + rs.integers(0, 4096, n) / 4096).astype(np.float32), (1 + rs.integers(0, 4096, n) / 4096).astype(np.float32),
         (rs.integers(-2 ** 20, 2 ** 20, n) * 2.0 ** -23).astype(np.float32)),
        # subnormal results and operands
        ((rs.standard_normal(n) * 1e-20).astype(np.float32), (rs.standard_normal(n) * 1e-20).astype(np.float32),
         (rs.standard_normal(n) * 1e-39).astype(np.float32)),
    ]
    a0, b0, _ = cases[0]
    cases.append((a0, b0, (-(a0.astype(np.float64) * b0)).astype(np.float32)))  # cancellation
    for a, b, c in cases:
        got = fmaf(a, b, c)
        want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- loading and validation --------------------------------------------------------------------------------------------
def test_gpt2_and_llama_adapters_load(tmp_path):
    from genlm_backend_amd.lora import load_adapter

    g = _gpt2()
    write_adapter(tmp_path / "g", g, GPT2_TARGETS, fan_in_fan_out=True)
    ad = load_adapter(str(tmp_path / "g"), g, "g")
    assert sorted(ad.modules) == sorted(GPT2_TARGETS) and all(m.transposed for m in ad.modules.values())
    assert ad.modules[GPT2_TARGETS[0]].scale == np.float32(8.0 / 4)
    ll = _llama()
    write_adapter(tmp_path / "l", ll, LLAMA_TARGETS, r=4, alpha=16, rslora=True, rank_pattern={"q_proj": 8, "lm_head": 2},
                  alpha_pattern={"down_proj": 3.0}, dtype=torch.bfloat16, name_segment=True)
    ad = load_adapter(str(tmp_path / "l"), ll, "l")
    assert len(ad.modules) == 15 and not any(m.transposed for m in ad.modules.values())
    q = ad.modules["model.layers.0.self_attn.q_proj"]
    assert q.rank == 8 and q.scale == float(np.float32(16 / math.sqrt(8))) and q.a.dtype == torch.bfloat16
    assert ad.modules["model.layers.1.mlp.down_proj"].scale == float(np.float32(3.0 / math.sqrt(4)))
    assert ad.modules["lm_head"].rank == 2
    llm = make_llm(ll)
    llm.add_new_lora(str(tmp_path / "l"), "l")
    assert llm.active_lora is None and llm.stats["lora_adapter_bytes"] > 0
    with pytest.raises(ValueError, match="already exists"):
        llm.add_new_lora(str(tmp_path / "l"), "l")
    with pytest.raises(ValueError, match="has not been loaded yet"):
        llm.set_lora(lora_name="nope")


@pytest.mark.parametrize("what", ["dora", "bias", "modules_to_save", "embedding", "peft_type", "no_module", "shape", "rank",
                                  "not_linear"])
def test_what_merging_cannot_serve_is_rejected(tmp_path, what):
    from genlm_backend_amd.lora import load_adapter

    g = _gpt2()
    kw = {}
    targets = GPT2_TARGETS[:2]
    if what == "dora":
        kw["cfg_extra"] = {"use_dora": True}
    elif what == "bias":
        kw["cfg_extra"] = {"bias": "lora_only"}
    elif what == "modules_to_save":
        kw["cfg_extra"] = {"modules_to_save": ["lm_head"]}
    elif what == "embedding":
        kw["keys_extra"] = {"base_model.model.transformer.wte.lora_embedding_A": torch.zeros(4, V)}
    elif what == "peft_type":
        kw["cfg_extra"] = {"peft_type": "IA3"}
    elif what == "no_module":
        kw["keys_extra"] = {"base_model.model.transformer.h.7.attn.c_attn.lora_A.weight": torch.zeros(4, 32),
                            "base_model.model.transformer.h.7.attn.c_attn.lora_B.weight": torch.zeros(96, 4)}
    elif what == "shape":
        kw["shape_off"] = 1
    elif what == "rank":
        kw["r"] = 257
    elif what == "not_linear":
        targets = ["transformer.ln_f"]
        kw["keys_extra"] = {}
    if what == "not_linear":
        from safetensors.torch import save_file

        os.makedirs(tmp_path / "a", exist_ok=True)
        save_file({"base_model.model.transformer.ln_f.lora_A.weight": torch.zeros(4, 32),
                   "base_model.model.transformer.ln_f.lora_B.weight": torch.zeros(32, 4)},
                  str(tmp_path / "a" / "adapter_model.safetensors"))
        with open(tmp_path / "a" / "adapter_config.json", "w") as f:
            json.dump(dict(peft_type="LORA", r=4, lora_alpha=8), f)
    else:
        write_adapter(tmp_path / "a", g, targets, **kw)
    with pytest.raises(ValueError):
        load_adapter(str(tmp_path / "a"), g, "a")
    llm = make_llm(g)
    with pytest.raises(ValueError):
        llm.add_new_lora(str(tmp_path / "a"), "a")
    assert llm.active_lora is None and not llm._loras


def test_adapter_in_bin_format(tmp_path):
    from genlm_backend_amd.lora import load_adapter
    from safetensors.torch import load_file

    g = _gpt2()
    write_adapter(tmp_path / "a", g, GPT2_TARGETS[:3], fan_in_fan_out=True)
    sd = load_file(str(tmp_path / "a" / "adapter_model.safetensors"))
    os.remove(tmp_path / "a" / "adapter_model.safetensors")
    torch.save(sd, tmp_path / "a" / "adapter_model.bin")
    assert len(load_adapter(str(tmp_path / "a"), g, "a").modules) == 3


# ---- results under an adapter --------------------------------------------------------------------------------------------
def _setup(kind, tmp_path):
    if kind == "gpt2":
        model = _gpt2()
        spec = write_adapter(tmp_path / "a", model, GPT2_TARGETS, fan_in_fan_out=True, seed=1)
    else:
        model = _llama()
        spec = write_adapter(tmp_path / "a", model, LLAMA_TARGETS, r=4, alpha=16, rslora=True, seed=2,
                             rank_pattern={"q_proj": 8, "lm_head": 2}, alpha_pattern={"down_proj": 3.0})
    spec = {p: (a, b, float(np.float32(s)), conv) for p, (a, b, s, conv) in spec.items()}
    return model, spec


def _steps(llm, ctxs, masks, rounds, refs=()):
    """`rounds` fused steps over the growing contexts (each context takes its drawn token); logZ of a masked row against
    logsumexp of the allowed log-probabilities of every reference."""
    for _ in range(rounds):
        mids = [i % 2 for i in range(len(ctxs))]
        logZ, tok = llm.batch_next_token_step_sync(ctxs, mids)
        for r in refs:
            lps = [ref_logprobs(r, c) for c in ctxs]
            wz = [np.logaddexp.reduce((lp + masks[m]).astype(np.float64)) for lp, m in zip(lps, mids)]
            assert np.abs(np.asarray(logZ) - np.asarray(wz)).max() < TOL
        assert all(masks[m][t] == 0 for m, t in zip(mids, np.asarray(tok)))
        ctxs = [c + [int(t)] for c, t in zip(ctxs, np.asarray(tok))]
    return ctxs


@pytest.mark.parametrize("kind", ["gpt2", "llama"])
@pytest.mark.parametrize("auto_rows", [0, 6])
@pytest.mark.parametrize("shadow", [True, False])
def test_results_under_an_adapter_match_two_references(tmp_path, kind, auto_rows, shadow):
    """Also without a shadow (fuse_activations=False, glb_attention=False: set_lora makes one) and with KV rows that follow
    the contexts (auto_kv_rows: 6 rows for 5 contexts, so their one-token forwards run in place, kv.SlabForward) built
    over the base model before the adapter is set: nothing made with the base weights serves a step under the adapter."""
    model, spec = _setup(kind, tmp_path)
    refs = [merged_reference(model, spec), hooked_reference(model, spec)]
    kw = {} if shadow else dict(fuse_activations=False, glb_attention=False)
    llm = make_llm(model, auto_kv_rows=auto_rows, auto_kv_cap=16, **kw)
    rs = np.random.default_rng(3)
    masks = np.where(rs.random((2, V)) < 0.5, 0.0, -np.inf).astype(np.float32)
    llm.register_masks(torch.from_numpy(masks))
    _steps(llm, [c + [5] for c in CTXS], masks, 3, refs=[model])  # (base weights: forwards and KV rows made over them)
    if auto_rows:
        assert llm._auto_kv.stats["in_place_calls"] > 0
    llm.add_new_lora(str(tmp_path / "a"), "a")
    llm.set_lora(lora_name="a")
    assert llm.active_lora == "a" and llm.stats["lora_merged_bytes"] > 0
    base_lp = ref_logprobs(model, CTXS[0])
    want = [[ref_logprobs(r, c) for c in CTXS] for r in refs]
    assert np.abs(want[0][0] - base_lp).max() > 10 * TOL  # (the adapter matters)
    for w in want:
        for c, wc in zip(CTXS, w):
            assert np.abs(llm.next_token_logprobs_sync(c).numpy() - wc).max() < TOL
            assert np.abs(llm.next_token_logprobs_uncached(c).numpy() - wc).max() < TOL
    llm.clear_cache()
    got = asyncio.run(llm.next_token_logprobs(CTXS[1])).numpy()
    assert np.abs(got - want[0][1]).max() < TOL
    llm.clear_cache()
    got = asyncio.run(llm.batch_next_token_logprobs(CTXS)).numpy()
    for w in want:
        assert np.abs(got - np.stack(w)).max() < TOL
    # the fused step under the adapter (later rounds find KV rows when auto_rows > 0, and run in place)
    _steps(llm, [c + [5] for c in CTXS], masks, 4, refs=refs)
    if auto_rows:
        assert llm._auto_kv.stats["in_place_calls"] > 0


def test_a_failed_merge_leaves_no_state_of_the_old_adapter(tmp_path):
    model, spec = _setup("gpt2", tmp_path)
    llm = make_llm(model)
    llm.add_new_lora(str(tmp_path / "a"), "a")
    llm.set_lora(lora_name="a")
    llm.next_token_logprobs_sync(CTXS[0])
    epoch, wepoch = llm.lora_epoch, llm.weights_epoch

    def fail(jobs):
        raise RuntimeError("merge failed")

    llm.engine.lora_merge = fail
    with pytest.raises(RuntimeError, match="merge failed"):
        llm.set_lora(lora_name="a")
    assert llm.active_lora is None and llm.lora_epoch == epoch + 1 and llm.weights_epoch == wepoch + 1
    assert not llm.cache.has_token(CTXS[0][0])  # (no row of the old adapter survives)
    assert np.abs(llm.next_token_logprobs_sync(CTXS[0]).numpy() - ref_logprobs(model, CTXS[0])).max() < TOL


def test_swaps_are_bit_identical_to_unswapped_runs(tmp_path):
    model = _llama()
    write_adapter(tmp_path / "a", model, LLAMA_TARGETS, r=4, alpha=8, seed=5)
    write_adapter(tmp_path / "b", model, LLAMA_TARGETS[:7], r=2, alpha=4, seed=6)

    def fresh(name):
        m = make_llm(model)
        if name is not None:
            m.add_new_lora(str(tmp_path / name), name)
            m.set_lora(lora_name=name)
        return m

    plain = {n: [fresh(n).next_token_logprobs_sync(c).numpy() for c in CTXS] for n in (None, "a", "b")}
    llm = make_llm(model)
    llm.add_new_lora(str(tmp_path / "a"), "a")
    llm.add_new_lora(str(tmp_path / "b"), "b")
    order = ["a", None, "b", "a", "a", None, None, "b", None, "a"]
    for step, name in enumerate(order):
        before = llm.stats["batches"]
        if name is None:
            llm.clear_lora()
        else:
            llm.set_lora(lora_name=name)
        assert llm.active_lora == name
        assert not llm.cache.has_token(CTXS[0][0])  # no row made before the switch is served after it
        for i in (step % len(CTXS), (step + 2) % len(CTXS)):
            got = llm.next_token_logprobs_sync(CTXS[i]).numpy()
            assert np.array_equal(got.view(np.uint32), plain[name][i].view(np.uint32)), (step, name, i)
        assert llm.stats["batches"] > before
    llm.clear_lora()
    llm.clear_lora()  # (a no-op that clears caches)
    assert llm.active_lora is None and llm.stats["lora_merged_bytes"] == 0


def _snapshot(model):
    snap = []
    for name, mod in model.named_modules():
        snap.append((name, id(mod._parameters), sorted(mod.__dict__), sorted(mod._forward_hooks),
                     [(k, id(p), p.data_ptr(), p._version, p.detach().clone()) for k, p in mod._parameters.items()
                      if p is not None]))
    return snap


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x[:4] == y[:4], x[0]
        for p, q in zip(x[4], y[4]):
            assert p[:4] == q[:4] and torch.equal(p[4], q[4]), (x[0], p[0])


@pytest.mark.parametrize("shadow", [True, False])
def test_the_callers_model_is_never_modified(tmp_path, shadow):
    for model, targets in ((_gpt2(), GPT2_TARGETS), (_llama(), LLAMA_TARGETS)):
        write_adapter(tmp_path / type(model).__name__, model, targets, fan_in_fan_out=targets is GPT2_TARGETS)
        before = _snapshot(model)
        kw = {} if shadow else dict(fuse_activations=False, glb_attention=False)
        llm = make_llm(model, **kw)
        assert (llm._net is model) != shadow
        base = llm.next_token_logprobs_uncached(CTXS[0]).numpy()
        llm.add_new_lora(str(tmp_path / type(model).__name__), "x")
        llm.set_lora(lora_name="x")
        assert llm._net is not model
        got = llm.next_token_logprobs_sync(CTXS[0]).numpy()
        assert np.abs(got - base).max() > 10 * TOL
        _same(before, _snapshot(model))
        llm.clear_lora()
        _same(before, _snapshot(model))
        again = llm.next_token_logprobs_uncached(CTXS[0]).numpy()
        assert np.abs(again - base).max() < TOL


def test_base_weight_changes_reach_the_merge(tmp_path):
    model, spec = _setup("gpt2", tmp_path)
    llm = make_llm(model)
    llm.add_new_lora(str(tmp_path / "a"), "a")
    llm.set_lora(lora_name="a")
    llm.next_token_logprobs_sync(CTXS[0])
    w = model.transformer.h[0].attn.c_attn.weight
    with torch.no_grad():
        w.mul_(1.25)  # in place: the version counter moves
    merges = llm.engine.merges
    got = llm.next_token_logprobs_uncached(CTXS[1]).numpy()
    assert llm.engine.merges == merges + 1
    assert np.abs(got - ref_logprobs(merged_reference(model, spec), CTXS[1])).max() < TOL
    w.data.copy_(w.data * 0.5)  # (no counter moves: refresh_weights)
    llm.refresh_weights()
    got = llm.next_token_logprobs_sync(CTXS[2]).numpy()
    assert np.abs(got - ref_logprobs(merged_reference(model, spec), CTXS[2])).max() < TOL
    assert np.abs(got - ref_logprobs(hooked_reference(model, spec), CTXS[2])).max() < TOL


def test_a_population_made_before_a_switch_refuses_to_step(tmp_path):
    from genlm_backend_amd.sis import DeviceSIS

    model, _ = _setup("gpt2", tmp_path)
    llm = make_llm(model)
    llm.add_new_lora(str(tmp_path / "a"), "a")
    sis = DeviceSIS(llm, 4, [3, 1, 4], max_tokens=3, eos_id=0, seed=1)
    sis.step()
    llm.set_lora(lora_name="a")
    with pytest.raises(RuntimeError, match="LoRA"):
        sis.step()
    sis2 = DeviceSIS(llm, 4, [3, 1, 4], max_tokens=3, eos_id=0, seed=1)
    sis2.step()
    llm.clear_lora()
    with pytest.raises(RuntimeError, match="LoRA"):
        sis2.step()
