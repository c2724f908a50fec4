"""A different LoRA adapter per context in one batched forward, on the CPU (the HIP engine replaced by
tests/lora_rows_engine.py): `lora_names` on the batched calls against peft's unmerged hooks on the caller's model, per third
of a mixed batch; order, dedup on (adapter, context), the fused step, the caches left alone, a 4-bit base, the errors."""
import copy

import numpy as np
import pytest
import torch

from tests import quant4_engine as Q
from tests import test_quant4_cpu as TQ
from tests.lora_rows_engine import LoraRowsOracleEngine
from tests.test_lora_cpu import (CTXS, GPT2_TARGETS, LLAMA_TARGETS, TOL, V, Tok, _gpt2, _llama, _same, _snapshot,
                                 hooked_reference, ref_logprobs, write_adapter)


def make_llm(model, engine=None, **kw):
    from genlm_backend_amd.llm import AsyncAmdLM

    m = AsyncAmdLM(model, None, batch_size=64, timeout=0.02, engine=engine or LoraRowsOracleEngine(), **kw)
    m.tokenizer = Tok()
    return m


def _f32(spec):
    return {p: (a, b, float(np.float32(s)), conv) for p, (a, b, s, conv) in spec.items()}


def _setup(kind, tmp_path):
    """Two adapters with different targets and ranks: `a` over every target (GPT-2: Conv1D fan_in_fan_out; Llama: rslora,
    rank_pattern, a targeted lm_head), `b` over a subset with another rank."""
    if kind == "gpt2":
        model = _gpt2()
        sa = write_adapter(tmp_path / "a", model, GPT2_TARGETS, fan_in_fan_out=True, seed=1, rank_pattern={"c_fc": 6})
        sb = write_adapter(tmp_path / "b", model, GPT2_TARGETS[1:6], r=3, alpha=9.0, fan_in_fan_out=True, seed=7, rslora=True)
    else:
        model = _llama()
        sa = write_adapter(tmp_path / "a", model, LLAMA_TARGETS, r=4, alpha=16, rslora=True, seed=2,
                           rank_pattern={"q_proj": 8, "lm_head": 2}, alpha_pattern={"down_proj": 3.0})
        sb = write_adapter(tmp_path / "b", model, LLAMA_TARGETS[2:11], r=5, alpha=10.0, seed=8, dtype=torch.bfloat16)
    return model, _f32(sa), _f32(sb)


def _llm(kind, tmp_path, **kw):
    model, sa, sb = _setup(kind, tmp_path)
    llm = make_llm(model, **kw)
    llm.add_new_lora(str(tmp_path / "a"), "a")
    llm.add_new_lora(str(tmp_path / "b"), "b")
    refs = {None: model, "a": hooked_reference(model, sa), "b": hooked_reference(model, sb)}
    return model, llm, refs


NAMES = [None] * 5 + ["a"] * 5 + ["b"] * 5


@pytest.mark.parametrize("kind", ["gpt2", "llama"])
@pytest.mark.parametrize("shadow", [True, False])
def test_mixed_batch_matches_the_hooked_references(tmp_path, kind, shadow):
    kw = {} if shadow else dict(fuse_activations=False, glb_attention=False)
    model, llm, refs = _llm(kind, tmp_path, **kw)
    got = llm.batch_next_token_logprobs_sync(CTXS * 3, lora_names=NAMES).numpy()
    want = np.stack([ref_logprobs(refs[nm], c) for nm, c in zip(NAMES, CTXS * 3)])
    for third in range(3):
        sl = slice(5 * third, 5 * third + 5)
        assert np.abs(got[sl] - want[sl]).max() < TOL, NAMES[5 * third]
    # the adapters matter: they differ from the base and from each other on some row
    assert np.abs(want[5:10] - want[0:5]).max() > 10 * TOL
    assert np.abs(want[10:15] - want[0:5]).max() > 10 * TOL
    assert np.abs(want[10:15] - want[5:10]).max() > 10 * TOL
    assert llm.stats["lora_rows_calls"] > 0 and llm.stats["unique"] == 15 and llm.stats["queries"] == 15


def test_shuffled_order_gives_the_same_rows(tmp_path):
    model, llm, _ = _llm("llama", tmp_path)
    got = llm.batch_next_token_logprobs_sync(CTXS * 3, lora_names=NAMES).numpy()
    perm = np.random.default_rng(5).permutation(15)
    ctxs = [(CTXS * 3)[i] for i in perm]
    names = [NAMES[i] for i in perm]
    shuffled = llm.batch_next_token_logprobs_sync(ctxs, lora_names=names).numpy()
    inv = np.argsort(perm)
    assert np.abs(shuffled[inv] - got).max() < TOL
    assert np.array_equal(shuffled[inv].argmax(-1), got.argmax(-1))


def test_dedup_is_on_adapter_and_context(tmp_path):
    model, llm, refs = _llm("gpt2", tmp_path)
    c = CTXS[0]
    names = [None, "a", "b", "a", None, "a"]
    before = llm.stats["unique"]
    got = llm.batch_next_token_logprobs_sync([c] * 6, lora_names=names).numpy()
    assert llm.stats["unique"] - before == 3  # equal (context, adapter) pairs are evaluated once
    assert np.abs(got[0] - got[1]).max() > 10 * TOL and np.abs(got[1] - got[2]).max() > 10 * TOL
    assert np.array_equal(got[1], got[3]) and np.array_equal(got[1], got[5]) and np.array_equal(got[0], got[4])
    for row, nm in zip(got, names):
        assert np.abs(row - ref_logprobs(refs[nm], c)).max() < TOL


@pytest.mark.parametrize("kind", ["gpt2", "llama"])
def test_the_fused_step_under_mixed_adapters(tmp_path, kind):
    model, llm, refs = _llm(kind, tmp_path)
    rs = np.random.default_rng(3)
    masks = np.where(rs.random((2, V)) < 0.5, 0.0, -np.inf).astype(np.float32)
    llm.register_masks(torch.from_numpy(masks))
    ctxs = [c + [5] for c in CTXS * 3]
    for _ in range(3):
        mids = [i % 2 for i in range(len(ctxs))]
        logZ, tok = llm.batch_next_token_step_sync(ctxs, mids, lora_names=NAMES)
        want = [np.logaddexp.reduce((ref_logprobs(refs[nm], c) + masks[m]).astype(np.float64))
                for nm, c, m in zip(NAMES, ctxs, mids)]
        assert np.abs(np.asarray(logZ) - np.asarray(want)).max() < TOL
        assert all(masks[m][t] == 0 for m, t in zip(mids, np.asarray(tok)))
        ctxs = [c + [int(t)] for c, t in zip(ctxs, np.asarray(tok))]


@pytest.mark.parametrize("shadow", [True, False])
def test_the_caches_and_the_callers_model_are_left_alone(tmp_path, shadow):
    kw = {} if shadow else dict(fuse_activations=False, glb_attention=False)
    for kind in ("gpt2", "llama"):
        model, sa, sb = _setup(kind, tmp_path / kind)
        before = _snapshot(model)
        llm = make_llm(model, **kw)
        never = make_llm(model, **kw)  # a backend that never loads an adapter
        llm.add_new_lora(str(tmp_path / kind / "a"), "a")
        llm.add_new_lora(str(tmp_path / kind / "b"), "b")
        first = llm.batch_next_token_logprobs_sync(CTXS).numpy()
        plain = never.batch_next_token_logprobs_sync(CTXS).numpy()
        assert np.array_equal(first.view(np.uint32), plain.view(np.uint32))
        llm.batch_next_token_logprobs_sync(CTXS * 3, lora_names=NAMES)
        llm.batch_next_token_step_sync(CTXS * 3, lora_names=NAMES)
        _same(before, _snapshot(model))
        assert llm.active_lora is None
        batches = llm.stats["batches"]
        again = llm.batch_next_token_logprobs_sync(CTXS).numpy()  # the output trie still serves them: no forward
        assert llm.stats["batches"] == batches
        assert np.array_equal(again.view(np.uint32), first.view(np.uint32))
        llm.clear_cache()
        fresh = llm.batch_next_token_logprobs_sync(CTXS).numpy()  # ... and a new forward gives the same bits
        assert llm.stats["batches"] == batches + 1
        assert np.array_equal(fresh.view(np.uint32), first.view(np.uint32))
        # no wrapper is left in the tree the forwards run on
        assert not any(type(m).__name__ == "RowLoraModule" for m in llm._net.modules())


class W4Engine(Q.StubW4Engine, LoraRowsOracleEngine):
    pass


@pytest.mark.parametrize("kind", ["llama", "gpt2"])
def test_over_a_quantised_base(tmp_path, kind):
    """Built as tests/test_quant4_cpu.py::test_backend_over_a_quantised_model builds it: the reference holds the dequantised
    weights, plus the unmerged hooks."""
    from genlm_backend_amd.quant import W4Config, quantize_model

    model = TQ._llama() if kind == "llama" else TQ._gpt2()
    names = TQ.LLAMA_LINEARS if kind == "llama" else TQ.GPT2_LINEARS
    ref = copy.deepcopy(model)
    with torch.no_grad():
        for p in names:
            w = ref.get_submodule(p).weight
            wq = Q.roundtrip(w.T if kind == "gpt2" else w, Q.codebook("fp4"))
            w.copy_(wq.T if kind == "gpt2" else wq)
    eng = W4Engine()
    quantize_model(model, W4Config("fp4", None, None), eng)
    llm = make_llm(model, engine=eng, w4_gemm="dequant")
    sa = _f32(write_adapter(str(tmp_path / "a"), ref, names, r=4, alpha=32.0, seed=3, fan_in_fan_out=kind == "gpt2"))
    sb = _f32(write_adapter(str(tmp_path / "b"), ref, names[3:9], r=2, alpha=16.0, seed=4, fan_in_fan_out=kind == "gpt2"))
    llm.add_new_lora(str(tmp_path / "a"), "a")
    llm.add_new_lora(str(tmp_path / "b"), "b")
    refs = {None: ref, "a": hooked_reference(ref, sa), "b": hooked_reference(ref, sb)}
    ctxs = [[3, 1, 4, 1, 5], [9, 2, 6, 5, 3, 5], [8, 9], [7]]
    nm = [None] * 4 + ["a"] * 4 + ["b"] * 4
    got = llm.batch_next_token_logprobs_sync(ctxs * 3, lora_names=nm)
    want = torch.stack([torch.from_numpy(ref_logprobs(refs[k], c)) for k, c in zip(nm, ctxs * 3)])
    assert torch.allclose(got.float().cpu(), want, atol=1e-4)
    assert (want[4:8] - want[0:4]).abs().max() > 1e-3 and (want[8:12] - want[4:8]).abs().max() > 1e-3
    with pytest.raises(ValueError, match="quantised"):
        llm.set_lora(lora_name="a")


def test_errors(tmp_path, monkeypatch):
    model, llm, _ = _llm("gpt2", tmp_path)
    with pytest.raises(ValueError, match="has not been loaded"):
        llm.batch_next_token_logprobs_sync(CTXS, lora_names=["a", "nope", None, None, None])
    with pytest.raises(ValueError, match="entries"):
        llm.batch_next_token_logprobs_sync(CTXS, lora_names=["a"])
    with pytest.raises(ValueError, match="entries"):
        llm.batch_next_token_step_sync(CTXS, None, lora_names=["a"] * 6)
    llm.set_lora(lora_name="a")
    with pytest.raises(ValueError, match="merged adapter"):
        llm.batch_next_token_logprobs_sync(CTXS, lora_names=[None] * 5)
    with pytest.raises(ValueError, match="merged adapter"):
        llm.batch_next_token_step_sync(CTXS, lora_names=["b"] * 5)
    llm.clear_lora()
    assert llm.batch_next_token_logprobs_sync(CTXS, lora_names=["b"] * 5).shape == (5, V)
    # more slots than the limit: loading is fine, the mixed call raises
    from genlm_backend_amd import lora

    assert lora.MAX_ROW_SLOTS >= 8
    write_adapter(tmp_path / "c", model, GPT2_TARGETS[:1], fan_in_fan_out=True, seed=9)
    for i in range(lora.MAX_ROW_SLOTS - 1):
        llm.add_new_lora(str(tmp_path / "c"), f"c{i}")
    assert len(llm._loras) == lora.MAX_ROW_SLOTS + 1
    with pytest.raises(ValueError, match="at most"):
        llm.batch_next_token_logprobs_sync(CTXS, lora_names=[None] * 5)
    assert llm.batch_next_token_logprobs_sync(CTXS).shape == (5, V)  # (default calls are not concerned)


def test_rows_2d_takes_the_pitch_from_a_dimension_that_has_one():
    """The stride of a dimension of size 1 is arbitrary: the row pitch comes from the innermost row dimension of size > 1."""
    from genlm_backend_amd.engine import HipEngine

    rows_2d = HipEngine._rows_2d
    base = torch.zeros(256)
    assert rows_2d(base.as_strided((4, 1, 32), (40, 7, 1)), "y") == (4, 40)  # [U, 1, N], an odd stride on the middle
    assert rows_2d(base.as_strided((1, 1, 32), (5, 7, 1)), "y") == (1, 32)  # one row: the pitch is its length
    assert rows_2d(base.as_strided((2, 2, 32), (80, 40, 1)), "y") == (4, 40)
    assert rows_2d(torch.zeros(3, 5, 48)[..., 16:32], "y") == (15, 48)  # a column slice
    with pytest.raises(ValueError):
        rows_2d(base.as_strided((2, 2, 32), (96, 40, 1)), "y")  # two pitches
    with pytest.raises(ValueError):
        rows_2d(torch.zeros(8, 4).T, "y")  # no unit inner stride
