"""Auto-KV rows that serve any shared prefix (auto_kv_chunk > 1) on the CPU: the host logic runs against the
pure-Python restatement of the matcher and the chunk plan (tests/kv_chunk_engine.py), the chunk forwards take the SDPA path
with the explicit mask."""
import ast
import asyncio
import os

import numpy as np
import pytest
import torch

from tests.kv_chunk_engine import ChunkCpuEngine, call_sequence, kv_plan_chunk, match_prefix_rows, run_sequence

G = os.path.join(os.path.dirname(__file__), "golden", "ref_hotpath_tiny.npz")
TOL = 1e-4  # (tests/test_host_cpu.py: log-probs within 1e-4 of the reference's transformers-CPU path)


class Tok:
    pad_token_id = None
    eos_token_id = 0


@pytest.fixture(scope="module")
def gold():
    return np.load(G)


def _gpt2(gold, **kw):
    from transformers import GPT2Config, GPT2LMHeadModel

    from genlm_backend_amd.llm import AsyncAmdLM

    cfg = ast.literal_eval(bytes(gold["config_json"]).decode())
    model = GPT2LMHeadModel(GPT2Config(**cfg)).eval()
    model.load_state_dict({k[3:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("w::")})
    m = AsyncAmdLM(model, None, batch_size=64, timeout=0.02, engine=ChunkCpuEngine(), **kw)
    m.tokenizer = Tok()
    m.register_masks(torch.from_numpy(gold["sis_masks"]))
    return m, cfg["vocab_size"]


def test_constructor_takes_and_validates_auto_kv_chunk(gold):
    m, _ = _gpt2(gold, auto_kv_rows=10, auto_kv_cap=24, auto_kv_chunk=8)
    assert m._auto_kv.chunk == 8 and m._auto_kv.stats["chunk_rows"] == 0 and m._auto_kv.stats["chunk_tokens"] == 0
    assert _gpt2(gold, auto_kv_rows=4)[0]._auto_kv.chunk == 1
    for bad in (0, 17, -1, 2.0, True):
        with pytest.raises(ValueError):
            _gpt2(gold, auto_kv_rows=10, auto_kv_chunk=bad)
    with pytest.raises(ValueError):
        _gpt2(gold, auto_kv_chunk=4)  # no rows to share prefixes in


@pytest.mark.parametrize("collide", [False, True])
def test_chunk_rows_match_a_backend_without_rows(gold, collide):
    """Twelve contexts over ten rows of 24 positions, fourteen calls, auto_kv_chunk = 8: logZ, tokens (torch draws) and
    log-prob rows equal those of a backend without rows and of auto_kv_chunk = 1; the stats equal the test's own count of
    the contexts that had a usable relative.  `collide`: every context hashes to one value."""
    V = _gpt2(gold)[1]
    run_sequence(lambda **kw: _gpt2(gold, **kw)[0], V, TOL, collide=collide)


def test_the_callers_model_is_untouched_and_one_token_calls_still_run_in_place(gold):
    m, V = _gpt2(gold, auto_kv_rows=8, auto_kv_cap=24, auto_kv_chunk=4)
    before = {k: v.clone() for k, v in m.model.state_dict().items()}
    mods = {n: type(x) for n, x in m.model.named_modules()}
    impl = m.model.config._attn_implementation
    rnd = np.random.default_rng(4)
    ctxs = [[int(t) for t in rnd.integers(1, V, 3)] for _ in range(8)]
    m.batch_next_token_step_sync(ctxs, [0] * 8)
    ctxs = [c + [int(t) for t in rnd.integers(1, V, 3)] for c in ctxs]  # chunks of three
    m.batch_next_token_step_sync(ctxs, [0] * 8)
    assert m._auto_kv.stats["chunk_rows"] == 8 and m._auto_kv.stats["chunk_tokens"] == 24
    calls = m._auto_kv.stats["in_place_calls"]
    for _ in range(3):  # one token each: every row is live, the forward runs on the slab where the rows lie
        ctxs = [c + [int(rnd.integers(1, V))] for c in ctxs]
        m.batch_next_token_step_sync(ctxs, [0] * 8)
    assert m._auto_kv.stats["in_place_calls"] == calls + 3 and m._auto_kv.stats["one_token_rows"] == 24
    # a mixed call: six rows grow by one token (in place), two by two (chunk rows, after the in-place forward)
    ctxs = [c + [int(t) for t in rnd.integers(1, V, 2 if i < 2 else 1)] for i, c in enumerate(ctxs)]
    plain, _ = _gpt2(gold)
    z0, _ = plain.batch_next_token_step_sync(ctxs, [0] * 8)
    z1, _ = m.batch_next_token_step_sync(ctxs, [0] * 8)
    assert np.abs(z0 - z1).max() < TOL
    assert m._auto_kv.stats["in_place_calls"] == calls + 4 and m._auto_kv.stats["chunk_rows"] == 10
    assert impl == m.model.config._attn_implementation and mods == {n: type(x) for n, x in m.model.named_modules()}
    for k, v in m.model.state_dict().items():
        assert torch.equal(v, before[k]), k


def test_rotary_model_sees_the_chunk_positions():
    """A Llama-shaped model (grouped query heads, rotary positions) in float32: chunk rows through the explicit-mask path
    equal the plain backend."""
    from transformers import LlamaConfig, LlamaForCausalLM

    from genlm_backend_amd.llm import AsyncAmdLM

    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=96, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, max_position_embeddings=64)
    model = LlamaForCausalLM(cfg).eval()

    def make(**kw):
        m = AsyncAmdLM(model, None, batch_size=64, timeout=0.02, engine=ChunkCpuEngine(), **kw)
        m.tokenizer = Tok()
        return m

    plain, chunk = make(), make(auto_kv_rows=8, auto_kv_cap=24, auto_kv_chunk=8)
    for call, (ctxs, _) in enumerate(call_sequence(96, n_ctx=6, n_calls=8)):
        for m in (plain, chunk):
            m.set_rng("torch", 5 + call)
        z0, t0 = plain.batch_next_token_step_sync(ctxs, [0] * len(ctxs))
        z1, t1 = chunk.batch_next_token_step_sync(ctxs, [0] * len(ctxs))
        assert np.abs(z0 - z1).max() < TOL and np.array_equal(t0, t1), call
    assert chunk._auto_kv.stats["chunk_rows"] > 0


def test_restatement_rules_on_hand_made_tables():
    """The tie rules and the in-place rule, on tables small enough to read."""
    row_tok = np.zeros((6, 8), np.int32)
    rows = [[1, 2, 3], [1, 2, 3, 4, 5], [1, 2, 3, 4, 9, 9], [1, 2, 3, 4, 5], [7], []]
    row_len = np.array([len(r) for r in rows], np.int32)
    for r, t in enumerate(rows):
        row_tok[r, :len(t)] = t
    ctxs = [[1, 2, 3, 4, 5], [1, 2, 3, 4, 6, 6], [7, 7, 7, 7], [5], [1, 2, 3, 4, 5, 6, 7, 8, 9]]
    old, keep, _ = match_prefix_rows(ctxs, np.arange(5), 5, row_tok, row_len, 3)
    # exact holder beats the longer row and the later copy; the sibling of length 6 is served by the smallest row with 4
    # shared tokens; keep 1 with 3 to feed; a one-token context has no prefix; longer than a row
    assert old.tolist() == [1, 1, 4, -1, -1] and keep.tolist() == [4, 4, 1, 0, 0]
    assert match_prefix_rows(ctxs, np.arange(5), 5, row_tok, row_len, 1)[0].tolist() == [1, -1, -1, -1, -1]
    plan = kv_plan_chunk(np.arange(5), np.arange(5), 5, old, keep, np.array([len(c) for c in ctxs]), 6, 8, row_len)
    # group 0 keeps row 1 in place (it holds keep + 1 tokens), group 1 copies its own 4 tokens of it into the first free
    # row, group 2 keeps row 4; groups 3 and 4 are encoded (4: too long for a row, nobody keeps it)
    assert plan["group_row"].tolist() == [1, 0, 4, 2, -1]
    assert (plan["copy_src"][0], plan["copy_len"][0]) == (1, 4)
    assert plan["head"].tolist() == [5, 3, 2, 1, 1, 9, 4, 0, 2, 3]
    assert plan["rows_a"][:3].tolist() == [1, 0, 4] and plan["n_new_a"][:3].tolist() == [1, 2, 3] and plan["pos_a"][:3].tolist() == [4, 4, 1]
    # a row longer than keep + 1 is never truncated in place: the only group copies, the long row is not free
    plan = kv_plan_chunk(np.arange(1), np.arange(1), 1, np.array([2]), np.array([4]), np.array([6]), 6, 8, row_len)
    assert plan["group_row"][0] == 0 and plan["copy_src"][0] == 2 and plan["copy_len"][0] == 4 and plan["head"][6] == 5
