"""`kv.encode_ragged` against the sequence it replaced, written out here: padded gather, prefix KV, transformer body, the
hidden rows at every context's last position, the layers' K / V.  Both sides run the same operations on the same inputs,
so every comparison is exact.  On the CPU the HIP engine is tests/cpu_engine.py; the `gpu` twin of the same cases runs the
real HipEngine in float32 and bfloat16."""
import numpy as np
import pytest
import torch

from tests.cpu_engine import CpuOracleEngine

V = 100


class Tok:
    pad_token_id = None
    eos_token_id = 0


PRE_A, PRE_B = [11, 12], [21, 22, 23]  # the cached prefixes (lengths 2 and 3)


def _contexts():
    """Nine contexts of lengths 1 .. 9 and two duplicates (of lengths 4 and 7); those of lengths 7 and 9 continue PRE_A,
    the one of length 5 continues PRE_B."""
    rs = np.random.default_rng(17)
    ctxs = [[int(t) for t in rs.integers(30, V, size=L)] for L in range(1, 10)]
    ctxs[6][:2], ctxs[8][:2], ctxs[4][:3] = PRE_A, PRE_A, PRE_B
    return ctxs + [list(ctxs[3]), list(ctxs[6])]


# four contexts out of order, one of them a duplicate's second copy (and two entries behind n_sel that must not be read)
SEL, N_SEL = [10, 1, 4, 8, 0, 2], 4
PREF_OF = {10: 0, 4: 1, 8: 0}  # context -> cached prefix; context 1 has none (-1)
CASES = ["plain", "prefixes", "keep_kv"]


def _llm(engine, device, dtype):
    from transformers import GPT2Config, GPT2LMHeadModel

    import genlm_backend_amd  # noqa: F401
    from genlm_backend_amd.llm import AsyncAmdLM

    torch.manual_seed(5)
    model = GPT2LMHeadModel(GPT2Config(vocab_size=V, n_embd=64, n_layer=2, n_head=2, n_positions=32)).eval()
    m = AsyncAmdLM(model.to(dtype).to(device), None, engine=engine)
    m.tokenizer = Tok()
    return m


def _check(llm, case):
    from genlm_backend_amd.cache import KVPrefix
    from genlm_backend_amd.kv import PrefixTable, encode_ragged, ragged

    eng, dev = llm.engine, llm.device
    ctxs = _contexts()
    batch = tuple(torch.from_numpy(a).to(dev) for a in ragged(ctxs))
    sel = torch.tensor(SEL, dtype=torch.int32, device=dev)
    base, table, pref, pad_id = None, None, None, 3
    with torch.no_grad():
        if case == "prefixes":
            entries = []
            for p in (PRE_A, PRE_B):
                out = llm._body(input_ids=torch.tensor([p], device=dev), use_cache=True)
                entries.append((KVPrefix.from_hf_cache(out.past_key_values), tuple(p)))
            table = PrefixTable(entries, dev)
            pref_all = [PREF_OF.get(i, -1) for i in range(len(ctxs))]
            base = torch.tensor([0 if p < 0 else len((PRE_A, PRE_B)[p]) for p in pref_all], dtype=torch.int32, device=dev)
            pref = torch.tensor([pref_all[i] for i in SEL[:N_SEL]], dtype=torch.int32, device=dev)
            l_max = max(len(ctxs[i]) - int(base[i]) for i in SEL[:N_SEL])
        else:
            l_max = max(len(ctxs[i]) for i in SEL[:N_SEL])
        keep = case == "keep_kv"

        enc = encode_ragged(llm, batch, sel, N_SEL, l_max, pad_id=pad_id, base=base,
                            prefixes=None if table is None else (table, pref), keep_kv=keep)

        # the sequence as every call site used to write it
        p_max = table.p_max if table is not None else 0
        ids, am, pos, last = eng.gather_padded(*batch, sel, N_SEL, base, pad_id, p_max, l_max)
        cache = table.cache_for(eng, pref) if table is not None else None
        out = llm._body(input_ids=ids, attention_mask=am, position_ids=pos, past_key_values=cache,
                        use_cache=cache is not None or keep)
        hidden = out.last_hidden_state
        rows = hidden[torch.arange(N_SEL, device=dev), last.long()]

    assert tuple(enc.hidden.shape) == (N_SEL, l_max, 64) and torch.equal(enc.hidden, hidden)
    assert torch.equal(enc.last, last) and torch.equal(enc.last_rows(), rows)
    want_last = [len(ctxs[i]) - (0 if base is None else int(base[i])) - 1 for i in SEL[:N_SEL]]
    assert last.tolist() == want_last  # (the rows ARE the last positions: the duplicate, the prefix-less row included)
    if case == "plain":
        assert enc.out.past_key_values is None  # the body ran without a cache
        return
    want = [(ly.keys.contiguous(), ly.values.contiguous()) for ly in out.past_key_values.layers]
    got = enc.kv_layers()
    assert len(got) == len(want) == 2
    for (gk, gv), (wk, wv) in zip(got, want):
        assert gk.is_contiguous() and gv.is_contiguous()
        assert tuple(gk.shape) == (N_SEL, 2, p_max + l_max, 32)
        assert torch.equal(gk, wk) and torch.equal(gv, wv)


@pytest.fixture(scope="module")
def cpu_llm():
    return _llm(CpuOracleEngine(), "cpu", torch.float32)


@pytest.mark.parametrize("case", CASES)
def test_encode_ragged_is_the_sequence_it_replaced(cpu_llm, case):
    _check(cpu_llm, case)


def test_body_and_head_are_read_at_call_time(cpu_llm):
    """`_lora_rows_logits` swaps `llm._body` for the duration of a call: the encoder must run what is there then."""
    from genlm_backend_amd.kv import encode_ragged, ragged

    batch = tuple(torch.from_numpy(a) for a in ragged(_contexts()))
    seen = []
    was = cpu_llm._body
    try:
        cpu_llm._body = lambda **kw: (seen.append(sorted(kw)), was(**kw))[1]
        with torch.no_grad():
            encode_ragged(cpu_llm, batch, torch.tensor(SEL, dtype=torch.int32), N_SEL, 9)
    finally:
        cpu_llm._body = was
    assert seen == [["attention_mask", "input_ids", "past_key_values", "position_ids", "use_cache"]]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("case", CASES)
def test_encode_ragged_is_the_sequence_it_replaced_gpu(engine, case, dtype):
    _check(_llm(engine, engine.device, dtype), case)
