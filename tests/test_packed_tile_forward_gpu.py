"""The row-packed encoding past 32 keys (kv.encode_packed(tile=True), DeviceSIS(share_prompt_rows="tile")) on
tiny random 2-layer models of head_dim 64: against kv.encode_ragged, and a DeviceSIS loop against the unpacked loop."""
import copy

import numpy as np
import pytest
import torch

from genlm_backend_amd.fuse import SplitConv1D
from genlm_backend_amd.kv import PromptGroups, encode_packed, encode_ragged, ragged

pytestmark = pytest.mark.gpu

V, EOS, ONLY = 512, 0, 5


def _make(engine, kind, dtype):
    from transformers import GPT2Config, LlamaConfig

    from genlm_backend_amd.llm import AsyncAmdLM

    if kind == "gpt2":  # width 768: the shadow's projections are SplitConv1D, as DeviceSIS's packed path wants them
        cfg = GPT2Config(vocab_size=V, n_positions=128, n_embd=768, n_layer=2, n_head=12, bos_token_id=EOS, eos_token_id=EOS)
    else:
        cfg = LlamaConfig(vocab_size=V, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                          num_key_value_heads=2, head_dim=64, max_position_embeddings=128, bos_token_id=EOS, eos_token_id=EOS)
    return AsyncAmdLM.from_config(cfg, None, device=engine.device, dtype=dtype, seed=7, engine=engine, batch_size=64)


def _both(llm, batch, sel, U, l_max, grp=None, groups=None, n_tail=0):
    """(last rows, log-probs of the head) of encode_ragged, or of encode_packed(tile=True) when `groups` is given."""
    with torch.no_grad():
        if groups is None:
            rows = encode_ragged(llm, batch, sel, U, l_max).last_rows()
        else:
            enc = encode_packed(llm, batch, sel, U, grp, groups, n_tail, max_keys=l_max, tile=True)
            rows = enc.last_rows()
        return rows.float(), torch.log_softmax(llm._lm_head(rows).float(), -1)


@pytest.mark.parametrize("kind,dtype", [("gpt2", torch.float32), ("llama", torch.bfloat16)])
def test_encode_packed_tile_matches_ragged(engine, kind, dtype):
    llm, dev = _make(engine, kind, dtype), engine.device
    rs = np.random.default_rng(4)
    prompts = [[int(t) for t in rs.integers(1, V, n)] for n in (40, 70)]
    grp, tails = [0, 1, 0, 1, 0, 1], [1, 2, 3, 4, 5, 3]
    seqs = [prompts[g] + [int(t) for t in rs.integers(1, V, n)] for g, n in zip(grp, tails)]
    batch = tuple(torch.from_numpy(a).to(dev) for a in ragged(seqs))
    U, l_max = len(seqs), max(len(s) for s in seqs)
    sel = torch.arange(U, dtype=torch.int32, device=dev)
    want = _both(llm, batch, sel, U, l_max)
    bound = 1e-4  # float32: the bound of §35's end-to-end test for the same comparison
    if dtype != torch.float32:  # bfloat16: twice what the padded path itself is off a float32 copy of the model
        from genlm_backend_amd.llm import AsyncAmdLM

        exact = _both(AsyncAmdLM(copy.deepcopy(llm.model).float(), None, batch_size=64, engine=engine), batch, sel, U, l_max)
        bound = 2 * max((w - e).abs().max().item() for w, e in zip(want, exact))
    calls = []
    inner = engine.packed_attention_tile
    engine.packed_attention_tile = lambda *a, **k: calls.append(1) or inner(*a, **k)
    try:
        got = _both(llm, batch, sel, U, l_max, torch.tensor(grp, dtype=torch.int32, device=dev), PromptGroups(prompts, dev), sum(tails))
    finally:
        del engine.packed_attention_tile
    engine.check()  # no segment was refused
    assert len(calls) == llm._body.config.num_hidden_layers  # pkv.served == n_layers, every layer on the tile kernel
    errs = [(g - w).abs().max().item() for g, w in zip(got, want)]
    print(f"{kind} {dtype}: packed tile vs ragged, last rows {errs[0]:.3e}, log-probs {errs[1]:.3e} (bound {bound:.3e})")
    assert max(errs) < bound


def test_device_sis_tile_mode(engine):
    from genlm_backend_amd.sis import DeviceSIS

    llm = _make(engine, "gpt2", torch.float32)
    one = torch.full((V,), float("-inf"))
    one[ONLY] = 0.0  # exactly one token may be drawn: every run draws the same tokens whatever the logits' last bits
    only_eos = torch.full((V,), float("-inf"))
    only_eos[EOS] = 0.0
    llm.register_masks(torch.stack([one, only_eos]))
    for m in llm._body.modules():
        if isinstance(m, SplitConv1D):
            m.min_rows = 0  # the packed path's row threshold is reachable at 16 particles
    prompt = [int(t) for t in np.random.default_rng(6).integers(1, V, 40)]

    def loop(mode):
        sis = DeviceSIS(llm, 16, prompt, 4, EOS, seed=5, share_prompt_rows=mode)
        for _ in range(4):
            sis.step()
        return sis

    tile, off, short = loop("tile"), loop(False), loop(True)
    assert tile.packed_steps == 3 and off.packed_steps == 0  # (step 0 feeds the bare prompt: no tail yet)
    assert short.packed_steps == 0  # 41 .. 43 keys: the short packed kernel's path is as it was
    assert torch.equal(tile.contexts, off.contexts) and torch.equal(tile.lengths, off.lengths)
    err = (tile.log_weights - off.log_weights).abs().max().item()
    print(f"DeviceSIS tile vs unpacked: log-weights differ by {err:.3e} after 4 steps (bound 4e-4)")
    assert err < 4 * 1e-4
    llm.engine.check()
    with pytest.raises(ValueError):
        DeviceSIS(llm, 16, prompt, 4, EOS, share_prompt_rows="tiles")
