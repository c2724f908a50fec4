"""The row-packed encoding (kv.encode_packed: every shared prompt's rows once per forward) against kv.encode_ragged on a
random-init 2-layer GPT-2 of width 768, float32, every projection on the split-bf16 kernel on both paths: the same bits in
the last hidden rows and the logits, the same population after a DeviceSIS loop, and the padded path wherever the packed
one does not apply."""
import numpy as np
import pytest
import torch

from genlm_backend_amd.fuse import SplitConv1D
from genlm_backend_amd.kv import PromptGroups, encode_packed, encode_ragged, ragged

pytestmark = pytest.mark.gpu

V, EOS = 512, 0


def _llm(engine, **kw):
    from transformers import GPT2Config

    from genlm_backend_amd.llm import AsyncAmdLM

    cfg = GPT2Config(vocab_size=V, n_positions=64, n_embd=768, n_layer=2, n_head=12, bos_token_id=EOS, eos_token_id=EOS)
    llm = AsyncAmdLM.from_config(cfg, None, device=engine.device, dtype=torch.float32, seed=7, engine=engine, batch_size=64, **kw)
    never_eos = torch.zeros(V)
    never_eos[EOS] = float("-inf")  # (no particle finishes before max_tokens: the population stays whole)
    only_eos = torch.full((V,), float("-inf"))
    only_eos[EOS] = 0.0
    llm.register_masks(torch.stack([never_eos, only_eos]))
    return llm


@pytest.fixture(scope="module")
def llm(engine):
    return _llm(engine)


@pytest.fixture()
def split_everywhere(llm):
    """min_rows = 0: both paths run the split kernel at every row count."""
    mods = [m for m in llm._body.modules() if isinstance(m, SplitConv1D)]
    assert len(mods) == 8, "the shadow's four projections per block are SplitConv1D"
    was = [m.min_rows for m in mods]
    for m in mods:
        m.min_rows = 0
    yield
    for m, r in zip(mods, was):
        m.min_rows = r


def _prompts(G):
    rs = np.random.default_rng(3)
    return [list(range(100, 108))] + [[int(t) for t in rs.integers(1, V, 8)] for _ in range(G - 1)]


@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("U", [4, 37])
def test_encode_packed_matches_ragged(llm, split_everywhere, U, G):
    dev, eng = llm.device, llm.engine
    rs = np.random.default_rng(10 * U + G)
    prompts = _prompts(G)
    grp = [u % G for u in range(U)]
    tails = [1 + (u % 10) for u in range(U)]  # 1 .. 10
    seqs = [prompts[g] + [int(t) for t in rs.integers(1, V, n)] for g, n in zip(grp, tails)]
    batch = tuple(torch.from_numpy(a).to(dev) for a in ragged(seqs))
    sel = torch.arange(U, dtype=torch.int32, device=dev)
    l_max = max(len(s) for s in seqs)
    with torch.no_grad():
        want = encode_ragged(llm, batch, sel, U, l_max).last_rows()
        enc = encode_packed(llm, batch, sel, U, torch.tensor(grp, dtype=torch.int32, device=dev), PromptGroups(prompts, dev),
                            sum(tails), max_keys=l_max)
        got = enc.last_rows()
        assert enc.n_rows == 8 * G + sum(tails)
        assert torch.equal(got, want)
        assert torch.equal(llm._lm_head(got), llm._lm_head(want))
    eng.check()  # no segment was refused


def _loop(llm, prompts, steps, n=64, **kw):
    from genlm_backend_amd.sis import DeviceSIS

    sis = DeviceSIS(llm, n, prompts, 10, EOS, seed=5, **kw)
    for _ in range(steps):
        sis.step()
    return sis


@pytest.mark.parametrize("G", [1, 2])
def test_sis_loop_same_population(llm, split_everywhere, G):
    ps = _prompts(G)
    prompts = ps[0] if G == 1 else [ps[i % G] for i in range(64)]
    on = _loop(llm, prompts, 6, share_prompt_rows=True)
    off = _loop(llm, prompts, 6, share_prompt_rows=False)
    assert on.packed_steps == 5 and off.packed_steps == 0  # (step 0 feeds the bare prompts: no tail yet)
    assert on.last_stats["fwd_tokens"] == 8 * G + on.last_stats["n_unique"] * 5
    for name in ("contexts", "lengths", "active", "log_weights"):
        assert torch.equal(getattr(on, name), getattr(off, name)), name
    llm.engine.check()


def test_sis_loop_resampled(llm, split_everywhere):
    """Two prompts, resampled after every step: the particles' prompt groups follow their ancestors."""
    ps = _prompts(2)
    prompts = [ps[i % 2] for i in range(64)]
    on = _loop(llm, prompts, 5, share_prompt_rows=True, resample_ess=1.0)
    off = _loop(llm, prompts, 5, share_prompt_rows=False, resample_ess=1.0)
    assert on.packed_steps == 4 and on.n_resamples == off.n_resamples > 0
    for name in ("contexts", "lengths", "active", "log_weights"):
        assert torch.equal(getattr(on, name), getattr(off, name)), name


# ---- routing: the padded path wherever the packed one does not apply ---------------------------------------------------------
def test_route_option_off(llm, split_everywhere):
    assert _loop(llm, _prompts(1)[0], 3, share_prompt_rows=False).packed_steps == 0


@pytest.mark.parametrize("kw", [dict(use_prefix_kv=True), dict(use_particle_kv=True), dict(use_particle_kv=True, share_kv=False)],
                         ids=["prefix_kv (cached prefixes)", "shared particle_kv", "private particle_kv"])
def test_route_kv_options(llm, split_everywhere, kw):
    assert _loop(llm, _prompts(1)[0], 3, **kw).packed_steps == 0


def test_route_no_tail_and_finished_particle(llm, split_everywhere):
    sis = _loop(llm, _prompts(1)[0], 1)
    assert sis.packed_steps == 0  # t = 0: the contexts are the prompts
    sis.step()
    assert sis.packed_steps == 1
    sis.active[3] = 0  # a finished particle is a 1-token stub, not prompt + tail
    sis.step()
    assert sis.packed_steps == 1


def test_route_more_than_32_keys(llm, split_everywhere):
    sis = _loop(llm, list(range(1, 31)), 4)  # 30 + t keys: 31 and 32 are served, 33 is not
    assert sis.packed_steps == 2


def test_route_small_batch_keeps_library_gemms(llm):
    """With the dispatch table as shipped, 64 contexts of a dozen tokens stay below the rows from which every projection
    runs the split kernel: the padded path, whose GEMMs they are."""
    assert _loop(llm, _prompts(1)[0], 3).packed_steps == 0


def test_route_foreign_attention(engine):
    other = _llm(engine, glb_attention=False)
    for m in other._body.modules():
        if isinstance(m, SplitConv1D):
            m.min_rows = 0
    assert _loop(other, _prompts(1)[0], 3).packed_steps == 0
