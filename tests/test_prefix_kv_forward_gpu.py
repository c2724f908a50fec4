"""KV rows behind prompts stored once (SlabKV.set_prefix, DeviceSIS(share_prompt_kv=True)) on the MI355X: the
same function as rows that hold the prompt, other rounding."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V = 200
PROMPTS = [[int(t) for t in np.random.default_rng(7).integers(1, V, k)] for k in (5, 37)]  # 37: past one key tile


def _llm(engine, n_embd=128):
    from transformers import GPT2Config, GPT2LMHeadModel

    from genlm_backend_amd.llm import AsyncAmdLM

    torch.manual_seed(3)
    model = GPT2LMHeadModel(GPT2Config(vocab_size=V, n_positions=96, n_embd=n_embd, n_layer=2, n_head=2, bos_token_id=0,
                                       eos_token_id=0)).eval().to(engine.device)  # head_dim 64 (32 with n_embd = 64)
    llm = AsyncAmdLM(model, None, batch_size=64, timeout=0.02, engine=engine)
    masks = torch.zeros(2, V)
    masks[0, ::3] = masks[0, 7:40] = float("-inf")  # uneven allowed mass across contexts: uneven weights, real resampling
    masks[1, 1:] = float("-inf")
    llm.register_masks(masks)
    return llm


@pytest.fixture(scope="module")
def llm(engine):
    return _llm(engine)


def test_forward_over_a_prefix_equals_forward_over_whole_rows(engine, llm):
    from genlm_backend_amd.kv import SlabForward, SlabKV, encode_ragged, ragged

    dev, n, tail = engine.device, 6, 8
    batch = tuple(torch.from_numpy(a).to(dev) for a in ragged(PROMPTS))
    plen = batch[2].to(torch.int32)
    l_max = int(plen.max())
    layers = encode_ragged(llm, batch, torch.arange(2, dtype=torch.int32, device=dev), 2, l_max, keep_kv=True).kv_layers()
    prefix_of = torch.tensor([0, 1, 1, 0, 1, 0], dtype=torch.int32, device=dev)
    behind, whole = SlabKV(engine, n, tail, len(layers)), SlabKV(engine, n, l_max + tail, len(layers))
    behind.set_prefix(layers, plen, prefix_of)
    whole.fill_rows(layers, prefix_of, plen[prefix_of.long()])
    assert behind.layers[0].keys.shape[2] == tail and behind.nbytes() < whole.nbytes()
    f_behind, f_whole = SlabForward(behind, llm._body), SlabForward(whole, llm._body)
    assert f_behind.fused and f_whole.fused
    rnd = np.random.default_rng(1)
    for t in range(4):  # calls 3 and 4 are replays of a captured graph
        ids = torch.from_numpy(rnd.integers(1, V, (n, 1))).to(dev)
        pos = torch.full((n,), t, dtype=torch.int32, device=dev)
        a = f_behind(ids, pos).clone()
        b = f_whole(ids, pos + plen[prefix_of.long()]).clone()
        err = (a - b).abs().max().item()
        print(f"call {t + 1}: max |hidden behind a prefix - hidden over whole rows| = {err:.3e}")
        assert err < 1e-4, t
    assert len(f_behind.graphs) == 1 and len(f_whole.graphs) == 1


@pytest.mark.parametrize("resample_ess", [0.5, 1.0])  # when the weights call for it; after every step
def test_device_sis_is_the_same_run_with_the_prompt_stored_once(engine, llm, resample_ess):
    from genlm_backend_amd.sis import DeviceSIS

    prompts = [PROMPTS[i % 2] for i in range(32)]
    runs = []
    for share in (True, False):
        sis = DeviceSIS(llm, 32, prompts, 6, 0, use_particle_kv=True, share_kv=False, share_prompt_kv=share, resample_ess=resample_ess,
                        seed=0)
        sis.run()
        runs.append(sis)
    a, b = runs
    assert torch.equal(a.contexts, b.contexts) and torch.equal(a.lengths, b.lengths)
    err = (a.log_weights - b.log_weights).abs().max().item()
    print(f"max |log-weight| difference = {err:.3e}, resampling steps {a.n_resamples}, KV bytes {a.pkv.nbytes()} against {b.pkv.nbytes()}")
    assert err < 1e-4 and a.n_resamples == b.n_resamples and (resample_ess < 1.0 or a.n_resamples >= 2)
    assert a.pkv.cap == 7 and a.pkv.nbytes() < b.pkv.nbytes()


def test_the_option_is_refused_where_it_cannot_serve(engine, llm):
    from genlm_backend_amd.sis import DeviceSIS

    with pytest.raises(ValueError, match="share_kv=False"):
        DeviceSIS(llm, 2, PROMPTS, 4, 0, use_particle_kv=True, share_kv=True, share_prompt_kv=True)
    with pytest.raises(ValueError, match="head_dim 32"):
        DeviceSIS(_llm(engine, n_embd=64), 2, PROMPTS, 4, 0, use_particle_kv=True, share_kv=False, share_prompt_kv=True)
