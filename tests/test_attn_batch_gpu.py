"""glb_batch_attention_tile on the MI355X: the MFMA tile kernel for padded batches of long contexts against
torch in float64 under every mask form the path builds, its refusals, and AsyncAmdLM(long_attention=True) end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

from genlm_backend_amd import _lib

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2, torch.float16: 3e-3}  # tests/test_attn_tile_gpu.py's: the same arithmetic and inputs
U = 4


def _masks(dev, Lq, Lk, seed):
    """name -> bool [U or 1, 1, Lq, Lk] (None: causal)."""
    P = Lk - Lq  # keys of a cached prefix in front of the queries' own
    s, t = torch.arange(Lk, device=dev)[None, None, :], torch.arange(Lq, device=dev)[None, :, None]
    causal = s <= t + P
    col = lambda lens: torch.tensor(lens, device=dev)[:, None, None]
    n_tok, n_pre = col([Lq, max(1, Lq // 2), max(1, Lq - 5), 1]), col([P, P // 2, 0, max(0, P - 3)])
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rnd = torch.rand((U, Lq, Lk), device=dev, generator=g) < 0.6
    rnd[1, Lq // 2] = False  # a query that sees nothing
    rnd[2, :64, min(64, Lk - 1):128] = False  # a 64-key stretch hidden from every query of the first block
    rnd[3, :, :40] = False  # ... and the first tiles hidden from every query of a row
    masks = {"null": None,
             "right": causal & (s < P + n_tok) & (t < n_tok),  # padding queries see nothing
             "left": causal & (s >= P + Lq - n_tok) & (t >= Lq - n_tok),
             "hole": causal & ((s < n_pre) | ((s >= P) & (s < P + n_tok))) & (t < n_tok),  # padded prefix, then padded tokens
             "random": rnd,
             "broadcast": causal[:1] & (s[:1] != 3)}
    return {k: (m if m is None else m[:, None].contiguous()) for k, m in masks.items()}


@pytest.mark.parametrize("Lq,Lk", [(1, 70), (65, 65), (33, 160), (130, 130), (96, 257)])
@pytest.mark.parametrize("H,Hkv", [(4, 2), (3, 3)])
@pytest.mark.parametrize("Dh", [64, 128])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_batch_attention_tile_against_float64(engine, dtype, Dh, H, Hkv, Lq, Lk):
    dev = engine.device
    g = torch.Generator(device=dev)
    g.manual_seed(Dh + H + Lq)
    proj = torch.randn((U, Lk, (H + 2 * Hkv) * Dh), device=dev, generator=g).to(dtype)  # q | k | v of one projection
    q = proj[:, Lk - Lq:, :H * Dh].view(U, Lq, H, Dh).transpose(1, 2)
    k = proj[..., H * Dh:(H + Hkv) * Dh].view(U, Lk, Hkv, Dh).transpose(1, 2)
    v = proj[..., (H + Hkv) * Dh:].view(U, Lk, Hkv, Dh).transpose(1, 2)
    before, scale, G = proj.clone(), Dh ** -0.5, H // Hkv
    sc = torch.einsum("uhtd,uhsd->uhts", q.double(), k.double().repeat_interleave(G, dim=1)) * scale
    vf = v.double().repeat_interleave(G, dim=1)
    causal = (torch.arange(Lk, device=dev)[None, :] <= torch.arange(Lq, device=dev)[:, None] + Lk - Lq)[None, None]
    for name, mask in _masks(dev, Lq, Lk, Lq + Lk).items():
        see = (causal if mask is None else mask).expand(U, 1, Lq, Lk)
        seen = see.any(-1)[:, 0]  # [U, Lq]
        w = torch.softmax(sc.masked_fill(~see, float("-inf")), -1).nan_to_num(0.0)
        ref = torch.einsum("uhts,uhsd->uthd", w, vf)
        m_arg = mask.expand(U, 1, Lq, Lk) if name == "broadcast" else mask  # (row stride 0)
        out = engine.batch_attention_tile(q, k, v, m_arg, scale)
        torch.cuda.synchronize()
        assert out.shape == (U, Lq, H, Dh) and out.dtype == dtype
        err = (out.double() - ref)[seen].abs().max().item()
        print(f"{name}: max |batch tile - float64| = {err:.3e} (bound {TOL[dtype]})")
        assert err < TOL[dtype], name
        assert not out[~seen].float().any(), name  # zeros exactly where a query sees nothing
        assert torch.equal(proj, before), name
    # one replay from a captured graph: the bits of the direct call (the last mask)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out2 = engine.batch_attention_tile(q, k, v, m_arg, scale)
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(out2, out)


def test_bad_arguments_are_refused_before_any_launch(engine):
    dev, Lq, Lk, H, Dh = engine.device, 4, 80, 2, 64
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    q, k, v = (torch.randn((2, H, n, Dh), device=dev, generator=g) for n in (Lq, Lk, Lk))
    out = torch.full((2, Lq, H, Dh), 7.0, device=dev)
    i64x3, ptr = C.c_int64 * 3, lambda x: C.c_void_p(x.data_ptr())

    def call(q_ptr=ptr(q), q_strides=q.stride()[:3], q_len=Lq, head_dim=Dh):
        return engine.lib.glb_batch_attention_tile(q_ptr, i64x3(*q_strides), ptr(k), i64x3(*k.stride()[:3]), ptr(v), i64x3(*v.stride()[:3]),
                                                   None, 0, 0, 2, H, H, q_len, Lk, head_dim, Dh ** -0.5, _lib.F32, ptr(out), engine._stream())

    assert call(head_dim=32) == _lib.GLB_EUNSUPPORTED and "head_dim 32 (64 and 128 are built)" in _lib.last_error()
    assert call(q_len=Lk + 1) == _lib.GLB_EINVAL and "q_len 81, k_len 80" in _lib.last_error()
    assert call(q_strides=(q.stride(0), q.stride(1), Dh + 2)) == _lib.GLB_EINVAL and "16-byte aligned" in _lib.last_error()
    assert call(q_ptr=C.c_void_p(q.data_ptr() + 4)) == _lib.GLB_EINVAL
    torch.cuda.synchronize()
    assert (out == 7.0).all()  # nothing was enqueued
    assert call() == _lib.GLB_OK  # ... and the same tensors are served
    ref = torch.nn.functional.scaled_dot_product_attention(q.double(), k.double(), v.double(), attn_mask=torch.ones(
        (Lq, Lk), dtype=torch.bool, device=dev).tril(Lk - Lq)).transpose(1, 2)
    assert (out.double() - ref).abs().max().item() < TOL[torch.float32]


def test_long_attention_backend_matches_the_sdpa_fall_through(engine):
    """A float32 GPT-2 (head_dim 64) behind two backends: with long_attention=True the padded batches of 70 .. 200 tokens run
    the kernel - once per layer per forward - and give the log-probs of the backend that leaves them to SDPA."""
    from transformers import GPT2Config, GPT2LMHeadModel

    from genlm_backend_amd.llm import AsyncAmdLM

    class Tok:
        pad_token_id = None
        eos_token_id = 0

    torch.manual_seed(3)
    V, n_layer = 200, 2
    model = GPT2LMHeadModel(GPT2Config(vocab_size=V, n_positions=384, n_embd=128, n_layer=n_layer, n_head=2, bos_token_id=0,
                                       eos_token_id=0)).eval().to(engine.device)
    calls = []
    inner = engine.batch_attention_tile

    def counted(*args):
        calls.append(tuple(args[0].shape))
        return inner(*args)

    engine.batch_attention_tile = counted
    try:
        def make(**kw):
            m = AsyncAmdLM(model, None, batch_size=64, timeout=0.02, engine=engine, **kw)
            m.tokenizer = Tok()
            return m

        on, off = make(long_attention=True), make(long_attention=False)
        rnd = np.random.default_rng(9)
        ctxs = [[int(t) for t in rnd.integers(1, V, n)] for n in (70, 93, 128, 131, 177, 200)]
        conts = [[int(t) for t in rnd.integers(1, V, 150)] for _ in ctxs]
        want = off.batch_next_token_logprobs_sync(ctxs).float()
        want_s = off.batch_sequence_logprobs_sync(ctxs, conts).token_logprobs
        assert not calls  # never with the flag off
        got = on.batch_next_token_logprobs_sync(ctxs).float()
        assert len(calls) == n_layer, calls  # once per layer per forward
        got_s = on.batch_sequence_logprobs_sync(ctxs, conts).token_logprobs
        assert len(calls) == 2 * n_layer and calls[-1][2] > 200, calls
    finally:
        del engine.batch_attention_tile  # (the instance attribute: the class's method is back)
    err = (got - want).abs().max().item()
    err_s = (got_s - want_s).abs().max().item()
    print(f"long_attention on / off: next-token rows {err:.3e}, sequence log-probs {err_s:.3e} (bound 1e-4)")
    assert err < 1e-4 and err_s < 1e-4
