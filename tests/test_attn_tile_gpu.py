"""glb_slab_attention_tile on the MI355X: the MFMA tile kernel against torch in float64, against the chunk
kernel where both apply, and auto_kv_span end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

from genlm_backend_amd import _lib

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2, torch.float16: 3e-3}  # test_slab_attention_chunk's bounds
CAP = 160


def _inputs(dev, dtype, Dh, H, Hkv, T, n=5, cap=CAP):
    """Slabs, q | k | v views of one projection tensor, and the five rows of the issue: pos = 0 with n_new = T, pos not a
    multiple of the key tile, pos + n_new = cap, n_new = 1 inside a wide forward, n_new = T behind a long prefix."""
    g = torch.Generator(device=dev)
    g.manual_seed(Dh + H + T)
    ks = torch.randn((n, Hkv, cap, Dh), device=dev, generator=g).to(dtype)
    vs = torch.randn((n, Hkv, cap, Dh), device=dev, generator=g).to(dtype)
    half = max(1, T // 2)
    nn = torch.tensor([T, half, half, 1, T], dtype=torch.int32, device=dev)
    pos = torch.tensor([0, 7, cap - half, 45, cap - T - 3], dtype=torch.int32, device=dev)
    proj = torch.randn((n, T, (H + 2 * Hkv) * Dh), device=dev, generator=g).to(dtype)
    q = proj[..., :H * Dh].view(n, T, H, Dh).transpose(1, 2)
    kn = proj[..., H * Dh:(H + Hkv) * Dh].view(n, T, Hkv, Dh).transpose(1, 2)
    vn = proj[..., (H + Hkv) * Dh:].view(n, T, Hkv, Dh).transpose(1, 2)
    return ks, vs, q, kn, vn, pos, nn


def _reference(ks, vs, q, kn, vn, pos, nn, scale):
    """(out float64 [n, T, H, Dh], the slabs after the call, valid [n, T]) from torch in float64 on the same values."""
    n, H, T, _ = q.shape
    cap, dev = ks.shape[2], ks.device
    k_ref, v_ref = ks.clone(), vs.clone()
    for r in range(n):
        p, c = int(pos[r]), int(nn[r])
        k_ref[r, :, p:p + c], v_ref[r, :, p:p + c] = kn[r, :, :c], vn[r, :, :c]
    G = H // ks.shape[1]
    kf, vf = k_ref.double().repeat_interleave(G, dim=1), v_ref.double().repeat_interleave(G, dim=1)
    sc = torch.einsum("rhtd,rhpd->rhtp", q.double(), kf) * scale
    last = pos[:, None] + torch.arange(T, device=dev)[None, :]
    sc = sc.masked_fill(torch.arange(cap, device=dev)[None, None, None, :] > last[:, None, :, None], float("-inf"))
    out = torch.einsum("rhtp,rhpd->rthd", torch.softmax(sc, -1), vf)
    return out, k_ref, v_ref, torch.arange(T, device=dev)[None, :] < nn[:, None]


@pytest.mark.parametrize("T", [17, 32, 33, 64, 128])
@pytest.mark.parametrize("H,Hkv", [(4, 2), (3, 3)])
@pytest.mark.parametrize("Dh", [64, 128])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_slab_attention_tile_against_float64(engine, dtype, Dh, H, Hkv, T):
    dev, n = engine.device, 5
    ks, vs, q, kn, vn, pos, nn = _inputs(dev, dtype, Dh, H, Hkv, T)
    scale = Dh ** -0.5
    ref, k_ref, v_ref, valid = _reference(ks, vs, q, kn, vn, pos, nn, scale)
    k2, v2 = ks.clone(), vs.clone()
    out = engine.slab_attention_tile(q, kn, vn, k2, v2, pos, nn, scale)
    torch.cuda.synchronize()
    assert out.shape == (n, T, H, Dh) and out.dtype == dtype
    err = (out.double() - ref)[valid].abs().max().item()
    print(f"max |tile - float64| = {err:.3e} (bound {TOL[dtype]})")
    assert err < TOL[dtype]
    assert not out[~valid].float().any()  # zeros behind a row's last token
    assert torch.equal(k2, k_ref) and torch.equal(v2, v_ref)  # exactly the new positions replaced
    # a chunk outside its row: NaN there, nothing appended, the other rows bit-equal
    bad = pos.clone()
    bad[1], bad[2] = -1, CAP - int(nn[2]) + 1
    k3, v3 = ks.clone(), vs.clone()
    out3 = engine.slab_attention_tile(q, kn, vn, k3, v3, bad, nn, scale)
    torch.cuda.synchronize()
    assert torch.isnan(out3[[1, 2]].float()).all() and torch.equal(out3[[0, 3, 4]], out[[0, 3, 4]])
    assert torch.equal(k3[[1, 2]], ks[[1, 2]]) and torch.equal(v3[[1, 2]], vs[[1, 2]])
    assert torch.equal(k3[[0, 3, 4]], k2[[0, 3, 4]]) and torch.equal(v3[[0, 3, 4]], v2[[0, 3, 4]])
    # rows anywhere in a larger slab: the same bits in the rows named, nothing else touched
    big_k, big_v = (torch.zeros((n + 3, Hkv, CAP, Dh), dtype=dtype, device=dev) for _ in range(2))
    rows = torch.tensor([6, 0, 3, 7, 2], dtype=torch.int32, device=dev)
    big_k[rows.long()], big_v[rows.long()] = ks, vs
    out4 = engine.slab_attention_tile(q, kn, vn, big_k, big_v, pos, nn, scale, rows=rows)
    assert torch.equal(out4, out) and torch.equal(big_k[rows.long()], k2) and torch.equal(big_v[rows.long()], v2)
    assert not big_k[[1, 4, 5]].any() and not big_v[[1, 4, 5]].any()
    # one replay from a captured graph: the same bits
    k5, v5 = ks.clone(), vs.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        engine.slab_attention_tile(q, kn, vn, k5.clone(), v5.clone(), pos, nn, scale)  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out5 = engine.slab_attention_tile(q, kn, vn, k5, v5, pos, nn, scale)
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(out5, out) and torch.equal(k5, k2) and torch.equal(v5, v2)


@pytest.mark.parametrize("T", [1, 16])
@pytest.mark.parametrize("H,Hkv", [(4, 2), (3, 3)])
@pytest.mark.parametrize("dtype,Dh", [(torch.float32, 64), (torch.bfloat16, 128), (torch.float16, 64)])
def test_small_chunks_agree_with_the_chunk_kernel(engine, dtype, Dh, H, Hkv, T):
    ks, vs, q, kn, vn, pos, nn = _inputs(engine.device, dtype, Dh, H, Hkv, T)
    k1, v1, k2, v2 = ks.clone(), vs.clone(), ks.clone(), vs.clone()
    want = engine.slab_attention_chunk(q, kn, vn, k1, v1, pos, nn, Dh ** -0.5)
    out = engine.slab_attention_tile(q, kn, vn, k2, v2, pos, nn, Dh ** -0.5)
    torch.cuda.synchronize()
    err = (out.float() - want.float()).abs().max().item()
    print(f"max |tile - chunk| = {err:.3e} (bound {TOL[dtype]})")
    assert err < TOL[dtype] and torch.equal(k1, k2) and torch.equal(v1, v2)


def test_span_rows_match_a_backend_without_rows(engine):
    """Contexts that grow by 20 to 40 tokens per call, shrink and fork: a backend with auto_kv_span = 48 gives the log-prob
    rows of a backend that re-encodes (the chunk end-to-end test's bound), and feeds rows more than 16 tokens."""
    from transformers import GPT2Config, GPT2LMHeadModel

    from genlm_backend_amd.kv import ragged
    from genlm_backend_amd.llm import AsyncAmdLM

    class Tok:
        pad_token_id = None
        eos_token_id = 0

    torch.manual_seed(3)
    V = 200
    model = GPT2LMHeadModel(GPT2Config(vocab_size=V, n_positions=160, n_embd=128, n_layer=2, n_head=2, bos_token_id=0,
                                       eos_token_id=0)).eval().to(engine.device)  # head_dim 64: the tile kernel's

    def make(**kw):
        m = AsyncAmdLM(model, None, batch_size=64, timeout=0.02, engine=engine, **kw)
        m.tokenizer = Tok()
        return m

    plain, span = make(), make(auto_kv_rows=8, auto_kv_cap=160, auto_kv_span=48)
    fwd = span._auto_kv.kv
    rnd = np.random.default_rng(5)
    new = lambda k: [int(t) for t in rnd.integers(1, V, k)]
    ctxs = [new(int(rnd.integers(3, 9))) for _ in range(4)]
    for call in range(4):
        if call:
            grown = [c + new(int(rnd.integers(20, 41))) for c in ctxs[:2]]
            ctxs = grown + [ctxs[2][:-2] + new(22), ctxs[0][:len(ctxs[0]) - 1] + new(25)]  # two grow, one shrinks and grows, one forks
        rows_p = np.stack([plain.next_token_logprobs_uncached(c).float().cpu().numpy() for c in ctxs])
        tok_d, st_d, ln_d = (torch.from_numpy(a).to(engine.device) for a in ragged(ctxs))
        g_of, rep, ng = engine.group_contexts(tok_d, st_d, ln_d)
        logits, row_of_group, _, _, _ = span._auto_kv.logits(tok_d, st_d, ln_d, g_of, rep, ng)
        rows_s = torch.log_softmax(logits.float(), -1)[row_of_group[g_of.long()].long()].cpu().numpy()
        assert np.abs(rows_s - rows_p).max() < 1e-4, call
        if call:
            plan, counts, (n_chunk, t_max) = span._auto_kv.last
            assert n_chunk == 4 and plan["n_new_a"][counts[1] - n_chunk:counts[1]].min().item() > 16  # cannot pass without the span
            assert fwd._chunk_fused(t_max)  # the tile kernel served it, not the SDPA fall-through
    st = span._auto_kv.stats
    print("auto_kv_span=48 stats:", st)
    assert st["chunk_rows"] == 12 and st["chunk_tokens"] >= 20 * 12 and st["encoded_rows"] == 4


@pytest.fixture(scope="module")
def tiny(engine):
    """The smallest valid call of the two chunk-shaped entries, as their C arguments by name (float32, two forward rows over
    rows 2 and 0 of a three-row slab), and the tensors behind them."""
    dev, n, R, H, Hkv, cap, Dh, T = engine.device, 2, 3, 2, 1, 8, 64, 2
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    t = {name: torch.randn(shape, device=dev, generator=g) for name, shape in
         (("k_slab", (R, Hkv, cap, Dh)), ("v_slab", (R, Hkv, cap, Dh)), ("q", (n, H, T, Dh)), ("k_new", (n, Hkv, T, Dh)),
          ("v_new", (n, Hkv, T, Dh)))}
    t["pos"] = torch.tensor([3, 0], dtype=torch.int32, device=dev)
    t["n_new"] = torch.tensor([2, 1], dtype=torch.int32, device=dev)
    t["row_of"] = torch.tensor([2, 0], dtype=torch.int32, device=dev)
    t["out"] = torch.full((n, T, H, Dh), 7.0, device=dev)
    args = {name: C.c_void_p(x.data_ptr()) for name, x in t.items()}
    for name in ("q", "k_new", "v_new"):
        args[name[0] + "_strides"] = (C.c_int64 * 3)(*t[name].stride()[:3])
    args.update(n_rows=n, n_slab_rows=R, heads=H, kv_heads=Hkv, cap=cap, head_dim=Dh, max_new=T, scale=Dh ** -0.5, dtype=_lib.F32,
                stream=engine._stream())
    return args, t


_ARG_ORDER = ("q", "q_strides", "k_new", "k_strides", "v_new", "v_strides", "k_slab", "v_slab", "pos", "n_new", "row_of", "n_rows",
              "n_slab_rows", "heads", "kv_heads", "cap", "head_dim", "max_new", "scale", "dtype", "out", "stream")


@pytest.mark.parametrize("entry,limit,built", [("glb_slab_attention_chunk", _lib.KV_CHUNK_MAX, "16, 32, 64 and 128"),
                                               ("glb_slab_attention_tile", _lib.KV_TILE_MAX, "64 and 128")], ids=["chunk", "tile"])
def test_bad_arguments_are_refused_before_any_launch(engine, tiny, entry, limit, built):
    args, t = tiny
    call = lambda **change: getattr(engine.lib, entry)(*({**args, **change}[name] for name in _ARG_ORDER))
    before = {name: x.clone() for name, x in t.items()}
    cases = [(dict(dtype=7), _lib.GLB_EINVAL, "bad dtype 7"),  # (the one message without the entry's name)
             (dict(max_new=0), _lib.GLB_EINVAL, f"{entry}: 0 query positions per row (1 .. {limit})"),
             (dict(max_new=limit + 1), _lib.GLB_EINVAL, f"{entry}: {limit + 1} query positions per row (1 .. {limit})"),
             (dict(kv_heads=3), _lib.GLB_EINVAL, f"{entry}: bad sizes"),  # heads = 2 is no multiple of it
             (dict(head_dim=48), _lib.GLB_EUNSUPPORTED, f"{entry}: head_dim 48 ({built} are built)"),
             (dict(q=C.c_void_p(t["q"].data_ptr() + 4)), _lib.GLB_EINVAL, f"{entry}: pointers and strides must be 16-byte aligned"),
             (dict(q_strides=(C.c_int64 * 3)(t["q"].stride(0), t["q"].stride(1), 3)), _lib.GLB_EINVAL,
              f"{entry}: pointers and strides must be 16-byte aligned"),
             (dict(pos=None), _lib.GLB_EINVAL, f"{entry}: null pointer")]
    if entry == "glb_slab_attention_tile":
        cases.append((dict(head_dim=32), _lib.GLB_EUNSUPPORTED, f"{entry}: head_dim 32 ({built} are built)"))
    for change, code, message in cases:
        assert call(**change) == code != 0 and _lib.last_error() == message, (change, _lib.last_error())
    torch.cuda.synchronize()
    for name, x in t.items():  # nothing was enqueued: the output keeps its fill, the slabs their values
        assert torch.equal(x, before[name]), name
    # ... and the same tensors, unchanged, are served: torch's SDPA in float64 on the rows after the append
    assert call() == _lib.GLB_OK
    torch.cuda.synchronize()
    rows, pos, nn, T, cap = t["row_of"].long(), t["pos"], t["n_new"], t["q"].shape[2], t["k_slab"].shape[2]
    k_ref, v_ref = before["k_slab"].clone(), before["v_slab"].clone()
    for r in range(2):
        p, c = int(pos[r]), int(nn[r])
        k_ref[rows[r], :, p:p + c], v_ref[rows[r], :, p:p + c] = t["k_new"][r, :, :c], t["v_new"][r, :, :c]
    assert torch.equal(t["k_slab"], k_ref) and torch.equal(t["v_slab"], v_ref)
    last = pos[:, None] + torch.arange(T, device=pos.device)[None, :]
    see = (torch.arange(cap, device=pos.device)[None, None, None, :] <= last[:, None, :, None])
    G = t["q"].shape[1] // k_ref.shape[1]
    ref = torch.nn.functional.scaled_dot_product_attention(
        t["q"].double(), k_ref[rows].double().repeat_interleave(G, dim=1), v_ref[rows].double().repeat_interleave(G, dim=1),
        attn_mask=see, scale=args["scale"]).transpose(1, 2)
    valid = torch.arange(T, device=pos.device)[None, :] < nn[:, None]
    err = (t["out"].double() - ref)[valid].abs().max().item()
    print(f"{entry}: max |out - float64| = {err:.3e} (bound {TOL[torch.float32]})")
    assert err < TOL[torch.float32] and not t["out"][~valid].any()
    t["k_slab"].copy_(before["k_slab"]), t["v_slab"].copy_(before["v_slab"]), t["out"].copy_(before["out"])  # (for the other entry)
