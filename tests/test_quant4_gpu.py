"""4-bit NF4 / FP4 weights on the GPU: glb_w4_quantize / glb_w4_dequantize bit for bit against tests/quant4_engine.py,
glb_w4_gemm against float64 on the dequantised weights (errors within 2x those of F.linear in the same 16-bit dtype on the
same operands - the rule of tests/test_split_gemm_gpu.py for a GEMM that sums in another order than the library's), and
quantised backends end to end against a float32 model that holds the dequantised weights.

Measured on an MI355X (this file's own output): the fused GEMM's max and Frobenius errors equal the library's to the
printed digits on every case; end to end the quantised backend's errors over the yardstick's (bound 2) are 1.00 / 1.00 on the
re-encoding path and 0.98-1.04 on the auto_kv path, both GEMM paths, both models.  The file adds 17 s to the gpu run."""
import numpy as np
import pytest
import torch

from tests import quant4_engine as Q

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
NP_DT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
BODY = [(2304, 768), (768, 3072), (2048, 2048), (512, 2048), (8192, 2048), (2048, 8192)]  # GPT-2 small, Llama-3.2-1B
SMALL = [(1, 64), (17, 64), (33, 192), (48, 128)]


def _bits(t):
    return t.contiguous().view(NP_DT[t.dtype])


def _guarded(rows, cols, pad, dtype, fill=7.0):
    ld = cols + pad
    buf = torch.full((GUARD + rows * ld + GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + rows * ld].view(rows, ld)[:, :cols], ld


def _guards_ok(buf, rows, cols, ld, fill=7.0):
    host = buf.cpu().float()
    ok = bool((host[:GUARD] == fill).all() and (host[GUARD + rows * ld:] == fill).all())
    if ld > cols:
        ok = ok and bool((host[GUARD:GUARD + rows * ld].view(rows, ld)[:, cols:] == fill).all())
    return ok


def _quantize_guarded(engine, w, cb, transposed):
    n, k = (w.shape[1], w.shape[0]) if transposed else w.shape
    nbytes = engine.w4_bytes(n, k)
    assert nbytes == n * k // 2 + 4 * (n * k // 64)
    ibuf = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    img = ibuf[GUARD:GUARD + nbytes]
    assert engine.w4_quantize(w, cb, transposed=transposed, out=img) is img
    torch.cuda.synchronize()
    assert bool((ibuf[:GUARD] == 0xA5).all() and (ibuf[GUARD + nbytes:] == 0xA5).all())
    return img


def _roundtrip_check(engine, w_host, src_dtype, name, transposed, pad, out_dtypes=(torch.float32, torch.bfloat16, torch.float16)):
    """w_host: float32 [n, k] values (rounded to src_dtype here).  Quantise on the device from a padded source, dequantise
    into padded, guarded outputs of every dtype, both layouts; everything bit for bit the restatement's."""
    cb = Q.codebook(name)
    w_src = w_host.to(src_dtype)
    n, k = w_src.shape
    codes, absmax = Q.quantize(w_src.float().numpy(), cb)
    lay = w_src.T.contiguous() if transposed else w_src
    rows, cols = lay.shape
    sbuf, src, _ = _guarded(rows, cols, pad, src_dtype)
    src.copy_(lay.to(DEV))
    img = _quantize_guarded(engine, src, tuple(cb), transposed)
    for od in out_dtypes:
        want = Q.dequantize(codes, absmax, cb, od)
        for tr in (False, True):
            orow, ocol = (k, n) if tr else (n, k)
            obuf, out, ld = _guarded(orow, ocol, pad, od)
            engine.w4_dequantize(img, n, k, tuple(cb), transposed=tr, out=out)
            torch.cuda.synchronize()
            got = out.cpu()
            exp = want.T if tr else want
            assert torch.equal(_bits(got), _bits(exp.contiguous())), (n, k, src_dtype, name, transposed, od, tr)
            assert _guards_ok(obuf, orow, ocol, ld)


@pytest.mark.parametrize("name", ["nf4", "fp4"])
@pytest.mark.parametrize("src_dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("transposed", [False, True])
def test_quantize_dequantize_bit_exact(engine, name, src_dtype, transposed):
    g = torch.Generator().manual_seed(17 + src_dtype.itemsize + 2 * int(transposed))
    for i, (n, k) in enumerate(SMALL + BODY[:4]):
        w = torch.randn(n, k, generator=g) * float(np.exp(np.random.default_rng(i).uniform(-3, 1)))
        _roundtrip_check(engine, w, src_dtype, name, transposed, pad=0 if i % 2 else 8)


@pytest.mark.parametrize("n,k", BODY[4:])
def test_quantize_dequantize_bit_exact_wide_shapes(engine, n, k):
    g = torch.Generator().manual_seed(n + k)
    w = torch.randn(n, k, generator=g) * 0.02
    _roundtrip_check(engine, w, torch.bfloat16, "nf4", False, pad=0, out_dtypes=(torch.bfloat16,))
    _roundtrip_check(engine, w[:, :1024], torch.float32, "fp4", True, pad=16, out_dtypes=(torch.float16,))


@pytest.mark.parametrize("name", ["nf4", "fp4"])
@pytest.mark.parametrize("src_dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_zero_subnormal_and_largest_blocks(engine, name, src_dtype):
    g = torch.Generator().manual_seed(3)
    w = torch.randn(20, 256, generator=g)
    w[0] = 0.0                      # all-zero blocks
    w[1, 64:128] = 0.0
    w[2] = 0.0
    w[2, 70] = -0.3                 # one non-zero element
    tiny = {torch.float32: 1e-41, torch.bfloat16: 1e-39, torch.float16: 3e-6}[src_dtype]  # subnormal in the dtype
    w[3] = torch.randn(256, generator=g) * tiny
    w[4, :64] = torch.randn(64, generator=g) * 1e-43  # float32 subnormals a few ulps apart (zero in the 16-bit sources)
    big = torch.finfo(src_dtype).max
    w[5] = torch.randn(256, generator=g).clamp(-1, 1) * big * 0.5
    w[5, 3], w[5, 130] = big, -big  # absmax = the dtype's largest finite value
    if src_dtype == torch.float32:
        assert (w[3].abs() < torch.finfo(torch.float32).tiny).all() and (w[3] != 0).any()
    for transposed in (False, True):
        _roundtrip_check(engine, w, src_dtype, name, transposed, pad=8)
    # float32 subnormal blocks are not flushed: the device's image dequantises to non-zero values
    if src_dtype == torch.float32:
        cb = tuple(Q.codebook(name))
        img = engine.w4_quantize(w.to(DEV), cb)
        back = engine.w4_dequantize(img, 20, 256, cb).cpu()
        assert (back[3] != 0).any() and (back[4, :64] != 0).any() and torch.isfinite(back).all()
        assert back[5].abs().max() == big


# ---- the fused GEMM ---------------------------------------------------------------------------------------------------------
def _errors(y, ref):
    d = y.double().cpu() - ref
    return d.abs().max().item(), (d.norm() / ref.norm()).item()


@pytest.mark.parametrize("n,k", [(2048, 2048), (512, 2048), (8192, 2048), (2048, 8192), (2304, 768), (768, 3072)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_w4_gemm_against_float64(engine, n, k, dtype):
    m_max = engine.w4_gemm_max_rows()
    g = torch.Generator().manual_seed(n + 3 * k + dtype.itemsize)
    name = "nf4" if (n + k) % 1024 == 0 else "fp4"
    cb = tuple(Q.codebook(name))
    w = (torch.randn(n, k, generator=g) * 0.02).to(dtype).to(DEV)
    img = engine.w4_quantize(w, cb)
    wq = engine.w4_dequantize(img, n, k, cb, dtype=dtype)  # W' in the 16-bit dtype: what the kernel multiplies by
    w64 = wq.double().cpu()
    ratios = []
    for m in sorted({1, 2, 7, 16, 17, 33, m_max}):
        for use_bias in (True, False):
            x = (torch.randn(m, k, generator=g) * 2.0 + 0.1).to(dtype)
            b = (torch.randn(n, generator=g) * 0.05).to(dtype)
            ref = x.double() @ w64.T + (b.double() if use_bias else 0.0)
            # strided X rows (a pitch of k + 8 elements keeps the 16-byte alignment) and a guarded, padded Y
            xbuf, xd, _ = _guarded(m, k, 8, dtype)
            xd.copy_(x.to(DEV))
            bd = b.to(DEV) if use_bias else None
            ybuf, yd, ld = _guarded(m, n, 8, dtype)
            got = engine.w4_gemm(xd, img, n, cb, bd, out=yd)
            assert got is not None, (m, n, k)
            lib = torch.nn.functional.linear(xd.contiguous(), wq, bd)
            torch.cuda.synchronize()
            assert _guards_ok(ybuf, m, n, ld) and _guards_ok(xbuf, m, k, k + 8)
            e_max, e_fro = _errors(yd, ref)
            l_max, l_fro = _errors(lib, ref)
            print(f"w4_gemm {n}x{k} {dtype} m={m} bias={use_bias}: max {e_max:.3e} (lib {l_max:.3e}) fro {e_fro:.3e} "
                  f"(lib {l_fro:.3e})")
            ratios.append((m, use_bias, e_max, l_max, e_fro, l_fro))
            # determinism: a second call gives the same bits (the K split has a fixed combine order)
            y2 = engine.w4_gemm(xd, img, n, cb, bd)
            assert torch.equal(_bits(y2), _bits(yd.contiguous()))
    for m, use_bias, e_max, l_max, e_fro, l_fro in ratios:
        assert e_max <= 2 * l_max + 1e-30 and e_fro <= 2 * l_fro + 1e-30, (m, use_bias, e_max, l_max, e_fro, l_fro)
    # beyond M_max: "unsupported" (the caller dequantises)
    x = torch.zeros(m_max + 1, k, dtype=dtype, device=DEV)
    assert engine.w4_gemm(x, img, n, cb) is None


def test_w4_gemm_unsupported_calls(engine):
    import ctypes as C

    from genlm_backend_amd import _lib

    cb = tuple(Q.codebook("nf4"))
    w = torch.randn(24, 128, device=DEV, dtype=torch.bfloat16)
    img = engine.w4_quantize(w, cb)
    x = torch.randn(4, 128, device=DEV, dtype=torch.bfloat16)
    assert engine.w4_gemm(x, img, 24, cb) is None  # n % 16 != 0
    assert engine.w4_gemm(x.float(), img, 24, cb) is None  # float32 activations
    w = torch.randn(32, 128, device=DEV, dtype=torch.bfloat16)
    img = engine.w4_quantize(w, cb)
    xs = torch.randn(4, 136, device=DEV, dtype=torch.bfloat16)[:, 4:132]  # rows not 16-byte aligned
    assert engine.w4_gemm(xs, img, 32, cb) is None
    assert engine.w4_gemm(x, img, 32, cb) is not None
    # through the C entry point: M_max + 1 rows is GLB_EUNSUPPORTED, not an error
    mx = engine.w4_gemm_max_rows()
    xb = torch.zeros(mx + 1, 128, device=DEV, dtype=torch.bfloat16)
    yb = torch.zeros(mx + 1, 32, device=DEV, dtype=torch.bfloat16)
    ws = torch.zeros(1 << 20, device=DEV, dtype=torch.uint8)
    a = _lib.W4GemmArgs()
    a.struct_size = C.sizeof(_lib.W4GemmArgs)
    a.dtype, a.m, a.n, a.k = _lib.BF16, mx + 1, 32, 128
    a.x, a.ldx, a.image, a.y, a.ldy = xb.data_ptr(), 128, img.data_ptr(), yb.data_ptr(), 32
    a.codebook = (C.c_float * 16)(*cb)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    assert engine.lib.glb_w4_gemm(C.byref(a), engine._stream()) == _lib.GLB_EUNSUPPORTED
    a.m = mx
    assert engine.lib.glb_w4_gemm(C.byref(a), engine._stream()) == _lib.GLB_OK
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_w4_gemm_graph_replay_gives_the_eager_bits(engine, dtype):
    n, k, m = 2048, 8192, 17  # (a shape whose K is split over workgroups)
    cb = tuple(Q.codebook("nf4"))
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(n, k, generator=g) * 0.02).to(dtype).to(DEV)
    x = torch.randn(m, k, generator=g).to(dtype).to(DEV)
    b = torch.randn(n, generator=g).to(dtype).to(DEV)
    img = engine.w4_quantize(w, cb)
    eager = engine.w4_gemm(x, img, n, cb, b).clone()
    out = torch.empty(m, n, device=DEV, dtype=dtype)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        engine.w4_gemm(x, img, n, cb, b, out=out)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    out.zero_()
    with torch.cuda.graph(graph):
        engine.w4_gemm(x, img, n, cb, b, out=out)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(eager))


# ---- end to end -------------------------------------------------------------------------------------------------------------
V = 320


def _tiny(kind):
    if kind == "llama":
        from transformers import LlamaConfig

        return LlamaConfig(vocab_size=V, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
                           num_key_value_heads=2, head_dim=32, max_position_embeddings=128, bos_token_id=1, eos_token_id=2,
                           tie_word_embeddings=True), torch.bfloat16
    from transformers import GPT2Config

    return GPT2Config(vocab_size=V, n_embd=128, n_layer=2, n_head=4, n_positions=128), torch.float16


def _formula(names, shapes):
    return sum(n * k // 2 + 4 * (n * k // 64) for n, k in (shapes[p] for p in names))


def _twins(llm, cfg, dtype, seed):
    """(yardstick, truth): the architecture made again from the same seed, every quantised module's weight replaced by the
    backend's own dequantised W' in the 16-bit dtype - as a 16-bit model, and as its float32 copy."""
    from transformers import AutoModelForCausalLM

    from genlm_backend_amd.quant import W4Linear

    torch.manual_seed(seed)
    yard = AutoModelForCausalLM.from_config(cfg).to(dtype).to(DEV).eval()
    with torch.no_grad():
        for name, mod in llm.model.named_modules():
            if isinstance(mod, W4Linear):
                wq = mod.dequantize(dtype)
                tgt = yard.get_submodule(name)
                tgt.weight.copy_(wq.T if type(tgt).__name__ == "Conv1D" else wq)
    import copy

    truth = copy.deepcopy(yard).float()
    return yard, truth


def _err(rows, truth_rows):
    d = torch.stack([r.double().cpu() for r in rows]) - torch.stack([r.double().cpu() for r in truth_rows])
    return d.abs().max().item(), d.norm().item()


@pytest.mark.parametrize("kind", ["llama", "gpt2"])
@pytest.mark.parametrize("mode", ["fused", "dequant"])
def test_end_to_end(engine, kind, mode):
    """A quantised backend against a float32 model holding the dequantised weights (the truth); yardstick: an unquantised
    backend in the 16-bit dtype holding the same weights.  Max and Frobenius errors of the quantised backend's log-probs
    within 2x the yardstick's, through the re-encoding path and - as logZ under random masks - through auto_kv_rows, where
    the one-token forward is replayed from a hipGraph."""
    from genlm_backend_amd.llm import AsyncAmdLM
    from genlm_backend_amd.quant import W4Linear

    cfg, dtype = _tiny(kind)
    qt = "nf4" if kind == "llama" else "fp4"
    llm = AsyncAmdLM.from_config(cfg, None, device=DEV, dtype=dtype, seed=4, w4_gemm=mode, auto_kv_rows=32, auto_kv_cap=32,
                                 engine=engine,
                                 bitsandbytes_opts={"load_in_4bit": True, "bnb_4bit_quant_type": qt})
    rep = llm.quantization
    shapes = {n: (m.out_features, m.in_features) for n, m in llm.model.named_modules() if isinstance(m, W4Linear)}
    assert rep is not None and sorted(rep["modules"]) == sorted(shapes) and len(shapes) == (14 if kind == "llama" else 8)
    assert rep["bytes"] == _formula(rep["modules"], shapes) and rep["quant_type"] == qt
    assert list(rep["skipped"]) == ["lm_head"]
    assert not any(hasattr(m, "weight") for m in llm.model.modules() if isinstance(m, W4Linear))
    yard_model, truth_model = _twins(llm, cfg, dtype, 4)
    yard = AsyncAmdLM(yard_model, None, engine=engine)
    truth = AsyncAmdLM(truth_model, None, engine=engine)
    rs = np.random.default_rng(8)
    ctxs = [[int(t) for t in rs.integers(3, V, rs.integers(2, 12))] for _ in range(24)]
    got, yr, tr = (b.batch_next_token_logprobs_sync(ctxs) for b in (llm, yard, truth))
    q_max, q_fro = _err(got, tr)
    y_max, y_fro = _err(yr, tr)
    print(f"e2e {kind} {mode} re-encoding: max {q_max:.3e} / {y_max:.3e} = {q_max / y_max:.2f}, fro {q_fro:.3e} / {y_fro:.3e} = "
          f"{q_fro / y_fro:.2f}")
    assert q_max <= 2 * y_max and q_fro <= 2 * y_fro, (q_max, y_max, q_fro, y_fro)
    # the fused step over KV rows that follow the contexts: logZ under random masks, contexts grown by the drawn tokens
    masks = np.where(rs.random((2, V)) < 0.5, 0.0, -np.inf).astype(np.float32)
    llm.register_masks(torch.from_numpy(masks))
    mids = [i % 2 for i in range(len(ctxs))]
    dq, dy = [], []
    for _ in range(6):
        logZ, tok = llm.batch_next_token_step_sync(ctxs, mids)
        lz = np.asarray(logZ, np.float64)

        def ref_logz(b):
            rows = b.batch_next_token_logprobs_sync(ctxs)
            return np.array([np.logaddexp.reduce(r.double().cpu().numpy() + masks[m]) for r, m in zip(rows, mids)])

        t = ref_logz(truth)
        dq.append(lz - t)
        dy.append(ref_logz(yard) - t)
        ctxs = [c + [int(x)] for c, x in zip(ctxs, np.asarray(tok))]
    dq, dy = np.concatenate(dq), np.concatenate(dy)
    assert llm._auto_kv.stats["in_place_calls"] > 0 and llm._auto_kv._slab_fwd.graphs  # (replayed from a hipGraph)
    print(f"e2e {kind} {mode} auto_kv: max {np.abs(dq).max():.3e} / {np.abs(dy).max():.3e} = "
          f"{np.abs(dq).max() / np.abs(dy).max():.2f}, fro {np.linalg.norm(dq):.3e} / {np.linalg.norm(dy):.3e} = "
          f"{np.linalg.norm(dq) / np.linalg.norm(dy):.2f}")
    assert np.abs(dq).max() <= 2 * np.abs(dy).max() and np.linalg.norm(dq) <= 2 * np.linalg.norm(dy)
    del yard, truth, yard_model, truth_model, got, yr, tr


@pytest.mark.parametrize("kind", ["llama", "gpt2"])
def test_memory_sampling_and_the_references_call_shape(engine, kind):
    from genlm_backend_amd.llm import AsyncAmdLM
    from genlm_backend_amd.quant import W4Linear

    cfg, dtype = _tiny(kind)
    import gc

    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    plain = AsyncAmdLM.from_config(cfg, None, device=DEV, dtype=dtype, seed=4, engine=engine)
    torch.cuda.synchronize()
    full = torch.cuda.memory_allocated() - base
    del plain
    gc.collect()
    base = torch.cuda.memory_allocated()
    llm = AsyncAmdLM.from_config(cfg, None, device=DEV, dtype=dtype, seed=4, bitsandbytes_opts={"load_in_4bit": True},
                                 batch_size=10, timeout=0.01, engine=engine)
    assert llm.batch_size == 10 and llm.timeout == 0.01  # the reference's own call (tests/test_hf_llm.py:227-245)
    rep = llm.quantization
    assert rep["quant_type"] == "fp4"
    torch.cuda.synchronize()
    used = torch.cuda.memory_allocated() - base
    # every replaced weight is gone: what is left is the unquantised model minus those weights, plus images and the shared
    # dequantisation scratch.  Slack: the allocator rounds every block up to 512 bytes - one per image and one for the
    # scratch - plus 64 KiB for what the two constructions may round differently.
    want = full - rep["bytes_before"] + rep["bytes"] + rep["scratch_bytes"]
    slack = 512 * len(rep["modules"]) + (64 << 10)
    print(f"memory {kind}: unquantised {full}, quantised {used}, expected {want} (+ slack {slack})")
    assert used <= want + slack and used < full
    # sampling runs to completion and is reproducible under a seed
    prompts = [[5, 6, 7], [9, 3], [11, 12, 13, 14]]
    a = llm.batch_sample_sync(prompts, max_tokens=6, eos_token_ids=[2], seed=3)
    llm.clear_cache()
    b = llm.batch_sample_sync(prompts, max_tokens=6, eos_token_ids=[2], seed=3)
    assert a == b and len(a) == 3 and all(len(s) <= 6 for s in a)
    with pytest.raises(NotImplementedError, match="load_in_8bit"):
        AsyncAmdLM.from_config(cfg, None, device=DEV, dtype=dtype, bitsandbytes_opts={"load_in_8bit": True}, engine=engine)
