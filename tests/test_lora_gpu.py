"""glb_lora_merge on the device against its bit-exact restatement (tests/lora_engine.py), and adapters served end to end
by AsyncAmdLM on the GPU against a model whose weights were merged beforehand."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.lora_engine import lora_merge_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 37  # elements of guard band around every output


@pytest.fixture(scope="module")
def eng():
    from genlm_backend_amd.engine import HipEngine

    return HipEngine(DEV)


def _case(rs, n_out, k_in, r, w_dtype, ab_dtype, transposed, pad=0, pad_o=None, mags=(1.0, 0.3, 0.3), scale=None):
    """(job dict, guarded output buffer, output pitch) with random data: `pad` / `pad_o` extra elements per row of W / out,
    `mags` the magnitudes of W, A and B."""
    wshape = (k_in, n_out) if transposed else (n_out, k_in)
    rows, cols = wshape
    pad_o = pad if pad_o is None else pad_o
    wbig = torch.from_numpy((rs.standard_normal((rows, cols + pad)) * mags[0]).astype(np.float32)).to(w_dtype).to(DEV)
    w = wbig[:, :cols]
    a = torch.from_numpy((rs.standard_normal((r, k_in)) * mags[1]).astype(np.float32)).to(ab_dtype).to(DEV)
    b = torch.from_numpy((rs.standard_normal((n_out, r)) * mags[2]).astype(np.float32)).to(ab_dtype).to(DEV)
    ld = cols + pad_o
    buf = torch.full((GUARD + rows * ld + GUARD,), 7.0, dtype=w_dtype, device=DEV)
    out = buf[GUARD:GUARD + rows * ld].view(rows, ld)[:, :cols]
    scale = float(np.float32(rs.uniform(0.1, 4.0))) if scale is None else scale
    return dict(w=w, a=a, b=b, scale=scale, transposed=transposed, out=out), buf, ld


def _check(job, buf, ld):
    want = lora_merge_ref(job["w"].cpu(), job["a"].cpu(), job["b"].cpu(), job["scale"], job["transposed"])
    got = job["out"].cpu()
    assert torch.equal(got.view(torch.int16 if got.element_size() == 2 else torch.int32),
                       want.view(torch.int16 if want.element_size() == 2 else torch.int32)), \
        f"merge differs: {tuple(job['w'].shape)} r={job['a'].shape[0]} {job['w'].dtype}/{job['a'].dtype} T={job['transposed']}"
    # guard bands and row padding untouched
    host = buf.cpu().float()
    rows, cols = job["out"].shape
    assert (host[:GUARD] == 7).all() and (host[GUARD + rows * ld:] == 7).all()
    if ld > cols:
        assert (host[GUARD:GUARD + rows * ld].view(rows, ld)[:, cols:] == 7).all()


@pytest.mark.parametrize("w_dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("ab_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("transposed", [False, True])
def test_merge_is_bit_exact_across_dtypes_and_layouts(eng, w_dtype, ab_dtype, transposed):
    rs = np.random.default_rng(10 * w_dtype.itemsize + ab_dtype.itemsize + 100 * int(transposed))
    for n_out, k_in, r, pad, pad_o in ((17, 1000, 16, 0, 0), (1000, 17, 3, 5, 5), (1, 1, 1, 0, 0), (300, 257, 64, 3, 3),
                                       (130, 129, 256, 0, 0), (256, 384, 16, 4, 0), (255, 130, 33, 0, 7)):
        job, buf, ld = _case(rs, n_out, k_in, r, w_dtype, ab_dtype, transposed, pad, pad_o)
        eng.lora_merge([job])
        torch.cuda.synchronize()
        _check(job, buf, ld)


@pytest.mark.parametrize("w_dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("ab_dtype", [torch.float32, torch.bfloat16])
def test_subnormal_operands_and_results_are_not_flushed(eng, w_dtype, ab_dtype):
    """A subnormal (float32 range: about 1e-39), products and sums in the subnormal range, W and the results subnormal in
    W's own type: the MFMA's A operand and accumulator, the epilogue's fma and the rounding keep them (no flush to zero)."""
    rs = np.random.default_rng(20 + w_dtype.itemsize + ab_dtype.itemsize)
    if w_dtype == torch.float16:  # (float16 subnormals lie below 6.1e-5: products of 1e-39 and 1e34)
        mags, scale = (3e-5, 1e-39, 1e34), 0.5
    else:
        mags, scale = (1e-39, 1e-39, 1.0), 0.5
    for n_out, k_in, r, transposed in ((64, 200, 16, False), (129, 70, 5, True)):
        job, buf, ld = _case(rs, n_out, k_in, r, w_dtype, ab_dtype, transposed, mags=mags, scale=scale)
        a32 = job["a"].float()
        assert ((a32 != 0) & (a32.abs() < 1.1754944e-38)).float().mean().item() > 0.5  # (A is mostly subnormal)
        eng.lora_merge([job])
        torch.cuda.synchronize()
        _check(job, buf, ld)
        tiny = torch.finfo(w_dtype).tiny
        o = job["out"].float()
        assert ((o != 0) & (o.abs() < tiny)).float().mean().item() > 0.3  # (results subnormal, kept)


def test_many_mixed_jobs_in_one_call_and_two_calls_agree(eng):
    rs = np.random.default_rng(5)
    cases = []
    dts = (torch.float32, torch.bfloat16, torch.float16)
    for i, (n_out, k_in, r) in enumerate(((17, 33, 1), (256, 128, 16), (1000, 64, 3), (64, 1000, 64), (129, 127, 256),
                                          (1, 500, 7), (384, 384, 16), (31, 1, 2), (2048, 256, 16), (200, 300, 33))):
        cases.append(_case(rs, n_out, k_in, r, dts[i % 3], (torch.float32, torch.bfloat16)[i % 2], bool(i % 3 == 1),
                           pad=(i % 4)))
    eng.lora_merge([c[0] for c in cases])
    torch.cuda.synchronize()
    for job, buf, ld in cases:
        _check(job, buf, ld)
    first = [c[0]["out"].clone() for c in cases]
    eng.lora_merge([c[0] for c in cases])
    torch.cuda.synchronize()
    for f, (job, _, _) in zip(first, cases):
        assert torch.equal(f.view(torch.uint8), job["out"].view(torch.uint8))


def test_argument_errors_return_einval_without_a_launch():
    from genlm_backend_amd import _lib

    lib = _lib.load()
    assert lib.glb_lora_merge_workspace_bytes(0) == 0 and lib.glb_lora_merge_workspace_bytes(224) >= 224 * 64
    q = (_lib.LoraJob * 1)()
    assert lib.glb_lora_merge(q, 1, None, 0, None) == _lib.GLB_EINVAL
    ws = torch.empty(lib.glb_lora_merge_workspace_bytes(1), dtype=torch.uint8, device=DEV)
    nb = ws.numel()
    assert lib.glb_lora_merge(q, 1, C.c_void_p(ws.data_ptr()), nb, None) == _lib.GLB_EINVAL
    assert "struct_size" in _lib.last_error()
    w = torch.zeros(8, 8, device=DEV)
    ab = torch.zeros(8, 8, device=DEV)
    j = q[0]
    j.struct_size = C.sizeof(_lib.LoraJob)
    j.w_dtype, j.ab_dtype, j.w_transposed = _lib.F32, _lib.F32, 0
    j.n_out, j.k_in, j.r = 8, 8, 8
    j.w, j.ldw, j.a, j.lda, j.b, j.ldb, j.scale, j.out, j.ldo = (w.data_ptr(), 8, ab.data_ptr(), 8, ab.data_ptr(), 8, 1.0,
                                                                w.data_ptr(), 8)
    assert lib.glb_lora_merge(q, 1, C.c_void_p(ws.data_ptr()), nb, None) == _lib.GLB_EINVAL  # out overlaps w
    assert "overlap" in _lib.last_error()
    out = torch.zeros(8, 8, device=DEV)
    j.out = out.data_ptr()
    j.r = 300
    j.lda = j.ldb = 300
    assert lib.glb_lora_merge(q, 1, C.c_void_p(ws.data_ptr()), nb, None) == _lib.GLB_EUNSUPPORTED
    assert "rank 300" in _lib.last_error()
    j.r, j.lda, j.ldb = 8, 8, 4  # ldb < r
    assert lib.glb_lora_merge(q, 1, C.c_void_p(ws.data_ptr()), nb, None) == _lib.GLB_EINVAL
    j.ldb, j.w_dtype = 8, 9
    assert lib.glb_lora_merge(q, 1, C.c_void_p(ws.data_ptr()), nb, None) == _lib.GLB_EINVAL
    j.w_dtype = _lib.F32
    assert lib.glb_lora_merge(q, 1, C.c_void_p(ws.data_ptr()), 8, None) == _lib.GLB_ENOSPC
    torch.cuda.synchronize()
    assert (out == 0).all()  # nothing ran
    # across jobs: one job's out may not be another job's w, a, b or out (the blocks of one call run in any order)
    q2 = (_lib.LoraJob * 2)()
    w2, out2 = torch.zeros(8, 8, device=DEV), torch.zeros(8, 8, device=DEV)
    ws2 = torch.empty(lib.glb_lora_merge_workspace_bytes(2), dtype=torch.uint8, device=DEV)
    for k, (src, dst) in enumerate(((w, out), (w2, out2))):
        C.memmove(C.addressof(q2[k]), C.addressof(j), C.sizeof(_lib.LoraJob))
        q2[k].w, q2[k].out = src.data_ptr(), dst.data_ptr()
    assert lib.glb_lora_merge(q2, 2, C.c_void_p(ws2.data_ptr()), ws2.numel(), None) == _lib.GLB_OK
    torch.cuda.synchronize()
    for bad in ("w", "out", "a"):
        q2[1].w, q2[1].out, q2[1].a = w2.data_ptr(), out2.data_ptr(), ab.data_ptr()
        setattr(q2[1], bad, out.data_ptr())  # job 1 reads / writes job 0's out
        if bad == "out":
            q2[1].w = w2.data_ptr()
        assert lib.glb_lora_merge(q2, 2, C.c_void_p(ws2.data_ptr()), ws2.numel(), None) == _lib.GLB_EINVAL, bad
        assert "of job" in _lib.last_error()


# ---- adapters served end to end -----------------------------------------------------------------------------------------
TOL = 1e-4  # float32 models (tests/test_host_gpu.py)
TOL_BF16 = 6e-2  # bfloat16 models (tests/test_host_gpu.py: attention through the library against SDPA)


def _contract_merged(model, tmp_dir, name):
    """A second model whose targeted weights are the contract's merge (lora_merge_ref) of the adapter in tmp_dir / name, and
    the adapter's modules."""
    import copy

    from genlm_backend_amd.lora import load_adapter

    ad = load_adapter(str(tmp_dir / name), model, name)
    ref = copy.deepcopy(model)
    with torch.no_grad():
        for p, lm in ad.modules.items():
            mod = ref.get_submodule(p)
            w = lora_merge_ref(mod.weight.cpu(), lm.a.cpu(), lm.b.cpu(), lm.scale, lm.transposed)
            mod.weight = torch.nn.Parameter(w.to(mod.weight.device))
    return ref, ad


def _lp(model, ctx):
    with torch.no_grad():
        return torch.log_softmax(model(torch.tensor([ctx], device=DEV)).logits[0, -1].float(), -1).cpu().numpy()


def test_gpt2_small_fp32_adapter_on_the_split_gemm_path(eng, tmp_path):
    from transformers import GPT2Config, GPT2LMHeadModel

    from genlm_backend_amd.llm import AsyncAmdLM
    from tests.test_lora_cpu import merged_reference, write_adapter

    torch.manual_seed(0)
    model = GPT2LMHeadModel(GPT2Config()).eval().to(DEV)
    targets = [f"transformer.h.{i}.{m}" for i in range(12) for m in ("attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj")]
    spec = write_adapter(tmp_path / "a", model, targets, r=16, alpha=32, fan_in_fan_out=True, seed=3)
    spec = {p: (a.to(DEV), b.to(DEV), float(np.float32(s)), c) for p, (a, b, s, c) in spec.items()}
    ref = merged_reference(model, spec)
    llm = AsyncAmdLM(model, None, engine=eng, batch_size=64, timeout=0.02)
    llm.add_new_lora(str(tmp_path / "a"), "a")
    llm.set_lora(lora_name="a")
    rs = np.random.default_rng(4)
    prompts = [[int(t) for t in rs.integers(0, 50257, 100)] for _ in range(16)]  # 1600 rows: the split GEMM's batches
    got = llm.batch_next_token_logprobs_sync(prompts).cpu().numpy()
    split = [m for m in llm._net.modules() if type(m).__name__ == "SplitConv1D" and m.__dict__.get("_glb_split") is not None]
    assert split and all(m.weight is not model.get_submodule(n).weight for n, m in llm._net.named_modules() if m in split)
    for p, g in zip(prompts[:4], got[:4]):
        assert np.abs(g - _lp(ref, p)).max() < TOL
    assert np.abs(got[0] - _lp(model, prompts[0])).max() > 10 * TOL  # (the adapter matters)
    # the merged weights are the kernel's: every targeted weight of the shadow equals the contract's merge bit for bit
    for p in targets[:8]:
        a, b, s, _ = spec[p]
        want = lora_merge_ref(model.get_submodule(p).weight.cpu(), a.cpu(), b.cpu(), s, True)
        assert torch.equal(llm._net.get_submodule(p).weight.cpu().view(torch.int32), want.view(torch.int32))


def _llama_bf16():
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(1)
    return LlamaForCausalLM(LlamaConfig(vocab_size=1000, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                                        num_attention_heads=4, num_key_value_heads=2, head_dim=64, max_position_embeddings=64,
                                        tie_word_embeddings=True)).eval().to(torch.bfloat16).to(DEV)


def test_llama_bf16_adapter_with_merged_qkv_gate_up_and_glb_attention(eng, tmp_path):
    from genlm_backend_amd.llm import AsyncAmdLM
    from tests.test_lora_cpu import LLAMA_TARGETS, write_adapter

    model = _llama_bf16()
    write_adapter(tmp_path / "a", model, LLAMA_TARGETS, r=16, alpha=16, seed=4, dtype=torch.bfloat16)
    ref, _ = _contract_merged(model, tmp_path, "a")
    llm = AsyncAmdLM(model, None, engine=eng, batch_size=64, timeout=0.02)
    assert llm.glb_attention and "gate_up" in llm.fused
    llm.add_new_lora(str(tmp_path / "a"), "a")
    llm.set_lora(lora_name="a")
    rs = np.random.default_rng(5)
    prompts = [[int(t) for t in rs.integers(0, 1000, n)] for n in (3, 9, 17, 30)]
    got = llm.batch_next_token_logprobs_sync(prompts).cpu().numpy()
    for p, g in zip(prompts, got):
        assert np.abs(g - _lp(ref, p)).max() < TOL_BF16
    attn = llm._net.model.layers[0].self_attn
    assert attn.__dict__["_glb_qkv"][3][0] is attn.q_proj.weight  # [q; k; v] made from the merged weights
    assert attn.q_proj.weight is not model.model.layers[0].self_attn.q_proj.weight
    assert llm._net.lm_head.weight is not model.model.embed_tokens.weight  # a tied head gets its own merged copy
    assert llm._net.model.embed_tokens.weight is model.model.embed_tokens.weight
    llm.clear_lora()
    fresh = AsyncAmdLM(model, None, engine=eng, batch_size=64, timeout=0.02)
    a = llm.batch_next_token_logprobs_sync(prompts).cpu()
    b = fresh.batch_next_token_logprobs_sync(prompts).cpu()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_device_sis_with_graph_replays_under_an_adapter(eng, tmp_path):
    from genlm_backend_amd.llm import AsyncAmdLM
    from genlm_backend_amd.sis import DeviceSIS
    from tests.test_lora_cpu import LLAMA_TARGETS, write_adapter

    model = _llama_bf16()
    write_adapter(tmp_path / "a", model, LLAMA_TARGETS, r=8, alpha=16, seed=6, dtype=torch.bfloat16)
    ref, _ = _contract_merged(model, tmp_path, "a")
    rs = np.random.default_rng(7)
    masks = torch.from_numpy(np.where(rs.random((2, 1000)) < 0.7, 0.0, -np.inf).astype(np.float32))
    prompt = [int(t) for t in rs.integers(0, 1000, 6)]

    def run(m):
        m.register_masks(masks)
        sis = DeviceSIS(m, 32, prompt, max_tokens=8, eos_id=0, seed=11, use_particle_kv=True, share_kv=False)
        sis.run()
        assert sis._slab_fwd is not None and sis._slab_fwd.graphs  # (the one-token forward was replayed from a hipGraph)
        return sis.results()

    llm = AsyncAmdLM(model, None, engine=eng, batch_size=64, timeout=0.02)
    base = run(llm)
    llm.add_new_lora(str(tmp_path / "a"), "a")
    llm.set_lora(lora_name="a")
    got = run(llm)
    want = run(AsyncAmdLM(ref, None, engine=eng, batch_size=64, timeout=0.02))
    assert got[0] == want[0] and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert got[0] != base[0]
    llm.clear_lora()
    after = run(llm)
    fresh = run(AsyncAmdLM(model, None, engine=eng, batch_size=64, timeout=0.02))
    assert after[0] == fresh[0] == base[0]
    assert np.array_equal(after[1].view(np.uint32), fresh[1].view(np.uint32))
