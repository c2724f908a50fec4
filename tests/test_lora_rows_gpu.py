"""glb_lora_rows on the device: against float64 with torch's unmerged form as the yardstick, untouched rows and padding, row
independence (other rows' slots and values, M, graph replay), argument errors, and `lora_names` end to end on GPT-2-shaped
fp32, Llama-shaped bf16 and an NF4 base against hooked references run by torch on the device."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
SHAPES = [(2304, 768), (768, 3072), (2048, 2048), (512, 2048), (8192, 2048), (1000, 777)]  # (N, K); the last: odd, element accesses
ROWS = [1, 7, 64, 1000, 9216]
TABLES = [[1], [3], [4], [16], [64], [256], [16, 3, None, 64, 1, 256, 4]]  # ranks per slot; None: the slot lacks the module
PATTERNS = ["none", "one", "blocks", "random"]
PADS = [0, 64, 3]  # ldy - N
MIXED = TABLES[-1]
# crossings the diagonal of test_against_float64 does not meet: (ranks, (N, K), M, pattern, pad)
CROSSINGS = [([256], (2304, 768), 9216, "random", 3),  # the largest rank at the largest M
             (MIXED, (8192, 2048), 1000, "blocks", 64),  # the mixed table on the widest shape, ldy > N
             (MIXED, (512, 2048), 9216, "blocks", 64),
             (MIXED, (2048, 2048), 1, "random", 0),  # one row: a random slot, and (next) a slot that certainly has an adapter
             (MIXED, (1000, 777), 1, "one", 3)]


@pytest.fixture(scope="module")
def eng():
    from genlm_backend_amd.engine import HipEngine

    return HipEngine(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _table(eng, g, ranks, n, k, ab_dtype, extra_module=True):
    """A table with len(ranks) slots and two modules (the second has other shapes and is never applied); returns
    (table, [(A, B, scale) or None per slot])."""
    ents, slots = [], []
    for r in ranks:
        if r is None:
            ents.append(None)
            slots.append([None, None])
            continue
        a = (torch.randn(r, k, generator=g, device=DEV) * 0.05).to(ab_dtype)
        b = (torch.randn(n, r, generator=g, device=DEV) * 0.05).to(ab_dtype)
        s = float(np.float32(1.0 + 0.5 * len(ents)))
        ents.append((a, b, s))
        other = dict(a=torch.zeros(2, 8, device=DEV, dtype=ab_dtype), b=torch.zeros(8, 2, device=DEV, dtype=ab_dtype), scale=1.0)
        slots.append([dict(a=a, b=b, scale=s), other if extra_module else None])
    if all(e is None for e in ents):
        raise ValueError("a table needs one adapter")
    return eng.lora_rows_table(slots), ents


def _slots(g, pattern, m, n_slots):
    if pattern == "none":
        s = torch.full((m,), -1, dtype=torch.int32)
    elif pattern == "one":
        s = torch.full((m,), n_slots - 1, dtype=torch.int32)
    elif pattern == "blocks":
        s = (torch.arange(m) * (n_slots + 1) // max(m, 1) - 1).to(torch.int32)
    else:
        s = torch.randint(-1, n_slots, (m,), generator=torch.Generator().manual_seed(int(g.initial_seed()) + m)).to(torch.int32)
    return s.to(DEV)


def _refs(x, y, slots, ents):
    """(float64 result, torch's unmerged form in the promoted dtype of x and A - `y + s * F.linear(F.linear(x, A), B)` per
    slot with index_select / index_add_)."""
    want = y.double()
    yard = y.clone()
    for si, e in enumerate(ents):
        rows = (slots == si).nonzero().flatten()
        if e is None or rows.numel() == 0:
            continue
        a, b, s = e
        xs = x.index_select(0, rows)
        want[rows] += s * ((xs.double() @ a.double().T) @ b.double().T)
        pd = torch.promote_types(x.dtype, a.dtype)
        d = s * F.linear(F.linear(xs.to(pd), a.to(pd)), b.to(pd))
        yard.index_add_(0, rows, d.to(y.dtype))
    return want, yard


@pytest.mark.parametrize("x_dtype", DTYPES, ids=["x_f32", "x_bf16", "x_f16"])
@pytest.mark.parametrize("ab_dtype", DTYPES, ids=["ab_f32", "ab_bf16", "ab_f16"])
def test_against_float64(eng, x_dtype, ab_dtype):
    """The kernel's maximum error against float64 is at most 2x the error of torch's unmerged form in the same dtypes (the
    criterion of tests/test_split_gemm_gpu.py).  Every (N, K), M, rank table, slot pattern and pitch appears for every pair of
    dtypes on a diagonal through them, then CROSSINGS."""
    pair = DTYPES.index(x_dtype) * 3 + DTYPES.index(ab_dtype)
    g = torch.Generator(device=DEV).manual_seed(100 + pair)
    worst = 0.0
    diagonal = [(ranks, SHAPES[i % len(SHAPES)], ROWS[(i + pair) % len(ROWS)], PATTERNS[(i + pair) % len(PATTERNS)],
                 PADS[(i + pair) % len(PADS)]) for i, ranks in enumerate(TABLES)]
    for ranks, (n, k), m, pattern, pad in diagonal + CROSSINGS:
        table, ents = _table(eng, g, ranks, n, k, ab_dtype)
        x = torch.randn(m, k, generator=g, device=DEV).to(x_dtype)
        ybuf = torch.randn(m, n + pad, generator=g, device=DEV).to(x_dtype)
        y = ybuf[:, :n]
        slots = _slots(g, pattern, m, len(ranks))
        want, yard = _refs(x, y, slots, ents)
        before = ybuf.clone()
        eng.lora_rows(x, y, slots, table, 0)
        torch.cuda.synchronize()
        e_k = (y.double() - want).abs().max().item()
        e_y = (yard.double() - want).abs().max().item()
        worst = max(worst, e_k / e_y if e_y > 0 else (0.0 if e_k == 0 else float("inf")))
        print(f"lora_rows x {x_dtype} ab {ab_dtype} M {m} N {n} K {k} ranks {ranks} {pattern} pad {pad}: "
              f"kernel {e_k:.3e} torch {e_y:.3e}")
        assert e_k <= 2 * e_y, (m, n, k, ranks, pattern, e_k, e_y)
        if pad:
            assert torch.equal(_bits(ybuf[:, n:]), _bits(before[:, n:]))
        idle = torch.tensor([si < 0 or ents[si] is None for si in slots.cpu().tolist()], device=DEV)
        assert torch.equal(_bits(y[idle]), _bits(before[:, :n][idle]))
    print(f"lora_rows x {x_dtype} ab {ab_dtype}: worst kernel / torch error ratio {worst:.2f}")


@pytest.mark.parametrize("x_dtype", DTYPES, ids=["f32", "bf16", "f16"])
def test_untouched_rows_and_padding(eng, x_dtype):
    g = torch.Generator(device=DEV).manual_seed(7)
    n, k, m, pad = 512, 256, 333, 24
    table, ents = _table(eng, g, [8, None, 16], n, k, torch.bfloat16)
    x = torch.randn(m, k + 8, generator=g, device=DEV).to(x_dtype)[:, :k]  # (ldx > K)
    ybuf = torch.randn(m, n + pad, generator=g, device=DEV).to(x_dtype)
    y = ybuf[:, :n]
    slots = _slots(g, "random", m, 3)
    slots[::11] = 7  # a slot beyond the table: as -1
    before = ybuf.clone()
    want, _ = _refs(x, y, slots, ents)
    eng.lora_rows(x, y, slots, table, 0)
    torch.cuda.synchronize()
    sl = slots.cpu()
    idle = ((sl < 0) | (sl == 1) | (sl == 7)).to(DEV)
    assert idle.any() and (~idle).any()
    assert torch.equal(_bits(ybuf[idle]), _bits(before[idle]))  # rows: slot -1, a slot without the module, outside the table
    assert torch.equal(_bits(ybuf[:, n:]), _bits(before[:, n:]))  # padding beyond N
    assert not torch.equal(_bits(y[~idle]), _bits(before[:, :n][~idle]))
    tol = 1e-5 if x_dtype == torch.float32 else 5e-2
    assert (y.double() - want).abs().max().item() < tol
    # module 1 of the table has other shapes than the call: nothing is written
    eng.lora_rows(x, y, slots, table, 1)
    torch.cuda.synchronize()
    assert (y.double() - want).abs().max().item() < tol


@pytest.mark.parametrize("x_dtype,ab_dtype", [(torch.float32, torch.float32), (torch.bfloat16, torch.bfloat16),
                                              (torch.float16, torch.float32)], ids=["f32", "bf16", "f16_f32"])
def test_row_independence_and_graph_replay(eng, x_dtype, ab_dtype):
    g = torch.Generator(device=DEV).manual_seed(9)
    n, k, m = 768, 1000, 300
    table, _ = _table(eng, g, [16, 3, 64], n, k, ab_dtype)
    keep = torch.tensor([5, 17, 40, 150, 299], device=DEV)
    x = torch.randn(m, k, generator=g, device=DEV).to(x_dtype)
    y0 = torch.randn(m, n, generator=g, device=DEV).to(x_dtype)
    slots = _slots(g, "random", m, 3)
    slots[keep] = torch.tensor([0, 1, 2, 0, 2], dtype=torch.int32, device=DEV)

    def run(xx, ss, rows=m):
        y = y0[:rows].clone()
        eng.lora_rows(xx[:rows], y, ss[:rows].contiguous(), table, 0)
        return y

    first = run(x, slots)
    assert torch.equal(_bits(run(x, slots)), _bits(first))  # two runs
    # other rows: other values, other slots
    x2 = torch.randn(m, k, generator=g, device=DEV).to(x_dtype)
    x2[keep] = x[keep]
    s2 = _slots(torch.Generator(device=DEV).manual_seed(10), "random", m, 3)
    s2[keep] = slots[keep]
    assert torch.equal(_bits(run(x2, s2)[keep]), _bits(first[keep]))
    s3 = torch.full_like(slots, -1)
    s3[keep] = slots[keep]
    assert torch.equal(_bits(run(x2, s3)[keep]), _bits(first[keep]))
    # another M: fewer rows, and the same rows inside a larger batch
    assert torch.equal(_bits(run(x2, s2, rows=41)[keep[:3]]), _bits(first[keep[:3]]))
    big_m = 2000
    xb = torch.randn(big_m, k, generator=g, device=DEV).to(x_dtype)
    xb[keep] = x[keep]
    yb = torch.randn(big_m, n, generator=g, device=DEV).to(x_dtype)
    yb[keep] = y0[keep]
    sb = _slots(torch.Generator(device=DEV).manual_seed(11), "random", big_m, 3)
    sb[keep] = slots[keep]
    eng.lora_rows(xb, yb, sb, table, 0)
    assert torch.equal(_bits(yb[keep]), _bits(first[keep]))
    # a hipGraph replay gives the eager bits
    out = y0.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        eng.lora_rows(x, out, slots, table, 0)  # (warm: the workspace exists before capture)
        out.copy_(y0)
        with torch.cuda.graph(graph, stream=side):
            eng.lora_rows(x, out, slots, table, 0)
    torch.cuda.current_stream().wait_stream(side)
    out.copy_(y0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(first))


def test_argument_errors_return_without_a_launch(eng):
    from genlm_backend_amd import _lib

    lib = _lib.load()
    assert lib.glb_lora_rows_table_bytes(0, 1) == 0 and lib.glb_lora_rows_table_bytes(65, 1) == 0
    assert lib.glb_lora_rows_table_bytes(8, 100) >= 8 * 100 * 64
    assert lib.glb_lora_rows_workspace_bytes(0, 16) == 0 and lib.glb_lora_rows_workspace_bytes(10, 257) == 0
    assert lib.glb_lora_rows_workspace_bytes(1000, 16) >= 1000 * 16 * 4
    a = _lib.LoraRowsArgs()
    assert lib.glb_lora_rows(None, None) == _lib.GLB_EINVAL
    assert lib.glb_lora_rows(C.byref(a), None) == _lib.GLB_EINVAL and "struct_size" in _lib.last_error()
    a.struct_size = C.sizeof(_lib.LoraRowsArgs)  # (the library compares it with its own sizeof: the layouts agree)
    assert lib.glb_lora_rows(C.byref(a), None) == _lib.GLB_EINVAL and "struct_size" not in _lib.last_error()
    g = torch.Generator(device=DEV).manual_seed(1)
    table, _ = _table(eng, g, [4], 64, 32, torch.float32)
    x = torch.zeros(8, 32, device=DEV)
    y = torch.ones(8, 64, device=DEV)
    slots = torch.zeros(8, dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.glb_lora_rows_workspace_bytes(8, 4), dtype=torch.uint8, device=DEV)

    def fill():
        a.dtype, a.m, a.n, a.k = _lib.F32, 8, 64, 32
        a.x, a.ldx, a.y, a.ldy = x.data_ptr(), 32, y.data_ptr(), 64
        a.row_slot, a.table = slots.data_ptr(), table.dev.data_ptr()
        a.n_slots, a.n_modules, a.module, a.r_max = 1, 2, 0, 4
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()

    for field, bad, code in (("dtype", 7, _lib.GLB_EINVAL), ("m", 0, _lib.GLB_EINVAL), ("ldy", 63, _lib.GLB_EINVAL),
                             ("ldx", 31, _lib.GLB_EINVAL), ("x", None, _lib.GLB_EINVAL), ("row_slot", None, _lib.GLB_EINVAL),
                             ("module", 2, _lib.GLB_EINVAL), ("r_max", 0, _lib.GLB_EINVAL), ("r_max", 257, _lib.GLB_EUNSUPPORTED),
                             ("n_slots", 65, _lib.GLB_EUNSUPPORTED), ("workspace_bytes", 16, _lib.GLB_ENOSPC),
                             ("y", x.data_ptr(), _lib.GLB_EINVAL), ("x", x.data_ptr() + 2, _lib.GLB_EINVAL)):
        fill()
        setattr(a, field, bad)
        assert lib.glb_lora_rows(C.byref(a), None) == code, field
    torch.cuda.synchronize()
    assert bool((y == 1).all())  # nothing was launched
    fill()
    assert lib.glb_lora_rows(C.byref(a), None) == _lib.GLB_OK
    torch.cuda.synchronize()
    # the table upload
    e = (_lib.LoraRowsEntry * 1)()
    dev = torch.empty(256, dtype=torch.uint8, device=DEV)
    assert lib.glb_lora_rows_table_upload(e, 1, 1, C.c_void_p(dev.data_ptr()), 256, None) == _lib.GLB_EINVAL
    assert "struct_size" in _lib.last_error()
    e[0].struct_size = C.sizeof(_lib.LoraRowsEntry)
    assert lib.glb_lora_rows_table_upload(e, 1, 1, C.c_void_p(dev.data_ptr()), 256, None) == _lib.GLB_OK  # (r == 0: absent)
    e[0].r, e[0].n_out, e[0].k_in, e[0].lda, e[0].ldb = 4, 64, 32, 32, 4
    assert lib.glb_lora_rows_table_upload(e, 1, 1, C.c_void_p(dev.data_ptr()), 256, None) == _lib.GLB_EINVAL  # null a / b
    e[0].a, e[0].b = x.data_ptr(), y.data_ptr()
    e[0].r, e[0].ldb = 257, 257
    assert lib.glb_lora_rows_table_upload(e, 1, 1, C.c_void_p(dev.data_ptr()), 256, None) == _lib.GLB_EUNSUPPORTED
    e[0].r, e[0].ldb = 4, 3
    assert lib.glb_lora_rows_table_upload(e, 1, 1, C.c_void_p(dev.data_ptr()), 256, None) == _lib.GLB_EINVAL
    assert lib.glb_lora_rows_table_upload(e, 1, 1, C.c_void_p(dev.data_ptr()), 16, None) == _lib.GLB_ENOSPC
    assert lib.glb_lora_rows_table_upload(e, 65, 1, C.c_void_p(dev.data_ptr()), 256, None) == _lib.GLB_EUNSUPPORTED
    torch.cuda.synchronize()


# ---- end to end ---------------------------------------------------------------------------------------------------------
TOL = 1e-4  # float32 models (tests/test_lora_gpu.py)
TOL_BF16 = 6e-2  # bfloat16 models (tests/test_lora_gpu.py)


def _hooked(model, spec, dtype):
    """peft's unmerged form as forward hooks on a copy of `model`, A / B in `dtype` on the device."""
    ref = copy.deepcopy(model)
    for p, (a, b, s, conv) in spec.items():
        def hook(mod, args, out, a=a.to(DEV, dtype), b=b.to(DEV, dtype), s=s):
            return out + s * ((args[0] @ a.T) @ b.T)

        ref.get_submodule(p).register_forward_hook(hook)
    return ref


def _lp(model, ctx):
    with torch.no_grad():
        return torch.log_softmax(model(torch.tensor([ctx], device=DEV)).logits[0, -1].float(), -1).cpu().numpy()


def _f32(spec):
    return {p: (a, b, float(np.float32(s)), conv) for p, (a, b, s, conv) in spec.items()}


def test_gpt2_fp32_mixed_batch_on_the_split_gemm_path(eng, tmp_path):
    from transformers import GPT2Config, GPT2LMHeadModel

    from genlm_backend_amd.llm import AsyncAmdLM
    from tests.test_lora_cpu import write_adapter

    torch.manual_seed(0)
    model = GPT2LMHeadModel(GPT2Config(n_layer=4)).eval().to(DEV)
    targets = [f"transformer.h.{i}.{m}" for i in range(4) for m in ("attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj")]
    sa = _f32(write_adapter(tmp_path / "a", model, targets, r=16, alpha=32, fan_in_fan_out=True, seed=3))
    sb = _f32(write_adapter(tmp_path / "b", model, targets[2:9], r=4, alpha=16, fan_in_fan_out=True, seed=4,
                            rank_pattern={"c_fc": 64}))
    refs = {None: model, "a": _hooked(model, sa, torch.float32), "b": _hooked(model, sb, torch.float32)}
    llm = AsyncAmdLM(model, None, engine=eng, batch_size=64, timeout=0.02)
    llm.add_new_lora(str(tmp_path / "a"), "a")
    llm.add_new_lora(str(tmp_path / "b"), "b")
    rs = np.random.default_rng(4)
    prompts = [[int(t) for t in rs.integers(0, 50257, 100)] for _ in range(6)] * 3  # 1800 rows: the split GEMM's batches
    names = [None] * 6 + ["a"] * 6 + ["b"] * 6
    base = llm.batch_next_token_logprobs_sync(prompts[:6]).cpu()
    got = llm.batch_next_token_logprobs_sync(prompts, lora_names=names).cpu().numpy()
    assert any(type(m).__name__ == "SplitConv1D" and m.__dict__.get("_glb_split") is not None for m in llm._net.modules())
    assert llm.stats["lora_rows_calls"] == 16 and llm.stats["unique"] == 6 + 18
    want = {nm: [_lp(refs[nm], p) for p in prompts[:2]] for nm in (None, "a", "b")}
    for i, nm in ((0, None), (1, None), (6, "a"), (7, "a"), (12, "b"), (13, "b")):
        assert np.abs(got[i] - want[nm][i % 6]).max() < TOL, (i, nm)
    assert np.abs(want["a"][0] - want[None][0]).max() > 10 * TOL and np.abs(want["b"][0] - want["a"][0]).max() > 10 * TOL
    # base rows of the mixed call are the base model's, and default calls are served by the trie as before
    assert np.abs(got[:6] - base.numpy()).max() < TOL
    batches = llm.stats["batches"]
    again = llm.batch_next_token_logprobs_sync(prompts[:6]).cpu()
    assert llm.stats["batches"] == batches and torch.equal(again.view(torch.int32), base.view(torch.int32))
    # the fused step: logZ under masks against the hooked references
    masks = np.where(rs.random((2, 50257)) < 0.5, 0.0, -np.inf).astype(np.float32)
    llm.register_masks(torch.from_numpy(masks))
    mids = [i % 2 for i in range(18)]
    logZ, tok = llm.batch_next_token_step_sync(prompts, mids, lora_names=names)
    for i, nm in ((0, None), (7, "a"), (13, "b")):
        wz = np.logaddexp.reduce((want[nm][i % 6] + masks[mids[i]]).astype(np.float64))
        assert abs(float(logZ[i]) - wz) < TOL
    assert all(masks[m][t] == 0 for m, t in zip(mids, np.asarray(tok)))


def _llama_bf16():
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(1)
    return LlamaForCausalLM(LlamaConfig(vocab_size=1000, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                                        num_attention_heads=4, num_key_value_heads=2, head_dim=64, max_position_embeddings=64,
                                        tie_word_embeddings=True)).eval().to(torch.bfloat16).to(DEV)


def test_llama_bf16_mixed_batch_with_merged_qkv_gate_up_and_glb_attention(eng, tmp_path):
    from genlm_backend_amd.llm import AsyncAmdLM
    from tests.test_lora_cpu import LLAMA_TARGETS, write_adapter

    model = _llama_bf16()
    sa = _f32(write_adapter(tmp_path / "a", model, LLAMA_TARGETS, r=16, alpha=16, seed=4, dtype=torch.bfloat16,
                            rank_pattern={"q_proj": 8, "lm_head": 2}))
    sb = _f32(write_adapter(tmp_path / "b", model, LLAMA_TARGETS[2:11], r=5, alpha=10, seed=5, rslora=True))  # (float32 A / B)
    refs = {None: model, "a": _hooked(model, sa, torch.bfloat16), "b": _hooked(model, sb, torch.bfloat16)}
    llm = AsyncAmdLM(model, None, engine=eng, batch_size=64, timeout=0.02)
    assert llm.glb_attention and "gate_up" in llm.fused
    llm.add_new_lora(str(tmp_path / "a"), "a")
    llm.add_new_lora(str(tmp_path / "b"), "b")
    rs = np.random.default_rng(5)
    prompts = [[int(t) for t in rs.integers(0, 1000, n)] for n in (3, 9, 17, 30)] * 3
    names = [None] * 4 + ["a"] * 4 + ["b"] * 4
    fresh = AsyncAmdLM(model, None, engine=eng, batch_size=64, timeout=0.02)
    base = llm.batch_next_token_logprobs_sync(prompts[:4]).cpu()
    got = llm.batch_next_token_logprobs_sync(prompts, lora_names=names).float().cpu().numpy()
    for p, nm, gr in zip(prompts, names, got):
        assert np.abs(gr - _lp(refs[nm], p)).max() < TOL_BF16, nm
    assert np.abs(_lp(refs["a"], prompts[3]) - _lp(model, prompts[3])).max() > 10 * TOL
    llm.clear_cache()
    after = llm.batch_next_token_logprobs_sync(prompts[:4]).cpu()
    plain = fresh.batch_next_token_logprobs_sync(prompts[:4]).cpu()
    assert torch.equal(_bits(after), _bits(base)) and torch.equal(_bits(after), _bits(plain))


@pytest.mark.parametrize("mode", ["fused", "dequant"])
def test_nf4_base_mixed_batch(eng, tmp_path, mode):
    """LoRA over a 4-bit base: against a float32 model holding the dequantised weights with the unmerged hooks (the truth);
    yardstick: the same architecture in the 16-bit dtype with the hooks, run by torch.  Max and Frobenius errors within 2x
    the yardstick's (the criterion of tests/test_quant4_gpu.py::test_end_to_end)."""
    from genlm_backend_amd.llm import AsyncAmdLM
    from tests.test_lora_cpu import LLAMA_TARGETS, write_adapter
    from tests.test_quant4_gpu import V, _tiny, _twins

    cfg, dtype = _tiny("llama")
    llm = AsyncAmdLM.from_config(cfg, None, device=DEV, dtype=dtype, seed=4, w4_gemm=mode, engine=eng,
                                 bitsandbytes_opts={"load_in_4bit": True, "bnb_4bit_quant_type": "nf4"})
    yard_model, truth_model = _twins(llm, cfg, dtype, 4)
    sa = _f32(write_adapter(tmp_path / "a", yard_model, LLAMA_TARGETS, r=8, alpha=32, seed=4, dtype=torch.bfloat16))
    sb = _f32(write_adapter(tmp_path / "b", yard_model, LLAMA_TARGETS[:7], r=4, alpha=32, seed=5, dtype=torch.bfloat16))
    llm.add_new_lora(str(tmp_path / "a"), "a")
    llm.add_new_lora(str(tmp_path / "b"), "b")
    with pytest.raises(ValueError, match="quantised"):
        llm.set_lora(lora_name="a")
    llm.clear_lora()
    rs = np.random.default_rng(8)
    ctxs = [[int(t) for t in rs.integers(3, V, rs.integers(2, 12))] for _ in range(8)] * 3
    names = [None] * 8 + ["a"] * 8 + ["b"] * 8
    got = llm.batch_next_token_logprobs_sync(ctxs, lora_names=names).double().cpu()
    truth = {nm: (truth_model if nm is None else _hooked(truth_model, s, torch.float32)) for nm, s in ((None, None), ("a", sa), ("b", sb))}
    yard = {nm: (yard_model if nm is None else _hooked(yard_model, s, dtype)) for nm, s in ((None, None), ("a", sa), ("b", sb))}
    tr = torch.stack([torch.from_numpy(_lp(truth[nm], c)).double() for nm, c in zip(names, ctxs)])
    yr = torch.stack([torch.from_numpy(_lp(yard[nm], c)).double() for nm, c in zip(names, ctxs)])
    q_max, q_fro = (got - tr).abs().max().item(), (got - tr).norm().item()
    y_max, y_fro = (yr - tr).abs().max().item(), (yr - tr).norm().item()
    print(f"nf4 lora rows {mode}: max {q_max:.3e} / {y_max:.3e}, fro {q_fro:.3e} / {y_fro:.3e}")
    assert q_max <= 2 * y_max and q_fro <= 2 * y_fro, (q_max, y_max, q_fro, y_fro)
    assert (tr[8:16] - tr[0:8]).abs().max() > 1e-2 and (tr[16:24] - tr[8:16]).abs().max() > 1e-2  # (the adapters matter)
