"""The two native pieces of the packed SIS step seen from a whole forward: on a random-init 2-layer
GPT-2 of width 128 - whose four projection shapes the split GEMM serves - 64 contexts are encoded packed and padded, with
the residual epilogue on and off and the native plan on and off: the last hidden rows and the logits are the same bits.
And the routing: in training mode, with autograd on, or with `split_gemms=False`, the blocks run their own adds - asserted
on the shadow's call path (SplitConv1D.fused_residuals), not on timing."""
import numpy as np
import pytest
import torch

from genlm_backend_amd import fuse
from genlm_backend_amd.fuse import SplitConv1D, split_gemm_all_rows
from genlm_backend_amd.kv import PromptGroups, encode_packed, encode_ragged, ragged

pytestmark = pytest.mark.gpu

V, EOS, D = 512, 0, 128
SHAPES = ((3 * D, D), (D, D), (4 * D, D), (D, 4 * D))  # (nf, nx) of c_attn, attn.c_proj, c_fc, mlp.c_proj


def _llm(engine, **kw):
    from transformers import GPT2Config

    from genlm_backend_amd.llm import AsyncAmdLM

    cfg = GPT2Config(vocab_size=V, n_positions=64, n_embd=D, n_layer=2, n_head=2, bos_token_id=EOS, eos_token_id=EOS)
    added = [s for s in SHAPES if s not in fuse.SPLIT_GEMM_MIN_ROWS]
    for s in added:  # (the dispatch table lists GPT-2 small's shapes: this body's run the kernel at every row count)
        fuse.SPLIT_GEMM_MIN_ROWS[s] = 0
    try:
        return AsyncAmdLM.from_config(cfg, None, device=engine.device, dtype=torch.float32, seed=11, engine=engine,
                                      batch_size=64, **kw)
    finally:
        for s in added:
            del fuse.SPLIT_GEMM_MIN_ROWS[s]


@pytest.fixture(scope="module")
def llm(engine):
    llm = _llm(engine)
    assert len(_projections(llm)) == 8 and all(engine.gemm_split_supports(nx, nf) for nf, nx in SHAPES)
    return llm


def _projections(llm):
    return [m for m in llm._body.modules() if isinstance(m, SplitConv1D)]


def _fused(llm):
    return sum(m.fused_residuals for m in _projections(llm))


@pytest.fixture(scope="module")
def contexts(llm):
    dev = llm.device
    rs = np.random.default_rng(5)
    prompts = [[int(t) for t in rs.integers(1, V, 6)], [int(t) for t in rs.integers(1, V, 3)]]
    U = 64
    grp = [u % 2 for u in range(U)]
    tails = [1 + u % 9 for u in range(U)]
    seqs = [prompts[g] + [int(t) for t in rs.integers(1, V, n)] for g, n in zip(grp, tails)]
    batch = tuple(torch.from_numpy(a).to(dev) for a in ragged(seqs))
    return dict(batch=batch, sel=torch.arange(U, dtype=torch.int32, device=dev), U=U,
                grp=torch.tensor(grp, dtype=torch.int32, device=dev), groups=PromptGroups(prompts, dev),
                n_tail_rows=sum(tails), l_max=max(len(s) for s in seqs))


def _packed(llm, c, native_plan=True):
    with torch.no_grad(), split_gemm_all_rows(llm.engine):
        rows = encode_packed(llm, c["batch"], c["sel"], c["U"], c["grp"], c["groups"], c["n_tail_rows"], max_keys=c["l_max"],
                             native_plan=native_plan).last_rows()
        return rows, llm._lm_head(rows)


def _padded(llm, c):
    with torch.no_grad():
        rows = encode_ragged(llm, c["batch"], c["sel"], c["U"], c["l_max"]).last_rows()
        return rows, llm._lm_head(rows)


@pytest.fixture()
def no_epilogue():
    fuse.RESIDUAL_EPILOGUE = False
    yield
    fuse.RESIDUAL_EPILOGUE = True


@pytest.fixture(scope="module")
def reference(llm, contexts):
    """Padded forward, every block running its own adds: computed once."""
    fuse.RESIDUAL_EPILOGUE = False
    try:
        before = _fused(llm)
        out = _padded(llm, contexts)
        assert _fused(llm) == before
        return out
    finally:
        fuse.RESIDUAL_EPILOGUE = True


def _same(got, want):
    for g, w in zip(got, want):
        assert g.shape == w.shape and torch.equal(g.view(torch.int32), w.view(torch.int32))


def test_padded_with_the_epilogue(llm, contexts, reference):
    before = _fused(llm)
    _same(_padded(llm, contexts), reference)
    assert _fused(llm) == before + 4  # two blocks, two c_proj each: every add ran in an epilogue


@pytest.mark.parametrize("native_plan", (True, False), ids=("native-plan", "torch-plan"))
def test_packed_with_the_epilogue(llm, contexts, reference, native_plan):
    before = _fused(llm)
    _same(_packed(llm, contexts, native_plan), reference)
    assert _fused(llm) == before + 4
    llm.engine.check()  # no segment was refused


@pytest.mark.parametrize("native_plan", (True, False), ids=("native-plan", "torch-plan"))
def test_packed_without_the_epilogue(llm, contexts, reference, no_epilogue, native_plan):
    before = _fused(llm)
    _same(_packed(llm, contexts, native_plan), reference)
    assert _fused(llm) == before


def _body_forward(llm):
    ids = torch.arange(1, 41, device=llm.device).view(2, 20)
    return llm._body(input_ids=ids).last_hidden_state


def test_training_mode_keeps_the_blocks_adds(llm):
    body = llm._body
    with torch.no_grad():
        want = _body_forward(llm)
        fused = _fused(llm)
        body.train()
        try:
            before = _fused(llm)
            _body_forward(llm)
            assert _fused(llm) == before  # no residual went into an epilogue
        finally:
            body.eval()
        assert _fused(llm) == fused
        _same((_body_forward(llm),), (want,))
        assert _fused(llm) == fused + 4


def test_autograd_keeps_the_blocks_adds(llm):
    with torch.no_grad():
        want = _body_forward(llm)
    before = _fused(llm)
    params = [p for p in llm._body.parameters()]
    was = [p.requires_grad for p in params]
    for p in params:
        p.requires_grad_(True)
    try:
        with torch.enable_grad():
            got = _body_forward(llm)
        assert got.requires_grad and _fused(llm) == before  # the modules' own code: addmm and ATen's add
    finally:
        for p, r in zip(params, was):
            p.requires_grad_(r)
    assert got.shape == want.shape


def test_split_gemms_off_keeps_the_blocks_adds(engine, llm):
    plain = _llm(engine, split_gemms=False)
    assert not _projections(plain)
    blocks = [m for m in plain._body.modules() if type(m).__name__ == "GPT2Block"]
    assert blocks and all("forward" not in b.__dict__ for b in blocks)  # the blocks' own forward, never patched
    patched = [m for m in llm._body.modules() if type(m).__name__ == "GPT2Block"]
    assert patched and all(b.__dict__["forward"].__func__ is fuse._gpt2_block_forward for b in patched)


def test_callers_model_is_untouched(llm):
    for m in llm.model.modules() if hasattr(llm, "model") else ():
        assert not isinstance(m, SplitConv1D) and "forward" not in m.__dict__
