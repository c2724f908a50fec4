"""glb_packed_plan (the plan of kv.encode_packed in two launches) against its two restatements: kv.packed_plan
(NumPy) and the torch ops of `encode_packed(native_plan=False)` - the four arrays element for element, for well-formed
batches and for hostile ones built by hand (a caller's row count above and below the true sum, a zero tail, a prompt group
out of range), where every index must stay in range and the attention kernel must refuse what it refuses today."""
import numpy as np
import pytest
import torch

from genlm_backend_amd import kv
from genlm_backend_amd.kv import PromptGroups, encode_packed, packed_plan, ragged

pytestmark = pytest.mark.gpu

V, EOS = 512, 0
US = (1, 2, 64, 65, 1025)  # one context, one wave, past a wave, past the scan's 1024-thread stride
TAILS = {"ones": lambda u: 1, "nines": lambda u: 9, "ragged": lambda u: 1 + (u * 7) % 24}


@pytest.fixture(scope="module")
def llm(engine):
    from transformers import GPT2Config

    from genlm_backend_amd.llm import AsyncAmdLM

    cfg = GPT2Config(vocab_size=V, n_positions=64, n_embd=128, n_layer=2, n_head=2, bos_token_id=EOS, eos_token_id=EOS)
    return AsyncAmdLM.from_config(cfg, None, device=engine.device, dtype=torch.float32, seed=3, engine=engine, batch_size=64)


def _batch(G, U, tail_of, dev, seed=0):
    rs = np.random.default_rng(seed)
    prompts = [[int(t) for t in rs.integers(1, V, 1 + (3 * g + 7) % 8)] for g in range(G)]  # lengths 1 .. 8
    grp = [(u * 5 + 1) % G for u in range(U)]
    tails = [tail_of(u) for u in range(U)]
    seqs = [prompts[g] + [int(t) for t in rs.integers(1, V, n)] for g, n in zip(grp, tails)]
    batch = tuple(torch.from_numpy(a).to(dev) for a in ragged(seqs))
    return prompts, grp, tails, seqs, batch


def _plans(llm, batch, sel, U, grp_d, groups, n_tail_rows):
    native = kv._packed_plan_arrays(llm, batch, sel, U, grp_d, groups, n_tail_rows, native_plan=True)
    torch_ops = kv._packed_plan_arrays(llm, batch, sel, U, grp_d, groups, n_tail_rows, native_plan=False)
    return native, torch_ops


def _assert_same(native, torch_ops):
    for name, a, b in zip(("segments", "ids", "pos", "last"), native, torch_ops):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert torch.equal(a, b), name
    assert native[4] == torch_ops[4]


@pytest.mark.parametrize("tails", sorted(TAILS))
@pytest.mark.parametrize("U", US)
@pytest.mark.parametrize("G", (1, 3))
def test_equals_numpy_plan_and_torch_ops(llm, G, U, tails):
    dev = llm.device
    prompts, grp, tail, seqs, batch = _batch(G, U, TAILS[tails], dev, seed=U + G)
    sel = torch.arange(U, dtype=torch.int32, device=dev)
    grp_d = torch.tensor(grp, dtype=torch.int32, device=dev)
    groups = PromptGroups(prompts, dev)
    native, torch_ops = _plans(llm, batch, sel, U, grp_d, groups, sum(tail))
    _assert_same(native, torch_ops)
    seg, pos, where, last = packed_plan([len(p) for p in prompts], grp, [len(s) for s in seqs])
    ids = np.array([prompts[-1 - c][o] if c < 0 else seqs[c][o] for c, o in where], np.int64)
    for name, got, want in zip(("segments", "ids", "pos", "last"), native, (seg, ids, pos, last)):
        assert np.array_equal(got.cpu().numpy(), want), name


def test_selection_in_another_order(llm):
    """`sel` picks contexts out of order and leaves some out; entries of sel and grp past n_sel are not read."""
    dev = llm.device
    prompts, grp, tail, seqs, batch = _batch(3, 40, TAILS["ragged"], dev, seed=9)
    order = [int(i) for i in np.random.default_rng(1).permutation(40)[:23]]
    sel = torch.tensor(order + [10 ** 6] * 5, dtype=torch.int32, device=dev)
    grp_d = torch.tensor([grp[i] for i in order] + [-77] * 5, dtype=torch.int32, device=dev)
    native, torch_ops = _plans(llm, batch, sel, 23, grp_d, PromptGroups(prompts, dev), sum(tail[i] for i in order))
    _assert_same(native, torch_ops)


def _in_range(plan, n_rows_of_prompts, U):
    seg, ids, pos, last, M = plan
    assert 0 <= int(ids.min()) and int(ids.max()) < V
    assert 0 <= int(pos.min()) and int(pos.max()) < kv.PACKED_MAX_KEYS
    assert 0 <= int(last.min()) and int(last.max()) < M
    assert ids.numel() == pos.numel() == M and last.numel() == U


HOSTILE = ("rows_above", "rows_below", "zero_tail", "grp_out_of_range")


@pytest.mark.parametrize("what", HOSTILE)
@pytest.mark.parametrize("U", (2, 65, 1025))
def test_hostile_plans_equal_and_in_range(llm, U, what):
    dev = llm.device
    prompts, grp, tail, seqs, batch = _batch(3, U, TAILS["ragged"], dev, seed=U)
    tokens, starts, lengths = batch
    n_tail_rows = sum(tail)
    if what == "rows_above":
        n_tail_rows += 37
    elif what == "rows_below":
        n_tail_rows = max(U, n_tail_rows - 11)
    elif what == "zero_tail":
        lengths = lengths.clone()
        lengths[U // 2] = len(prompts[grp[U // 2]])  # a context that is its bare prompt
        lengths[0] = 0  # ... and one shorter than its prompt: a negative tail, sums that are not sorted
    else:
        grp = [g if u % 3 else (7 if u % 2 else -4) for u, g in enumerate(grp)]
    sel = torch.arange(U, dtype=torch.int32, device=dev)
    grp_d = torch.tensor(grp, dtype=torch.int32, device=dev)
    groups = PromptGroups(prompts, dev)
    native, torch_ops = _plans(llm, (tokens, starts, lengths), sel, U, grp_d, groups, n_tail_rows)
    _assert_same(native, torch_ops)
    _in_range(native, groups.n_rows, U)


@pytest.mark.parametrize("what", HOSTILE)
def test_hostile_forward_is_refused_as_today(llm, what):
    """The forward over a hostile plan: the attention kernel counts the segments it refuses in the error word - the same
    count on both plans - and raise_if_failed reports it (or nothing) on both."""
    dev, eng = llm.device, llm.engine
    U = 65
    prompts, grp, tail, seqs, batch = _batch(3, U, lambda u: 1 + u % 9, dev, seed=4)
    tokens, starts, lengths = batch
    n_tail_rows = sum(tail)
    if what == "rows_above":
        n_tail_rows += 37
    elif what == "rows_below":
        n_tail_rows -= 11
    elif what == "zero_tail":
        lengths = lengths.clone()
        lengths[U // 2] = len(prompts[grp[U // 2]])
    else:
        grp = [g if u % 3 else 7 for u, g in enumerate(grp)]
    sel = torch.arange(U, dtype=torch.int32, device=dev)
    grp_d = torch.tensor(grp, dtype=torch.int32, device=dev)
    groups = PromptGroups(prompts, dev)
    words, raised = [], []  # (the rows of a refused segment hold whatever their buffer held: not compared)
    try:
        eng.raise_if_failed(int(eng.error_word()[0].cpu()))  # (start from a clear error word)
    except Exception:  # noqa: BLE001
        pass
    for native in (False, True):
        with torch.no_grad(), kv_all_rows(eng):
            encode_packed(llm, (tokens, starts, lengths), sel, U, grp_d, groups, n_tail_rows, max_keys=17, native_plan=native)
        words.append(int(eng.error_word()[0].cpu()))
        try:
            eng.raise_if_failed(words[-1])
            raised.append(None)
        except Exception as e:  # noqa: BLE001 - whatever it raises today, both plans raise it
            raised.append(type(e))
    assert words[0] == words[1] and raised[0] == raised[1]


def kv_all_rows(eng):
    from genlm_backend_amd.fuse import split_gemm_all_rows

    return split_gemm_all_rows(eng)


def test_argument_errors(llm):
    import ctypes as C

    from genlm_backend_amd import _lib

    eng = llm.engine
    a = _lib.PackedPlanArgs()
    assert eng.lib.glb_packed_plan(None, None) == _lib.GLB_EINVAL
    a.struct_size = 8
    assert eng.lib.glb_packed_plan(C.byref(a), None) == _lib.GLB_EINVAL and "struct_size" in _lib.last_error()
    a.struct_size = C.sizeof(_lib.PackedPlanArgs)
    a.n_tokens = a.n_contexts = a.n_sel = a.n_groups = a.n_pre = a.pos_cap = 1
    assert eng.lib.glb_packed_plan(C.byref(a), None) == _lib.GLB_EINVAL  # n_tail_rows < n_sel
    a.n_tail_rows = 1
    assert eng.lib.glb_packed_plan(C.byref(a), None) == _lib.GLB_EINVAL and "null" in _lib.last_error()
