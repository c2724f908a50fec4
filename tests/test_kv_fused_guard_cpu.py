"""The host path of a fused KV forward (kv.py) without a GPU and without the native library: which
kernel a forward reaches, that the kernel asked for is the kernel called, and the guards around a body that tampers with the
slab's tensors, bypasses the attention entry or raises."""
from types import SimpleNamespace

import pytest
import torch

from genlm_backend_amd import kv

LAYERS, ROWS, CAP, HEADS, DH = 2, 3, 8, 2, 16
KERNELS = ("slab_attention", "slab_attention_chunk", "slab_attention_tile")


class _OnGpu(torch.Tensor):
    """A CPU tensor that says it is on the GPU: all the predicate asks of the slabs' device."""
    is_cuda = True


class FakeEngine:
    """Records the kernel calls (`calls`) and the `_supports` questions (`asked`); zeros of the kernels' output shapes."""

    def __init__(self, unsupported=()):
        self.calls, self.asked, self.unsupported = [], [], unsupported

    def slab_attention(self, query, k_new, v_new, k_slab, v_slab, pos, scale):
        self.calls.append(("slab_attention", dict(pos=pos, n_new=None, rows=None)))
        return torch.zeros((query.shape[0], 1, query.shape[1], query.shape[3]))

    def _chunk_shaped(self, name, query, pos, n_new, rows):
        self.calls.append((name, dict(pos=pos, n_new=n_new, rows=rows)))
        n, H, T, Dh = query.shape
        return torch.zeros((n, T, H, Dh))

    def slab_attention_chunk(self, query, k_new, v_new, k_slab, v_slab, pos, n_new, scale, rows=None):
        return self._chunk_shaped("slab_attention_chunk", query, pos, n_new, rows)

    def slab_attention_tile(self, query, k_new, v_new, k_slab, v_slab, pos, n_new, scale, rows=None):
        return self._chunk_shaped("slab_attention_tile", query, pos, n_new, rows)

    def _supports(self, name, dtype, head_dim):
        self.asked.append(name)
        return name not in self.unsupported and dtype == torch.float32 and head_dim == DH


for _name in KERNELS:
    setattr(FakeEngine, _name + "_supports", lambda self, dtype, head_dim, _n=_name: self._supports(_n, dtype, head_dim))


class Body:
    """A transformer body reduced to what the guards see: every layer hands its new K / V to the cache and then calls the
    attention entry.  skip: layers that do not call it; boom: the layer that raises between the two; tamper: "key" / "value"
    pass a copy of that tensor on, "query" two query positions."""

    def __init__(self, engine, skip=(), boom=None, tamper=None):
        self.config = SimpleNamespace(_attn_implementation="glb", _glb_engine=engine)
        self.skip, self.boom, self.tamper = skip, boom, tamper

    def modules(self):
        return []

    def __call__(self, input_ids, position_ids, attention_mask, past_key_values, use_cache):
        assert attention_mask is None and use_cache
        n, T = input_ids.shape
        for i, layer in enumerate(past_key_values.layers):
            k_new, v_new = torch.zeros((2, n, HEADS, T, DH)).unbind(0)
            keys, values = layer.update(k_new, v_new)
            if i == self.boom:
                raise KeyError("the body's own failure")
            if i in self.skip:
                continue
            if self.tamper == "key":  # (tagged like the slab: an untagged tensor is none of the entry's business)
                keys = keys.clone()
                keys._glb_layer = layer
            if self.tamper == "value":
                values = values.clone()
            query = torch.zeros((n, HEADS, 2 if self.tamper == "query" else T, DH))
            out, _ = kv._glb_attention_forward(self, query, keys, values, None)
            assert out.shape == (n, query.shape[2], HEADS, DH)
        return SimpleNamespace(last_hidden_state=torch.zeros((n, T, 4)))


def _slabs(cls, engine, on_gpu=True):
    pkv = cls(engine, ROWS, CAP, LAYERS)
    for layer in pkv.layers:
        layer.lazy_initialization(*torch.zeros((2, 1, HEADS, 1, DH)).unbind(0))
        if on_gpu:
            layer.keys, layer.values = layer.keys.as_subclass(_OnGpu), layer.values.as_subclass(_OnGpu)
    return pkv


def _in_place(cls, engine, **body):
    """(the in-place forward over fresh slabs, its ids and positions)"""
    fwd = kv.SlabForward(_slabs(cls, engine), Body(engine, **body), graph=False)
    return fwd, torch.zeros((ROWS, 1), dtype=torch.int64), torch.tensor([0, 3, 7], dtype=torch.int32)


def _chunk(engine, T, **body):
    """(the runner over fresh shared slabs, the plan of a chunk forward of up to T tokens over rows 2 and 0, `_run_chunk`'s
    arguments)"""
    llm = SimpleNamespace(engine=engine, _body=Body(engine, **body), device=torch.device("cpu"))
    runner = kv.SlabRunner(llm, ROWS, CAP, graph=False)
    runner.pkv = _slabs(kv.SharedSlabKV, engine)
    plan = {"rows_a": torch.tensor([1, 2, 0], dtype=torch.int32), "pos_a": torch.tensor([5, 0, 3], dtype=torch.int32),
            "n_new_a": torch.tensor([1, T, max(1, T // 2)], dtype=torch.int32), "ctx_a": torch.tensor([0, 1, 2], dtype=torch.int32)}
    return runner, plan, (plan, 1, 3, T, lambda ctx, at: ctx * 100 + at, 0)


def _assert_clean(pkv):
    assert pkv.fused_attention is False
    assert all(layer._new_k is None and layer._new_v is None for layer in pkv.layers)


@pytest.mark.parametrize("cls", [kv.SlabKV, kv.SharedSlabKV])
def test_in_place_forward_reaches_slab_attention(cls):
    eng = FakeEngine()
    fwd, ids, pos = _in_place(cls, eng)
    assert fwd.fused and fwd._run(ids, pos).shape == (ROWS, 4)
    assert [name for name, _ in eng.calls] == ["slab_attention"] * LAYERS
    assert all(rec["pos"] is pos for _, rec in eng.calls)
    _assert_clean(fwd.pkv)


@pytest.mark.parametrize("T,name", [(1, "slab_attention_chunk"), (kv.CHUNK_KERNEL_MAX, "slab_attention_chunk"),
                                    (kv.CHUNK_KERNEL_MAX + 1, "slab_attention_tile")])
def test_chunk_forward_reaches_the_kernel_of_its_width(T, name):
    eng = FakeEngine()
    runner, plan, args = _chunk(eng, T)
    assert runner._run_chunk(*args).shape == (2, 4)
    assert [called for called, _ in eng.calls] == [name] * LAYERS
    for _, rec in eng.calls:  # what set_forward_chunk was given: rows lo .. hi - 1 of the plan
        assert rec["rows"] is runner.pkv.rows and rec["pos"] is runner.pkv.pos
        for key in ("rows", "pos", "n_new"):
            assert torch.equal(rec[key], plan[key + "_a"][1:3])
    _assert_clean(runner.pkv)
    assert runner.pkv.n_new is None


def test_the_kernel_asked_for_is_the_kernel_called():
    for T in range(1, 129):
        eng = FakeEngine()
        runner, _, args = _chunk(eng, T)
        assert runner._chunk_fused(T)
        asked, eng.asked = eng.asked, []
        runner._run_chunk(*args)
        assert len(asked) == 1 and eng.asked == asked and {name for name, _ in eng.calls} == set(asked), T


def test_tampered_tensors_are_refused():
    eng = FakeEngine()
    for tamper in ("key", "value", "query"):
        fwd, ids, pos = _in_place(kv.SharedSlabKV, eng, tamper=tamper)
        with pytest.raises(RuntimeError, match="glb_slab_attention: .* never appended"):
            fwd._run(ids, pos)
        _assert_clean(fwd.pkv)
    for tamper in ("key", "value"):
        runner, _, args = _chunk(eng, 4, tamper=tamper)
        with pytest.raises(RuntimeError, match="glb_slab_attention_chunk: .* never appended"):
            runner._run_chunk(*args)
        _assert_clean(runner.pkv)
        assert runner.pkv.n_new is None
    assert not eng.calls


@pytest.mark.parametrize("T", [None, 4, kv.CHUNK_KERNEL_MAX + 1])  # None: the in-place forward
def test_a_layer_that_bypasses_the_entry_is_named(T):
    eng = FakeEngine()
    if T is None:
        fwd, ids, pos = _in_place(kv.SlabKV, eng, skip=(1,))
        pkv, run = fwd.pkv, lambda: fwd._run(ids, pos)
    else:
        runner, _, args = _chunk(eng, T, skip=(1,))
        pkv, run = runner.pkv, lambda: runner._run_chunk(*args)
    with pytest.raises(RuntimeError, match=r"was not reached in layers \[1\]"):
        run()
    assert len(eng.calls) == 1  # layer 0 was served
    _assert_clean(pkv)
    assert getattr(pkv, "n_new", None) is None


@pytest.mark.parametrize("T", [None, 4])
def test_a_body_that_raises_leaves_the_slabs_clean(T):
    eng = FakeEngine()
    if T is None:
        fwd, ids, pos = _in_place(kv.SharedSlabKV, eng, boom=1)
        pkv, run = fwd.pkv, lambda: fwd._run(ids, pos)
    else:
        runner, _, args = _chunk(eng, T, boom=1)
        pkv, run = runner.pkv, lambda: runner._run_chunk(*args)
    with pytest.raises(KeyError, match="the body's own failure"):
        run()
    _assert_clean(pkv)
    assert pkv.n_new is None


def test_when_a_kernel_may_serve_the_slabs():
    eng = FakeEngine()
    pkv, body = _slabs(kv.SharedSlabKV, eng), Body(eng)
    for name in KERNELS:
        assert kv._kernel_serves(eng, name, pkv, body) is True
        assert kv._kernel_serves(eng, name, _slabs(kv.SharedSlabKV, eng, on_gpu=False), body) is False  # slabs on the CPU
        assert kv._kernel_serves(eng, name, pkv, Body(FakeEngine())) is False                          # another engine's body
        assert kv._kernel_serves(FakeEngine(unsupported=(name,)), name, pkv, body) is False             # a form that is not built
        assert kv._kernel_serves(eng, name, kv.SharedSlabKV(eng, ROWS, CAP, LAYERS), body) is False     # no slabs yet
    bare = SimpleNamespace()
    assert kv._kernel_serves(bare, "slab_attention_tile", pkv, Body(bare)) is False  # an engine without the method
    body.config._attn_implementation = "sdpa"
    assert kv._kernel_serves(eng, "slab_attention", pkv, body) is False
    # ... and its two users: SlabForward.fused, SlabRunner._chunk_fused
    assert not kv.SlabForward(pkv, body, graph=False).fused and kv.SlabForward(pkv, Body(eng), graph=False).fused
    assert not kv.SlabForward(pkv, Body(eng), graph=False, fused_attention=False).fused
    no_tile = FakeEngine(unsupported=("slab_attention_tile",))
    runner = _chunk(no_tile, 4)[0]
    assert runner._chunk_fused(kv.CHUNK_KERNEL_MAX) and not runner._chunk_fused(kv.CHUNK_KERNEL_MAX + 1)
