"""The fused step's mask sources (genlm-backend_amd/masks.py, constraints.DeviceConstraint.step_masks) on the CPU test
doubles: what each hands to `HipEngine.step`, and that all three answer the same call."""
import types

import numpy as np
import pytest
import torch

import genlm_backend_amd  # noqa: F401
from genlm_backend_amd._lib import MASK_BITS, MASK_F32, MASK_NONE
from genlm_backend_amd.masks import ParticleMasks, RegisteredMasks
from tests.cpu_engine import CpuOracleEngine, _Prepared

V = 70


class CountingEngine(CpuOracleEngine):
    def __init__(self):
        self.prepared, self.updated = [], []

    def prepare_masks(self, bits, vocab, logits_dtype=torch.float32):
        self.prepared.append((vocab, logits_dtype))
        return super().prepare_masks(bits, vocab, logits_dtype)

    def update_prepared_masks(self, prepared, bits, rows):
        self.updated.append(sorted(rows.tolist()))
        return super().update_prepared_masks(prepared, bits, rows)


def _binary(k, seed=0):
    m = torch.where(torch.rand((k, V), generator=torch.Generator().manual_seed(seed)) < 0.5, float("-inf"), 0.0)
    m[:, 0] = 0.0
    return m


def _logits(dtype=torch.float32, rows=3):
    return torch.zeros((rows, V), dtype=dtype)


def test_registered_masks_nothing_registered_gives_no_keywords():
    src = RegisteredMasks(CountingEngine())
    assert src.kind == MASK_NONE and src.tables(torch.float32) == {}
    assert src.step_masks(_logits(), None, False, 4) == ({}, False)
    assert src.step_masks(_logits(), torch.zeros(3, dtype=torch.int32), True, 4) == ({}, False)


def test_registered_binary_masks_become_bit_rows_prepared_once_per_element_width():
    eng = CountingEngine()
    src = RegisteredMasks(eng)
    masks = _binary(2)
    src.register(masks)
    assert src.kind == MASK_BITS and src.vocab == V
    assert torch.equal(src.table, eng.mask_to_bits(masks)[0])
    ids = torch.tensor([0, 1, 0], dtype=torch.int32)
    for dtype in (torch.float32, torch.bfloat16, torch.float32, torch.float16, torch.bfloat16):
        kw, raw = src.step_masks(_logits(dtype), ids, False, 3)
        assert not raw and list(kw) == ["mask", "mask_id"] and isinstance(kw["mask"], _Prepared) and kw["mask_id"] is ids
        assert torch.equal(kw["mask"].bits, src.table)
    assert eng.prepared == [(V, torch.float32), (V, torch.bfloat16)]  # one form for float32 rows, one for the 16-bit ones
    src.register(_binary(2, seed=1))  # new tables: prepared again
    src.step_masks(_logits(), ids, False, 3)
    assert len(eng.prepared) == 3


def test_registered_masks_with_a_finite_weight_stay_float():
    eng = CountingEngine()
    src = RegisteredMasks(eng)
    masks = _binary(2)
    masks[1, 5] = -0.25
    src.register(masks)
    ids = torch.tensor([1, 0, 1], dtype=torch.int32)
    kw, raw = src.step_masks(_logits(torch.bfloat16), ids, True, 5)
    assert raw and src.kind == MASK_F32 and eng.prepared == []
    assert list(kw) == ["mask_kind", "mask", "row_mask_id"] and kw["mask_kind"] == MASK_F32 and kw["mask"] is masks


def test_particle_masks_raw_or_prepared():
    """The sequence tests/test_host_cpu.py drives through `DeviceSIS`, on the object itself: a tensor state seen for the first
    time goes raw, seen again it is prepared; few changed rows are prepared again, many make the step raw while the prepared
    form lags, a step before which nothing moved brings it up to date; `raw_above = 1.0` and the parity draw never go raw."""
    N = 40
    g = torch.Generator().manual_seed(11)
    eng = CountingEngine()
    rows = lambda n: eng.mask_to_bits(torch.where(torch.rand((n, V), generator=g) < 0.5, float("-inf"), 0.0))[0]
    pm0 = rows(N + 1)
    script = [None, None, 3, 30, 2, None, N, 1]  # rows moved before each step (float32 rows: raw above a quarter = 10)
    edits = [None if e is None else (torch.randperm(N, generator=g)[:e].to(torch.int32), rows(e)) for e in script]
    ids = torch.arange(N, dtype=torch.int32)
    kinds = {}
    for above, parity in ((None, False), (1.0, False), (None, True)):
        eng.prepared, eng.updated = [], []
        src = ParticleMasks(eng, N, pm0.clone())
        src.raw_above = above
        kinds[above, parity] = []
        for e in edits:
            if e is not None:
                src.update(*e)
            kw, raw = src.step_masks(_logits(rows=N), ids, False, N, parity=parity)
            kinds[above, parity].append(raw)
            assert kw["mask_id"] is ids and list(kw) == (["mask_kind", "mask", "mask_id"] if raw else ["mask", "mask_id"])
            if raw:
                assert kw["mask_kind"] == MASK_BITS and kw["mask"] is src.masks
            else:  # the prepared form is up to date with every row
                assert torch.equal(kw["mask"].bits, src.masks)
        assert src.raw_steps == sum(kinds[above, parity])
        if above is None and not parity:
            # prepared at step 1; steps 2 and 5 bring the rows named since up to date (3; then 30 + 2, one call)
            assert eng.prepared == [(V, torch.float32)] and [len(u) for u in eng.updated] == [3, len(set(edits[3][0].tolist()) | set(edits[4][0].tolist()))]
        src.reset()
        assert src._prepared is None and src._dirty is None and src._seen is None and not src._moved
    assert kinds[None, False] == [True, False, False, True, True, False, True, True]
    assert kinds[1.0, False] == [False] * len(script) and kinds[None, True] == [False] * len(script)


def test_particle_masks_written_behind_its_back_are_prepared_again():
    eng = CountingEngine()
    src = ParticleMasks(eng, 4, eng.mask_to_bits(_binary(5))[0])
    src.raw_above = 1.0
    ids, x = torch.arange(4, dtype=torch.int32), _logits(rows=4)
    src.step_masks(x, ids, False, 4)
    src.step_masks(x, ids, False, 4)
    assert len(eng.prepared) == 1
    src.masks[2] = 0  # in place, untold: the version counter moves
    kw, _ = src.step_masks(x, ids, False, 4)
    assert len(eng.prepared) == 2 and torch.equal(kw["mask"].bits, src.masks)
    src.masks = src.masks.clone()  # rebound
    src.step_masks(x, ids, False, 4)
    assert len(eng.prepared) == 3 and eng.updated == []


def _constraint(weighted):
    """A `DeviceConstraint` over a stub engine that records the library calls (no device: the CU count is given)."""
    from genlm_backend_amd.constraints import ByteDFA, ByteWFSA, DeviceConstraint

    class StubEngine(CountingEngine):
        def __init__(self):
            super().__init__()
            self.calls = []
            self.lib = types.SimpleNamespace(glb_dfa_bank_rows=lambda b, v, s: min(s + 2, b // (4 * ((v + 31) // 32))),
                                             glb_dfa_weight_bank_rows=lambda b, v, s: min(s + 2, b // (4 * ((v + 63) // 64 * 64))))

        def dfa_call(self, name, args):
            self.calls.append((name, type(args).__name__))

    dfa = ByteDFA.from_strings([b"ab", b"b"])
    eng = StubEngine()
    c = DeviceConstraint(eng, ByteWFSA.from_dfa(dfa) if weighted else dfa, [bytes([97 + i % 3]) for i in range(V)], eos_id=0, skip_ids=())
    c._cus = 256
    return c, eng


@pytest.mark.parametrize("weighted", [False, True])
def test_device_constraint_calls_its_bank_kind_decided_once(weighted):
    c, eng = _constraint(weighted)
    assert c.bank.dtype == (torch.float32 if weighted else torch.int32) and c.bank.shape == (c.dfa.n_states + 2, 128 if weighted else 3)
    c._claim_and_fill(c.states0(4))
    block = "DfaWeightArgs" if weighted else "DfaArgs"
    assert eng.calls == [("glb_dfa_weight_bank_init" if weighted else "glb_dfa_bank_init", block), ("glb_dfa_claim_rows", "DfaArgs"),
                         ("glb_dfa_fill_weights" if weighted else "glb_dfa_fill_masks", block)]
    ids = torch.tensor([2, 0, 1, 2], dtype=torch.int32)
    kw, raw = c.step_masks(_logits(), ids, False, 4, parity=False)
    if weighted:  # a float bank is read where it lies
        assert raw and kw["mask_kind"] == MASK_F32 and kw["mask"] is c.bank and kw["mask_id"] is ids
    else:  # few units: their rows gathered, each unit its own
        assert not raw and kw["mask_kind"] == MASK_BITS and torch.equal(kw["mask"], c.bank[ids.long(), :c.words])
        assert kw["mask_id"].tolist() == [0, 1, 2, 3]
        many = torch.zeros(600, dtype=torch.int32)
        kw, raw = c.step_masks(_logits(), many, True, 600)  # more than 512 (unit, chunk) items: the bank itself
        assert raw and kw["mask"] is c.bank and kw["row_mask_id"] is many
        assert not c.step_masks(_logits(), many, True, 600, parity=True)[1]  # the parity race is two launches: gathered


@pytest.mark.parametrize("by_row", [False, True])
def test_every_source_names_exactly_one_kind_of_ids(by_row):
    eng = CountingEngine()
    reg_bits, reg_f32 = RegisteredMasks(eng), RegisteredMasks(eng)
    reg_bits.register(_binary(2))
    soft = _binary(2)
    soft[0, 1] = -1.5
    reg_f32.register(soft)
    particle = ParticleMasks(eng, 4, eng.mask_to_bits(_binary(5))[0])
    ids = torch.tensor([0, 1, 1, 0], dtype=torch.int32)
    want, other = ("row_mask_id", "mask_id") if by_row else ("mask_id", "row_mask_id")
    for src in (reg_bits, reg_f32, particle, particle, _constraint(False)[0], _constraint(True)[0]):  # (particle: raw, then prepared)
        for parity in (False, True):
            kw, raw = src.step_masks(_logits(rows=4), ids, by_row, 4, parity=parity)
            assert want in kw and other not in kw and "mask" in kw and isinstance(raw, bool)
            assert set(kw) <= {"mask_kind", "mask", "mask_id", "row_mask_id"}
            assert np.array_equal(kw[want].numpy(), ids.numpy()) or src.__class__.__name__ == "DeviceConstraint"
