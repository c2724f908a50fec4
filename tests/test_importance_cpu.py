"""The importance-weighted step without a GPU: the float64 reference's own identities (tests/importance_ref.py), the
argument conflicts of `DeviceSIS(proposal_temperature=, proposal=)`, and the new entry points' argument errors, which
return before any launch."""
import ctypes as C

import numpy as np
import pytest

from tests import importance_ref as IR


def _rows(seed, V, kind):
    rs = np.random.default_rng(seed)
    p = (2 * rs.standard_normal(V)).astype(np.float32)
    q = (2 * rs.standard_normal(V)).astype(np.float32)
    p[rs.random(V) < 0.05] = -np.inf
    if kind == 0:
        m = np.zeros(V)
    elif kind == 1:
        m = np.where(rs.random(V) < 0.6, 0.0, -np.inf)
        m[int(rs.integers(V))] = 0.0
    else:
        m = rs.standard_normal(V).astype(np.float32).astype(np.float64)
        m[rs.random(V) < 0.3] = -np.inf
    return p, q, m


@pytest.mark.parametrize("V", [1, 37, 4097, 8200])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_weights_are_proper_for_the_target(V, kind):
    """sum_j qt(j) exp(dlogw(j)) = sum_j softmax(p)_j e^{m_j}: the identity that makes dlogw the weight."""
    for scale in (1.0, 0.5):
        p, q, m = _rows(V * 3 + kind, V, kind)
        r = IR.Row(IR.widen(p), IR.proposal_values(q, scale), m)
        d = r.dlogw()
        live = r.qt > 0
        lhs = float(np.sum(r.qt[live] * np.exp(d[live])))
        Z = r.target_mass()
        assert abs(lhs - Z) <= 1e-12 * max(1.0, Z), (lhs, Z)
        assert kind == 2 or Z <= 1.0 + 1e-12


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_proposing_from_the_target_gives_the_fused_steps_logZ(kind):
    p, _, m = _rows(11 + kind, 5000, kind)
    r = IR.Row(IR.widen(p), IR.proposal_values(p, 1.0), m)
    logZ = IR.lse(IR.widen(p) + m) - IR.lse(IR.widen(p))
    d = r.dlogw()
    live = (r.qt > 0) & np.isfinite(d)
    assert live.sum() > 100 and np.abs(d[live] - logZ).max() < 1e-12
    assert abs(r.logZ_proposal - logZ) < 1e-12


@pytest.mark.parametrize("V", [1, 33, 4096, 4097, 8200])
def test_the_two_stage_intervals_tile_the_unit_interval(V):
    p, q, m = _rows(V, V, 1)
    r = IR.Row(IR.widen(p), IR.proposal_values(q, 1.0), m)
    hi = 0.0
    for c in range(r.nch):
        lo, hi_c = r.chunk_interval(c)
        assert lo == hi or abs(lo - hi) < 1e-15
        hi = hi_c
        if r.mass[c] == 0:
            continue
        at = 0.0
        for j in range(c * IR.CHUNK, min(V, (c + 1) * IR.CHUNK)):
            a, b = r.elem_interval(j)
            assert abs(a - at) < 1e-13 and b >= a and (b > a) == (r.qt[j] > 0)
            at = b
        assert abs(at - 1.0) < 1e-12
    assert abs(hi - 1.0) < 1e-12


def test_bf16_words_and_the_scale_rounding():
    x = np.array([1.0, -2.5, 3.14159, -np.inf, 1e-3], np.float32)
    w = IR.bf16_bits(x)
    back = IR.widen(w)
    assert np.isneginf(back[3]) and np.abs(back[[0, 1]] - x[[0, 1]]).max() == 0 and abs(back[2] - 3.140625) == 0
    y = IR.proposal_values(x, 0.3)
    assert np.array_equal(y[:3], (x[:3] * np.float32(0.3)).astype(np.float64)) and np.isneginf(y[3])
    assert np.array_equal(IR.proposal_values(x, 1.0)[:3], x[:3].astype(np.float64))


def test_philox_words_are_the_librarys(oracle):
    r1, r2 = IR.philox_pair(seed=(7 << 32) | 5, offset=(9 << 32) | 3, gidx=(1 << 32) | 2)
    o = oracle.philox([2, 1, 3, 9], [5, 7])
    assert r1 == (o[1] << 32) | o[0] and r2 == (o[3] << 32) | o[2]


# ---- DeviceSIS arguments -------------------------------------------------------------------------------------------------------
def test_device_sis_argument_conflicts():
    from genlm_backend_amd.sis import DeviceSIS
    from tests.test_resample_cpu import _tiny

    llm, other = _tiny("gpt2"), _tiny("gpt2", seed=1)
    base = dict(n_particles=4, prompt_ids=[5, 6, 7], max_tokens=3, eos_id=0)
    with pytest.raises(ValueError, match="rng='philox'"):
        DeviceSIS(llm, rng="torch", proposal_temperature=2.0, **base)
    with pytest.raises(ValueError, match="rng='philox'"):
        DeviceSIS(llm, rng="torch", proposal=other, **base)
    with pytest.raises(ValueError, match="use_prefix_kv"):
        DeviceSIS(llm, proposal=other, use_prefix_kv=True, **base)
    with pytest.raises(ValueError, match="use_particle_kv"):
        DeviceSIS(llm, proposal=other, proposal_temperature=1.5, use_particle_kv=True, **base)
    with pytest.raises(ValueError, match="proposal_temperature must be > 0"):
        DeviceSIS(llm, proposal_temperature=0.0, **base)

    class OtherVocab:
        device = llm.device

        class model:
            class config:
                vocab_size = 301

    with pytest.raises(ValueError, match="another vocabulary: 301 tokens, the target 300"):
        DeviceSIS(llm, proposal=OtherVocab(), **base)
    # neither argument: today's object, no proposal state
    s = DeviceSIS(llm, **base)
    assert s._propose is False and s.proposal is None


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def _valid_block(_lib):
    """An argument block that passes every check (the pointers are never followed: these tests stop before a launch)."""
    a = _lib.ImportanceArgs()
    a.struct_size = C.sizeof(_lib.ImportanceArgs)
    a.target, a.target_dtype, a.ld_p = 0x10000, _lib.F32, 64
    a.n_rows, a.vocab, a.n_particles = 2, 50, 2
    a.proposal_scale = 1.0
    a.workspace, a.workspace_bytes = 0x20000, 0
    return a


def test_importance_entry_points_reject_bad_arguments_before_any_launch():
    from genlm_backend_amd import _lib

    lib = _lib.load()
    assert C.sizeof(_lib.ImportanceArgs) == 216  # layout guard (sizeof in C, include/glb.h compiled with gcc)
    assert lib.glb_importance_workspace_bytes(1024, 700, 50257) == 1024 * 13 * 64
    assert lib.glb_importance_workspace_bytes(3, 65, 4096) == 65 * 64
    assert lib.glb_importance_workspace_bytes(0, 1, 1) == 0 and lib.glb_importance_workspace_bytes(1, 1, 0) == 0
    call = lambda a: lib.glb_importance_step(C.byref(a), None)
    assert lib.glb_importance_step(None, None) == _lib.GLB_EINVAL
    a = _valid_block(_lib)
    a.struct_size = 1
    assert call(a) == _lib.GLB_EINVAL and "struct_size" in _lib.last_error()
    # a block that is right except for its workspace: too small is GLB_ENOSPC, and the last check made
    a = _valid_block(_lib)
    assert call(a) == _lib.GLB_ENOSPC and "workspace" in _lib.last_error()
    bad = [("target", 0, "target is null"), ("target_dtype", 3, "target_dtype"), ("target_dtype", -1, "target_dtype"),
           ("ld_p", 49, "ld_p"), ("vocab", 0, "positive"), ("n_rows", 0, "positive"), ("n_particles", 0, "positive"),
           ("n_particles", 3, "row_of"), ("vocab", 1 << 31, "31 bits"), ("proposal_scale", float("nan"), "NaN"),
           ("mask_kind", _lib.MASK_PREPARED, "GLB_MASK_PREPARED"), ("mask_kind", 4, "mask_kind"), ("mask_kind", -1, "mask_kind"),
           ("workspace", 0, "workspace is null"), ("workspace", 0x20008, "aligned"), ("target", 0x10002, "aligned")]
    for field, value, word in bad:
        a = _valid_block(_lib)
        setattr(a, field, value)
        if field == "vocab" and value > 64:
            a.ld_p = value
        assert call(a) == _lib.GLB_EINVAL, field
        assert word in _lib.last_error(), (field, _lib.last_error())
    # fields of a proposal that is not given are not read; given, they are
    a = _valid_block(_lib)
    a.proposal_dtype, a.ld_q = 77, -5
    assert call(a) == _lib.GLB_ENOSPC
    a.proposal = 0x30000
    assert call(a) == _lib.GLB_EINVAL and "proposal_dtype" in _lib.last_error()
    a.proposal_dtype = _lib.BF16
    assert call(a) == _lib.GLB_EINVAL and "ld_q" in _lib.last_error()
    a.ld_q = 50
    assert call(a) == _lib.GLB_ENOSPC
    # mask fields are read only with a mask
    a = _valid_block(_lib)
    a.mask_ld, a.n_masks, a.mask_id, a.row_mask_id = -1, -1, 0x40000, 0x50000
    assert call(a) == _lib.GLB_ENOSPC
    a.mask_kind = _lib.MASK_BITS
    assert call(a) == _lib.GLB_EINVAL and "mask table missing" in _lib.last_error()
    a.mask, a.n_masks, a.mask_ld = 0x60000, 2, 1
    assert call(a) == _lib.GLB_EINVAL and "mask_ld" in _lib.last_error()
    a.mask_ld = 2
    assert call(a) == _lib.GLB_EINVAL and "not both" in _lib.last_error()
    a.mask_id = None
    assert call(a) == _lib.GLB_ENOSPC
    a.row_mask_id, a.n_masks = None, 3
    assert call(a) == _lib.GLB_EINVAL and "neither 1 nor" in _lib.last_error()
    a.mask_kind, a.mask_ld = _lib.MASK_F32, 49
    assert call(a) == _lib.GLB_EINVAL and "mask_ld" in _lib.last_error()
