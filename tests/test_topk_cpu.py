"""Top-k rows and beam selection without a GPU: the layout of `glb_topk_args`, the argument errors of glb_topk_rows and
glb_beam_select (they return before any launch), `DeviceBeam`'s argument errors, and the reference (tests/topk_ref.py)
against hand-made examples."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import topk_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_topk_args_layout_matches_the_header(tmp_path):
    from genlm_backend_amd import _lib

    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "glb.h"\nint main(void) { printf("%zu %zu %d\\n", '
                   'sizeof(glb_topk_args), offsetof(glb_topk_args, out_logZ), GLB_ABI_VERSION); return 0; }\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "size")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "size")]).split()]
    assert out == [C.sizeof(_lib.TopkArgs), _lib.TopkArgs.out_logZ.offset, 9]
    assert _lib.ABI_VERSION == 9
    lib = _lib.load()
    assert lib.glb_abi_version() == 9
    for name in ("glb_topk_rows", "glb_beam_select"):
        assert name in _lib.SYMBOLS and getattr(lib, name)


def _valid_block(_lib):
    """An argument block that passes every check (these tests stop before a launch: the pointers are never followed)."""
    a = _lib.TopkArgs()
    a.struct_size = C.sizeof(_lib.TopkArgs)
    a.logits, a.dtype, a.ld = 0x10000, _lib.F32, 64
    a.n_rows, a.vocab, a.logit_scale, a.k = 2, 50, 1.0, 4
    a.out_token = 0x20000
    return a


def test_topk_rows_rejects_bad_arguments_before_any_launch():
    from genlm_backend_amd import _lib

    lib = _lib.load()
    call = lambda a: lib.glb_topk_rows(C.byref(a), None)
    assert lib.glb_topk_rows(None, None) == _lib.GLB_EINVAL
    bad = [("struct_size", 1, "struct_size"), ("logits", 0, "logits is null"), ("out_token", 0, "out_token is null"),
           ("k", 0, "k 0 outside"), ("k", 65, "k 65 outside"), ("k", -1, "outside"), ("dtype", 3, "dtype"),
           ("dtype", -1, "dtype"), ("n_rows", 0, "positive"), ("vocab", 0, "positive"), ("n_rows", -1, "positive"),
           ("vocab", 1 << 31, "31 bits"), ("n_rows", 1 << 31, "31 bits"), ("ld", 49, "ld"), ("logits", 0x10002, "aligned"),
           ("logit_scale", float("nan"), "NaN"), ("logit_scale", 0.0, "positive and finite"),
           ("logit_scale", -1.0, "positive and finite"), ("logit_scale", float("inf"), "positive and finite"),
           ("mask_kind", _lib.MASK_PREPARED, "GLB_MASK_PREPARED"), ("mask_kind", 4, "mask_kind"), ("mask_kind", -1, "mask_kind")]
    for field, value, word in bad:
        a = _valid_block(_lib)
        setattr(a, field, value)
        if field == "vocab" and value > 64:
            a.ld = value
        assert call(a) == _lib.GLB_EINVAL, field
        assert word in _lib.last_error(), (field, _lib.last_error())
    # with a mask: the table, its pitch, the ids
    a = _valid_block(_lib)
    a.mask_kind = _lib.MASK_BITS
    assert call(a) == _lib.GLB_EINVAL and "mask table missing" in _lib.last_error()
    a.mask, a.n_masks, a.mask_ld = 0x60000, 3, 1
    assert call(a) == _lib.GLB_EINVAL and "mask_ld" in _lib.last_error()
    a.mask_ld = 2
    assert call(a) == _lib.GLB_EINVAL and "neither 1 nor" in _lib.last_error()
    a.mask = 0x60002
    a.n_masks = 2
    assert call(a) == _lib.GLB_EINVAL and "misaligned" in _lib.last_error()
    a.mask, a.mask_kind, a.mask_ld = 0x60000, _lib.MASK_F32, 49
    assert call(a) == _lib.GLB_EINVAL and "mask_ld" in _lib.last_error()
    a.n_masks, a.mask_ld = 0, 50
    assert call(a) == _lib.GLB_EINVAL and "mask table missing" in _lib.last_error()
    a.n_masks, a.mask_ld = 1 << 31, 50
    assert call(a) == _lib.GLB_EINVAL and "neither 1 nor" in _lib.last_error()
    a.row_mask_id = 0x70000
    assert call(a) == _lib.GLB_EINVAL and "n_masks exceeds" in _lib.last_error()


def test_beam_select_rejects_bad_arguments_before_any_launch():
    from genlm_backend_amd import _lib

    lib = _lib.load()
    good = dict(score=0x10000, alive=0x20000, cand_token=0x30000, cand_logp=0x40000, n_groups=2, width=4, k=4, out_parent=0x50000,
                out_token=0x60000, out_score=0x70000)
    order = list(good)
    bad = [(f, None, "null") for f in order if f not in ("n_groups", "width", "k")]
    bad += [("width", 0, "width 0 outside"), ("width", 65, "width 65 outside"), ("width", -3, "outside"), ("k", 0, "k 0 outside"),
            ("k", 65, "k 65 outside"), ("n_groups", 0, "n_groups"), ("n_groups", -1, "n_groups"), ("n_groups", 1 << 19, "n_groups")]
    for field, value, word in bad:
        args = dict(good)
        args[field] = value
        assert lib.glb_beam_select(*[args[f] for f in order], None) == _lib.GLB_EINVAL, field
        assert word in _lib.last_error(), (field, _lib.last_error())


def test_device_beam_argument_errors():
    from genlm_backend_amd import DeviceBeam

    for kw, word in ((dict(width=0), "width"), (dict(width=65), "width"), (dict(width=2.0), "width"), (dict(k=0), "k must"),
                     (dict(k=65), "k must"), (dict(max_tokens=0), "max_tokens"), (dict(temperature=0.0), "temperature"),
                     (dict(prompt_ids=[]), "no prompt"), (dict(prompt_ids=[[1], []]), "at least one token")):
        args = dict(llm=None, width=4, prompt_ids=[1, 2], max_tokens=3, eos_id=0)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            DeviceBeam(**args)
    for name in ("rng", "proposal", "rank", "world", "dist", "seed"):  # nothing is drawn, nothing is spread over ranks
        with pytest.raises(TypeError, match=name):
            DeviceBeam(None, 4, [1, 2], 3, 0, **{name: None})


# ---- the reference's own identities --------------------------------------------------------------------------------------------
def test_reference_rows():
    x = np.array([[0.0, 1.0, -np.inf, 2.0, 1.0], [-np.inf] * 5, [-0.0, -1.0, 0.0, -np.inf, -2.0]], np.float32)
    r = TR.topk_rows(x, 3)
    l = np.log(1 + 2 * np.e + np.e ** 2)
    assert r["token"].tolist() == [[3, 1, 4], [-1, -1, -1], [0, 2, 1]]  # equal keys by lower index; -0 equals +0
    assert np.allclose(r["logp"][0], [2 - l, 1 - l, 1 - l], atol=1e-12) and abs(r["lse"][0] - l) < 1e-12 and r["logZ"][0] == 0.0
    assert np.all(np.isneginf(r["logp"][1])) and r["lse"][1] == -np.inf and r["logZ"][1] == -np.inf
    bits = np.array([[0b10110], [0]], np.uint32)
    r = TR.topk_rows(x[:1], 4, 1.0, 1, bits, [0])
    lz = np.log(np.e + np.e)  # tokens 1, 2 (-inf) and 4
    assert r["token"].tolist() == [[1, 4, -1, -1]]
    assert np.allclose(r["logp"][0, :2], [1 - l, 1 - l], atol=1e-12) and np.all(np.isneginf(r["logp"][0, 2:]))
    assert np.allclose(r["logp_masked"][0, :2], [1 - lz] * 2, atol=1e-6) and abs(r["logZ"][0] - (lz - l)) < 1e-6
    assert TR.topk_rows(x[:1], 2, 1.0, 1, bits, [1])["token"].tolist() == [[-1, -1]]  # the empty mask
    assert TR.topk_rows(x[:1], 2, 1.0, 1, bits, [5])["token"].tolist() == [[-1, -1]]  # an id out of range
    w = np.array([[0.5, -np.inf, 0.0, -3.0, 1.0]], np.float32)
    r = TR.topk_rows(x[:1], 5, 0.5, 2, w)  # keys 0.5, -inf, -inf, -2, 1.5
    assert r["token"].tolist() == [[4, 0, 3, -1, -1]]
    assert abs(r["logp"][0, 0] - (1.5 - np.log(1 + 2 * np.exp(0.5) + np.e))) < 1e-6


def test_reference_beam_step_by_hand():
    """Three beams, k = 2.  Beam 0 is finished at -1.0 and outranks every live candidate but one; beams 1 and 2 are alive:
    (1, 0) = -0.5 - 0.25 = -0.75, (1, 1) = -0.5 - 1.0 = -1.5, (2, 0) = -1.0 - 0.5 = -1.5 (a tie with (1, 1): the lower
    (b, j) first), (2, 1): token -1, not a candidate."""
    score = np.array([-1.0, -0.5, -1.0], np.float32)
    alive = np.array([0, 1, 1], np.int32)
    tok = np.array([[7, 8], [3, 4], [5, -1]], np.int32)
    lp = np.array([[-0.1, -0.2], [-0.25, -1.0], [-0.5, -0.75]], np.float32)
    parent, token, out = TR.beam_select(score, alive, tok, lp, 3)
    assert parent.tolist() == [1, 0, 1] and token.tolist() == [3, -1, 4] and out.tolist() == [-0.75, -1.0, -1.5]
    # one more slot than candidates; a beam at -inf gives nothing; a -inf candidate value is none
    score = np.array([-np.inf, -0.5, -1.0, -2.0], np.float32)
    alive = np.array([1, 1, 0, 1], np.int32)
    tok = np.array([[1, 2], [3, 4], [5, 6], [7, 8]], np.int32)
    lp = np.array([[-0.1, -0.2], [-0.25, -np.inf], [-0.5, -0.75], [-0.5, -0.5]], np.float32)
    parent, token, out = TR.beam_select(score, alive, tok, lp, 4)
    assert parent.tolist() == [1, 2, 3, 3] and token.tolist() == [3, -1, 7, 8] and out.tolist() == [-0.75, -1.0, -2.5, -2.5]
    parent, token, out = TR.beam_select(score[:2], alive[:2], tok[:2], lp[:2], 2)
    assert parent.tolist() == [1, -1] and token.tolist() == [3, -1] and out.tolist() == [-0.75, -np.inf]
