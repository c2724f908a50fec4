"""Truncated sampling without a GPU: the reference of glb_truncate_rows (tests/truncate_ref.py) against a literal composition
of the common samplers' warpers in torch float64, the layout of `glb_truncate_args`, and the samplers' new keywords."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import truncate_ref as TQ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _warpers(key, top_k, top_p, min_p):
    """(keep bool [V], margin): top-k, top-p and min-p warpers applied in sequence to float64 scores, each on the softmax of
    what the one before left (sort, softmax, cumsum as the transformers library writes them).  The one stated difference: the
    tokens that equal the smallest kept score are kept too.  margin: the distance from top_p to the nearest cumulative
    probability."""
    s = torch.from_numpy(np.asarray(key, np.float64)).clone()
    margin = np.inf
    if top_k > 0:
        kth = torch.topk(s, min(top_k, s.numel()))[0][-1]
        s = s.masked_fill(s < kth, -np.inf)
    if top_p < 1.0:
        srt, idx = torch.sort(s, descending=False)
        cum = srt.softmax(dim=-1).cumsum(dim=-1)
        remove = cum <= 1.0 - top_p
        remove[-1] = False
        margin = float((cum - (1.0 - top_p)).abs().min())
        s = s.masked_fill(torch.zeros_like(remove).scatter(0, idx, remove), -np.inf)
    if min_p > 0.0:
        pr = s.softmax(dim=-1)
        s = s.masked_fill(pr < min_p * pr.max(), -np.inf)
    keep = torch.isfinite(s)
    keep |= torch.from_numpy(np.asarray(key, np.float64)) == s[keep].min()
    return keep.numpy(), margin


@pytest.mark.parametrize("sigma", [1.0, 3.0, 6.0])
@pytest.mark.parametrize("opts", [dict(top_k=50), dict(top_p=0.9), dict(top_p=0.5), dict(min_p=0.05), dict(top_k=5, top_p=0.8, min_p=0.05),
                                  dict(top_k=1000, top_p=0.95), dict(top_k=1), dict(top_p=0.01)])
def test_reference_equals_the_warpers_in_sequence(sigma, opts):
    rs = np.random.default_rng(int(sigma * 10) + 7)
    checked = 0
    for V in (33, 257, 4099):
        x = (sigma * rs.standard_normal((6, V))).astype(np.float32)
        x[:, ::7] = -np.inf
        for r, ref in enumerate(TQ.truncate_rows(x, **opts)):
            o = dict(top_k=0, top_p=1.0, min_p=0.0)
            o.update(opts)
            keep, margin = _warpers(ref["key"], **o)
            assert ref["tau_p_lo"] <= ref["tau_p"] <= ref["tau_p_hi"]
            if min(margin, ref["margin"]) <= 1e-3:
                continue
            checked += 1
            assert np.array_equal(ref["keep"], keep), (V, r, opts, int(ref["keep"].sum()), int(keep.sum()))
            assert ref["kept"] == keep.sum() and ref["keep"][np.argmax(ref["key"])]
            w = np.exp(ref["key"].astype(np.float64) - ref["key"].max())
            assert abs(ref["logmass"] - np.log(w[keep].sum() / w.sum())) < 1e-12
    assert checked >= 3  # (flat rows at a large vocabulary have no token of share 1e-3 at the boundary: the small ones count)


def test_everything_off_keeps_every_finite_key():
    rs = np.random.default_rng(3)
    x = rs.standard_normal((3, 100)).astype(np.float32)
    x[0, 5:50] = -np.inf
    x[1] = -np.inf
    x[2, 7] = -0.0
    for r, ref in enumerate(TQ.truncate_rows(x)):
        assert np.array_equal(ref["keep"], np.isfinite(x[r]))
        assert ref["kept"] == np.isfinite(x[r]).sum()
        if r == 1:
            assert ref["tau"] == np.inf and ref["logmass"] == -np.inf
        else:
            assert ref["tau"] == -np.inf and ref["logmass"] == 0.0
    assert np.array_equal(TQ.unpack_bits(TQ.pack_bits(np.isfinite(x)))[:, :100], np.isfinite(x))
    assert not TQ.unpack_bits(TQ.pack_bits(np.ones((2, 33), bool)))[:, 33:].any()


def test_reference_by_hand():
    # probabilities 0.5, 0.25, 0.125, 0.0625, 0.0625 (the last two tied)
    x = np.log(np.array([0.125, 0.5, 0.0625, 0.25, 0.0625])).astype(np.float32)
    assert TQ.truncate_row(x, top_k=2)["keep"].tolist() == [False, True, False, True, False]
    assert TQ.truncate_row(x, top_k=4)["keep"].tolist() == [True] * 5  # the tie at the fourth place is kept whole
    assert TQ.truncate_row(x, top_k=5)["tau_k"] == -np.inf and TQ.truncate_row(x, top_k=9)["kept"] == 5
    assert TQ.truncate_row(x, top_p=0.6)["keep"].tolist() == [False, True, False, True, False]
    assert TQ.truncate_row(x, top_p=0.4)["kept"] == 1 and abs(TQ.truncate_row(x, top_p=0.4)["margin"] - 0.1) < 1e-7
    assert TQ.truncate_row(x, top_p=0.9)["kept"] == 5  # 0.875 < 0.9: the tied pair is needed, and kept whole
    assert TQ.truncate_row(x, top_k=2, top_p=0.7)["kept"] == 2  # 0.5 / 0.75 < 0.7: the nucleus of the two survivors is both
    assert TQ.truncate_row(x, top_k=2, top_p=0.6)["kept"] == 1
    assert TQ.truncate_row(x, min_p=0.25)["keep"].tolist() == [True, True, False, True, False]  # 0.125 = 0.25 * 0.5: at the bound
    assert TQ.truncate_row(x, min_p=0.26)["kept"] == 2
    got = TQ.truncate_row(x, top_k=2)
    assert abs(got["logmass"] - np.log(0.75)) < 1e-7 and got["tau"] == x[3]


def test_truncate_args_layout_matches_the_header(tmp_path):
    from genlm_backend_amd import _lib

    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "glb.h"\nint main(void) { printf("%zu %zu %zu %zu %d\\n", '
                   'sizeof(glb_truncate_args), offsetof(glb_truncate_args, top_k), offsetof(glb_truncate_args, out_bits), '
                   'offsetof(glb_truncate_args, out_logmass), GLB_ABI_VERSION); return 0; }\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "size")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "size")]).split()]
    T = _lib.TruncateArgs
    assert out == [C.sizeof(T), T.top_k.offset, T.out_bits.offset, T.out_logmass.offset, 9]
    assert "glb_truncate_rows" in _lib.SYMBOLS and _lib.load().glb_truncate_rows


def test_samplers_take_the_truncation_keywords():
    """Checked before any device work: an empty batch returns at once, a bad value raises by name."""
    from genlm_backend_amd.llm import AsyncAmdLM

    lm = object.__new__(AsyncAmdLM)
    assert lm.batch_sample_sync([], 4, [0], top_p=0.9) == []
    assert lm.batch_sample_sync([], 4, [0], temperature=0.7, seed=1, top_k=5, top_p=0.8, min_p=0.05) == []
    for kw, word in ((dict(top_p=0.0), "top_p"), (dict(top_p=1.5), "top_p"), (dict(top_p=float("nan")), "top_p"), (dict(top_p=-0.1), "top_p"),
                     (dict(top_k=-1), "top_k"), (dict(top_k=2.5), "top_k"), (dict(min_p=-0.1), "min_p"), (dict(min_p=1.5), "min_p"),
                     (dict(min_p=float("nan")), "min_p")):
        with pytest.raises(ValueError, match=word) as e:
            lm.batch_sample_sync([[1, 2]], 4, [0], **kw)
        assert repr(list(kw.values())[0]) in str(e.value)
