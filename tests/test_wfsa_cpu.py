"""Weighted byte automata without a GPU: `ByteWFSA` (validation, -inf arcs, `from_weighted_strings`, `path_logw`), the
restatement tests/wfsa_ref.py checked against a per-token loop and against tests/dfa_ref.py at zero weights, the C ABI's
new symbols and the size of the new argument block."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from genlm_backend_amd.constraints import ByteWFSA  # (without the feature every test of this file fails here)
from tests import dfa_ref as R
from tests import wfsa_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = -np.inf


def _chain():
    """0 -A-> 1 -B-> 2 (final)."""
    d = np.full((3, 256), -1, np.int32)
    d[0, 65], d[1, 66] = 1, 2
    arc = np.full((3, 256), NINF, np.float32)
    arc[0, 65], arc[1, 66] = -0.5, -1.25
    fin = np.array([NINF, NINF, -2.0], np.float32)
    return d, arc, fin


def test_byte_wfsa_validation():
    from genlm_backend_amd.constraints import ByteDFA

    d, arc, fin = _chain()
    w = ByteWFSA(d, arc, fin, 0)
    assert isinstance(w, ByteDFA) and w.n_states == 3 and w.arc_logw.dtype == np.float32 and w.final_logw.dtype == np.float32
    assert w.accepting.tolist() == [False, False, True] and w.live.all()
    assert w.accepts(b"AB") and not w.accepts(b"A")
    assert w.path_logw(b"AB") == np.float32(-3.75) and w.path_logw(b"AB").dtype == np.float32
    assert w.path_logw(b"A") == NINF and w.path_logw(b"ABA") == NINF and w.path_logw(b"") == NINF

    def broken(where, value):
        a, f = arc.copy(), fin.copy()
        (a if where != "final" else f)[(0, 65) if where == "arc" else ((2, 9) if where == "no-arc" else 2)] = value
        return d, a, f, 0

    for args in [broken("arc", np.nan), broken("arc", np.inf), broken("final", np.nan), broken("final", np.inf),
                 broken("no-arc", -1.0), broken("no-arc", 0.0),  # a finite weight where delta has no arc
                 (d, arc[:2], fin, 0), (d, arc, fin[:2], 0), (d, arc, fin, 3), (d.astype(np.float32), arc, fin, 0)]:
        with pytest.raises(ValueError):
            ByteWFSA(*args)
    ByteWFSA(*broken("no-arc", NINF))  # -inf where there is no arc is what a missing arc weighs


def test_minus_inf_arcs_are_removed_before_liveness():
    d, arc, fin = _chain()
    arc[1, 66] = NINF  # state 1's only way out
    w = ByteWFSA(d, arc, fin, 0)
    assert w.delta[1, 66] == -1 and d[1, 66] == 2  # (the caller's table is not written)
    assert w.live.tolist() == [False, False, True] and not w.accepts(b"AB") and w.path_logw(b"AB") == NINF
    fin2 = np.full(3, NINF, np.float32)
    assert not ByteWFSA(d, _chain()[1], fin2, 0).live.any() and not ByteWFSA(d, _chain()[1], fin2, 0).accepting.any()


def test_from_weighted_strings_and_from_dfa():
    from genlm_backend_amd.constraints import ByteDFA

    lex = {b"yes": -0.25, b"no": -1.5, b"yesno": -3.0, b"y": 0.0, b"\x00\xff": -7.125}
    w = ByteWFSA.from_weighted_strings(lex)
    assert w.n_states == ByteDFA.from_strings(list(lex)).n_states and w.live.all()
    assert not w.arc_logw[w.delta >= 0].any() and np.isneginf(w.arc_logw[w.delta < 0]).all()
    for s, lw in lex.items():
        assert w.accepts(s) and w.path_logw(s) == np.float32(lw)
    for s in (b"", b"ye", b"yesn", b"yesnoo", b"n", b"\x00", b"on"):
        assert not w.accepts(s) and w.path_logw(s) == NINF
    with pytest.raises(ValueError):
        ByteWFSA.from_weighted_strings({})
    with pytest.raises(ValueError):
        ByteWFSA.from_weighted_strings({b"a": np.nan})
    assert not ByteWFSA.from_weighted_strings({b"a": -1.0, b"ab": NINF}).accepts(b"ab")  # weight -inf: not a member
    for name, (d, acc, start) in R.automata().items():
        dfa = ByteDFA(d, acc, start)
        z = ByteWFSA.from_dfa(dfa)
        assert np.array_equal(z.delta, dfa.delta) and np.array_equal(z.accepting, dfa.accepting) and np.array_equal(z.live, dfa.live)
        assert not z.arc_logw[dfa.delta >= 0].any() and not z.final_logw[dfa.accepting].any(), name


def _weighted(name, seed=5):
    d, acc, start = R.automata()[name]
    arc, fin = W.random_weights(d, acc, seed)
    return d, acc, start, arc, fin


@pytest.mark.parametrize("name", ["digits", "everything", "trap", "random37"])
def test_restatement_equals_a_per_token_loop(name):
    """A self-check of the yardstick: tests/wfsa_ref.py sums the weights in two independent ways (`weight`, one token byte by
    byte; `weights_all`, every token side by side) and the GPU tests compare against the second."""
    vocab, eos, skip = R.synth_vocab(300, 1)
    assert len(vocab) == 300 and b"" in vocab and max(map(len, vocab)) == 70
    d, acc, start, arc, fin = _weighted(name)
    ref = W.WRef(d, arc, fin, start, vocab, eos, skip)
    wf = ByteWFSA(d, arc, fin, start)
    assert np.array_equal(ref.live, wf.live) and np.array_equal(ref.accepting, wf.accepting)
    finite = 0
    for s in range(min(len(acc), 6)):
        row = ref.row(s)
        assert row.dtype == np.float32 and row.shape == (300,)
        for t in range(300):
            want = ref.final[s] if t == eos else ref.weight(s, t)
            assert row[t].tobytes() == np.float32(want).tobytes(), (name, s, t)
            if t != eos and ref.next(s, t) >= 0:  # the product's own host walk, from state s
                assert np.isfinite(row[t])
                finite += 1
        assert row[256] == NINF and row[257] == NINF  # the empty token, the special
    assert finite > 0
    assert np.isneginf(ref.row(-1)).all() and np.isneginf(ref.wrow_dead()).all()
    e = ref.wrow_eos()
    assert e[eos] == 0.0 and np.isneginf(np.delete(e, eos)).all()
    # a 70-byte token sums 70 weights in byte order: the float32 chain, not a float64 sum rounded once
    if name == "digits":
        t = vocab.index(b"0" * 70)
        chain = np.float32(0.0)
        for _ in range(1):
            chain = np.float32(chain + arc[0, 48])
        for _ in range(69):
            chain = np.float32(chain + arc[1, 48])
        assert ref.row(0)[t].tobytes() == chain.tobytes()
        assert wf.path_logw(b"0" * 70) == np.float32(chain + fin[1]) == ref.path_logw(b"0" * 70)


@pytest.mark.parametrize("name", ["digits", "everything", "trap", "random37"])
def test_zero_weights_give_the_boolean_mask(name):
    vocab, eos, skip = R.synth_vocab(300, 1)
    d, acc, start = R.automata()[name]
    arc, fin = W.zero_weights(d, acc)
    ref, bref = W.WRef(d, arc, fin, start, vocab, eos, skip), R.Ref(d, acc, start, vocab, eos, skip)
    for s in range(len(acc)):
        assert ref.row(s).tobytes() == W.bits_to_weights(bref.mask(s), 300).tobytes(), (name, s)
    assert ref.wrow_eos().tobytes() == W.bits_to_weights(bref.row_eos(), 300).tobytes()
    assert ref.wrow_dead().tobytes() == W.bits_to_weights(bref.row_dead(), 300).tobytes()


def test_abi_symbols_and_bank_rows():
    import genlm_backend_amd
    from genlm_backend_amd import _lib

    lib = _lib.load()
    for name in ("glb_dfa_weight_bank_init", "glb_dfa_fill_weights", "glb_dfa_weight_bank_rows"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert "ByteWFSA" in genlm_backend_amd.__all__ and genlm_backend_amd.ByteWFSA is ByteWFSA
    row = 50304 * 4  # 50257 floats padded to a multiple of 64: about 201 KB
    assert lib.glb_dfa_weight_bank_rows(256 << 20, 50257, 100) == 102
    assert lib.glb_dfa_weight_bank_rows(256 << 20, 50257, 5000) == (256 << 20) // row == 1334
    assert lib.glb_dfa_weight_bank_rows(10 * row + 3, 50257, 100) == 10 and lib.glb_dfa_weight_bank_rows(3 * row - 1, 50257, 100) == 2
    assert lib.glb_dfa_weight_bank_rows(1 << 44, 300, 1 << 20) == 65535
    assert lib.glb_dfa_weight_bank_rows(1 << 20, 0, 4) == 0 and lib.glb_dfa_weight_bank_rows(1 << 20, 64, 0) == 0
    assert lib.glb_dfa_weight_bank_init(None, None) == _lib.GLB_EINVAL and lib.glb_dfa_fill_weights(None, None) == _lib.GLB_EINVAL
    assert lib.glb_abi_version() == 9 == _lib.ABI_VERSION


def test_argument_blocks_have_the_headers_sizes(tmp_path):
    from genlm_backend_amd import _lib

    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler"
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "glb.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                   'sizeof(glb_dfa_weight_args), offsetof(glb_dfa_weight_args, dfa), offsetof(glb_dfa_weight_args, arc_logw), '
                   'offsetof(glb_dfa_weight_args, wbank_ld), sizeof(glb_dfa_args)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = tuple(int(v) for v in subprocess.check_output([str(exe)]).split())
    A = _lib.DfaWeightArgs
    assert got == (C.sizeof(A), A.dfa.offset, A.arc_logw.offset, A.wbank_ld.offset, C.sizeof(_lib.DfaArgs)) == (248, 8, 216, 240, 208)
