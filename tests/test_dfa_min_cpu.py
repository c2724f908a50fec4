"""Minimisation without a GPU: the argument block against the header, every GLB_EINVAL case (the checks run before any
launch), `minimize=` validation, `ByteDFA.reachable` against a plain search, and the sanity of the restatement
tests/dfa_min_ref.py that the GPU tests compare against."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from genlm_backend_amd import _lib
from genlm_backend_amd.constraints import ByteDFA, ByteWFSA, DeviceConstraint, minimize
from tests import dfa_min_ref as M
from tests import dfa_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTERS = ("delta", "keep", "final_bits", "arc_bits", "cls", "scratch", "table", "status", "new_id", "rep", "arc_logw", "final_logw",
            "accepting", "delta_out", "arc_out", "final_out", "accepting_out")


def test_argument_block_has_the_headers_size_and_offsets(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler"
    fields = [name for name, _ in _lib.DfaMinArgs._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "glb.h"\nint main(void) { printf("%zu %d", '
                   'sizeof(glb_dfa_min_args), GLB_DFA_MIN_STATUS);\n'
                   + "".join(f'printf(" %zu", offsetof(glb_dfa_min_args, {f}));\n' for f in fields) + "return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    A = _lib.DfaMinArgs
    assert got[:2] == [C.sizeof(A), _lib.DFA_MIN_STATUS] == [168, 8]
    assert got[2:] == [getattr(A, f).offset for f in fields] == [0, 4, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 84, 88, 96, 104, 112, 120,
                                                               128, 136, 144, 152, 160]


def _block(**kw):
    """A block that passes every check of both calls; its pointers are never followed: the calls below fail before any launch."""
    p = _lib.DfaMinArgs()
    p.struct_size = C.sizeof(_lib.DfaMinArgs)
    p.n_states, p.table_slots, p.rounds, p.restart, p.n_new = 4, 8, 1, 1, 2
    for f in POINTERS:
        setattr(p, f, 0x1000)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_argument_errors_without_a_device():
    lib = _lib.load()
    for name in ("glb_dfa_refine", "glb_dfa_quotient"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.glb_abi_version() == 9 == _lib.ABI_VERSION
    both = [("struct_size", 0), ("struct_size", 160), ("struct_size", 176), ("n_states", 0), ("n_states", -3), ("delta", None),
            ("keep", None)]
    own = {"glb_dfa_refine": [("rounds", 0), ("rounds", -5), ("rounds", 65537), ("table_slots", 7), ("table_slots", 4), ("table_slots", 12),
                              ("table_slots", 0), ("table_slots", -8), ("final_bits", None), ("cls", None), ("scratch", None),
                              ("table", None), ("table", 0x1004), ("status", None)],
           "glb_dfa_quotient": [("n_new", 0), ("n_new", 5), ("n_new", -1), ("new_id", None), ("rep", None), ("delta_out", None),
                                ("arc_logw", None), ("final_logw", None), ("accepting", None)]}
    for name, cases in own.items():
        fn = getattr(lib, name)
        assert fn(None, None) == _lib.GLB_EINVAL
        for field, value in both + cases:
            assert fn(C.byref(_block(**{field: value})), None) == _lib.GLB_EINVAL, (name, field, value)
            assert field in _lib.last_error(), (name, field, _lib.last_error())


def test_minimize_validation():
    d, acc, start = R.automata()["digits"]
    vocab = [bytes([b]) for b in range(256)]
    # (the arguments are refused before the engine is looked at: no device is needed to be told so)
    for bad in ("yes", 1, None, 0):
        with pytest.raises(ValueError, match="minimize must be"):
            DeviceConstraint(None, ByteDFA(d, acc, start), vocab, 0, minimize=bad)
    with pytest.raises(ValueError, match="ByteDFA"):
        minimize(None, (d, acc, start))
    for bad in (0, -1, True, 1.5):
        with pytest.raises(ValueError, match="max_rounds"):
            minimize(None, ByteDFA(d, acc, start), max_rounds=bad)
    import genlm_backend_amd

    assert genlm_backend_amd.__all__[-1] == "minimize" and genlm_backend_amd.minimize is minimize


@pytest.mark.parametrize("name", ["digits", "everything", "trap", "random37"])
def test_reachable_against_a_plain_search(name):
    d, acc, start = R.automata()[name]
    for s in range(len(acc)):
        got = ByteDFA(d, acc, s).reachable
        assert got.dtype == np.bool_ and np.array_equal(got, M.reachable(d, s)), (name, s)
    dd, dacc, dstart = M.doubled(d, acc, start)
    r = ByteDFA(dd, dacc, dstart).reachable
    assert np.array_equal(r, M.reachable(dd, dstart)) and not r[2 * len(acc):].any()


def test_the_restatement_minimises_what_it_should():
    A = R.automata()
    sizes = {}
    for name, (d, acc, start) in A.items():
        q, qacc, qstart, state_map, rounds = M.minimize(d, acc, start)
        sizes[name] = (len(acc), len(qacc), int((state_map >= 0).sum()))
        assert M.isomorphic((q, qacc, qstart), M.minimize(q, qacc, qstart)[:3])  # minimal: a second pass merges nothing
        assert M.minimize(q, qacc, qstart)[0].shape == q.shape
    assert sizes == {"digits": (2, 2, 2), "everything": (1, 1, 1), "trap": (4, 2, 2), "random37": (37, 37, 37)}
    # the doubled automaton folds back onto the single one
    d, acc, start = A["random37"]
    dd, dacc, dstart = M.doubled(d, acc, start)
    q, qacc, qstart, state_map, _ = M.minimize(dd, dacc, dstart)
    assert len(dacc) == 84 and len(qacc) == 37 and (state_map[74:] == -1).all() and (state_map[:74] >= 0).all()
    assert M.isomorphic((q, qacc, qstart), (d, acc, start)) and np.array_equal(state_map[:37], state_map[37:74])
    assert not M.isomorphic((q, qacc, qstart), (d, ~acc, start))


def test_the_trie_and_the_chain():
    t = ByteDFA.from_strings(M.lexicon_trie())
    q, qacc, qstart, state_map, rounds = M.minimize(t.delta, t.accepting, t.start)
    assert (t.n_states, len(qacc), rounds) == (1440, 406, 5) and qstart == 0
    small = ByteDFA(q, qacc, qstart)
    rng = np.random.default_rng(2)
    for s in M.lexicon_trie()[:200] + [bytes(rng.choice(np.frombuffer(b"abcd", np.uint8), int(rng.integers(0, 9)))) for _ in range(300)]:
        assert small.accepts(s) == t.accepts(s)
    c = ByteDFA.from_regex(rb"a{200}")
    q, qacc, qstart, state_map, rounds = M.minimize(c.delta, c.accepting, c.start)
    assert (c.n_states, len(qacc), rounds) == (201, 201, 200) and np.array_equal(state_map, np.arange(201))


def test_weights_are_labels_bit_for_bit():
    """Two strings with one suffix merge only where the suffix's weights have equal bits; -0.0 and 0.0 are different labels."""
    wf = ByteWFSA.from_weighted_strings({b"ax": -1.0, b"bx": -1.0, b"cx": -1.0000001})
    keep = M.keep_of(wf.delta, wf.accepting, wf.start)
    cls, _ = M.refine(wf.delta, keep, wf.final_logw.view(np.uint32), wf.arc_logw.view(np.uint32))
    new_id, rep = M.new_ids(cls)
    assert len(rep) == 5 and new_id[wf.delta[0, ord("a")]] == new_id[wf.delta[0, ord("b")]] != new_id[wf.delta[0, ord("c")]]
    cls0, _ = M.refine(wf.delta, keep, wf.accepting.astype(np.int64))  # unweighted: one suffix
    assert len(M.new_ids(cls0)[1]) == 3
    arc = wf.arc_logw.copy()
    arc[wf.delta[0, ord("b")], ord("x")] = np.float32(-0.0)
    cls1, _ = M.refine(wf.delta, keep, wf.final_logw.view(np.uint32), arc.view(np.uint32))
    assert len(M.new_ids(cls1)[1]) == 6  # the final states of ax and bx still merge, the states before them no longer do
