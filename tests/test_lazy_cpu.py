"""`constraints.LazyConstraint` without a GPU: the restatement tests/lazy_ref.py (the yardstick of the GPU tests) against
tests/nfa_det_ref.py and tests/dfa_ref.py - the sets reached are the determinised automaton's, cut to the useful states; the
rows are its states' rows; a particle dies where the automaton's dies; the argument errors that must be raised before a device
is looked at; the new entries of the signature table and their block."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import genlm_backend_amd
from genlm_backend_amd import _lib, constraints
from genlm_backend_amd.constraints import ByteDFA, ByteNFA, ByteWFSA, LazyConstraint  # (no test here passes without the class)
from tests import dfa_ref as R
from tests import lazy_ref as L
from tests import nfa_det_ref as N
from tests.test_regex_cpu import PATTERNS as REGEX_PATTERNS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = list(REGEX_PATTERNS) + [rb"(a*)*"]  # (b"" is REGEX_PATTERNS[0]; (a*)*: a cycle of empty arcs)
assert b"" in PATTERNS


def _bytes(pattern):
    return pattern.encode("utf-8") if isinstance(pattern, str) else pattern


def _small_vocab(pattern):
    """(vocab, eos, skip): the pattern's own letters (digits and non-ASCII bytes first) and three more as single bytes, pairs
    and triples of them, an empty token, a skipped token whose bytes the pattern may well read, and the EOS."""
    rank = lambda b: (0 if bytes([b]).isalnum() or b >= 128 else 1 if b in b"-. " else 2, b)
    letters = list(dict.fromkeys(sorted(set(_bytes(pattern)), key=rank) + [97, 98, 48, 10]))[:6]
    vocab = [bytes([b]) for b in letters]
    vocab += [bytes([a, b]) for a in letters[:4] for b in letters[:4]] + [bytes([a, b, a]) for a in letters[:3] for b in letters[:3]]
    vocab += [b"", bytes(letters[:1]), b"<eos>"]
    return vocab, len(vocab) - 1, (len(vocab) - 2, len(vocab) - 1)


@pytest.mark.parametrize("pattern", PATTERNS, ids=[repr(p) for p in PATTERNS])
def test_restatement_against_the_determinised_automaton(pattern):
    nfa = ByteNFA.from_regex(pattern)
    det = N.determinize(nfa)
    vocab, eos, skip = _small_vocab(pattern)
    dref, lref = R.Ref(det["delta"], det["accepting"], 0, vocab, eos, skip), L.Ref(nfa, vocab, eos, skip)
    rng = np.random.default_rng(len(_bytes(pattern)))
    n, ld = 300, 6
    tokens = rng.integers(0, len(vocab) - 2, (n, ld)).astype(np.int32)  # (the skipped tokens and one id past V come below)
    tokens[rng.random((n, ld)) < 0.02] = len(vocab) - 2
    tokens[rng.random((n, ld)) < 0.01] = len(vocab)
    to = rng.integers(0, ld + 1, n).astype(np.int32)
    cut = np.minimum(to, rng.integers(0, ld + 1, n)).astype(np.int32)
    # two calls: [0, cut) from the start, then [cut, to) from the states of the first
    first = lref.advance(None, tokens, np.zeros(n, np.int32), cut)
    n_first = lref.n_states
    out = lref.advance(first, tokens, cut, to)
    assert not lref.overflow and (first < n_first).all() and (out[first < 0] == -1).all()
    sets, acc = lref.sets(), lref.accepting()
    assert len(set(map(bytes, sets))) == len(sets) and sets.dtype == np.uint64 and sets.shape == (lref.n_states, det["sets"].shape[1])
    assert not (sets & ~lref.useful).any() and np.array_equal(lref.states, det["states"])
    checked = set()
    for i in range(n):
        for got, upto in ((first[i], cut[i]), (out[i], to[i])):
            d = dref.advance(0, tokens[i, :upto])
            assert (got < 0) == (d < 0), (i, upto)  # dead exactly when the automaton's particle is
            if got < 0:
                continue
            assert np.array_equal(sets[got], det["sets"][d] & lref.useful) and acc[got] == det["accepting"][d], (i, upto)
            if got not in checked and len(checked) < 8:
                checked.add(int(got))
                assert np.array_equal(lref.mask(int(got)), dref.mask(d)), (i, upto)
    # numbering: ids appear in the order of the particles, first call then second
    for ids in (first, out):
        new = [s for s in dict.fromkeys(ids[ids >= 0].tolist())]
        fresh = [s for s in new if s >= (1 if ids is first else n_first)]
        assert fresh == sorted(fresh)
    assert len(checked) > 0 or not det["live"][0] or (to == 0).all()


def test_restatement_overflow_cuts_in_particle_order():
    nfa = ByteNFA.from_regex(rb"(a|b)*a(a|b){3}")
    vocab, eos, skip = _small_vocab(rb"ab")
    tokens = np.array([[0], [1], [0], [4], [5], [8], [9]], np.int32)  # a b a aa ab ba bb
    frm, to = np.zeros(7, np.int32), np.ones(7, np.int32)
    whole = L.Ref(nfa, vocab, eos, skip)
    want = whole.advance(None, tokens, frm, to)
    assert not whole.overflow and want.tolist() == [1, 0, 1, 2, 3, 1, 0] and whole.n_states == 4
    tight = L.Ref(nfa, vocab, eos, skip, max_states=3)
    got = tight.advance(None, tokens, frm, to)
    assert tight.overflow and got.tolist() == [1, 0, 1, 2, -1, 1, 0] and tight.n_states == 3
    assert np.array_equal(tight.sets(), whole.sets()[:3])
    exact = L.Ref(nfa, vocab, eos, skip, max_states=4)
    assert exact.advance(None, tokens, frm, to).tolist() == want.tolist() and not exact.overflow
    # degenerate ranges and states
    r = L.Ref(nfa, vocab, eos, skip)
    t2 = np.array([[0, 1]] * 6, np.int32)
    got = r.advance(np.array([0, 0, 0, -1, 1, 0], np.int32), t2, np.array([1, 2, 0, 0, 0, -1], np.int32), np.array([1, 1, 3, 1, 1, 1], np.int32))
    assert got.tolist() == [0, -1, -1, -1, -1, -1]  # stays | frm > to | to > ld | dead stays dead | a state not yet numbered | frm < 0


def test_useful_states_agree():
    from genlm_backend_amd.constraints.lazy import useful_states

    for pattern in PATTERNS[::3]:
        nfa = ByteNFA.from_regex(pattern)
        assert np.array_equal(useful_states(nfa), L.useful(nfa))
    dead_end = ByteNFA(4, 0, [0, 0, 1, 0], [0, 0, 3], [1, 3, 3], np.stack([np.arange(256) == 97, np.arange(256) == 98, np.zeros(256, np.bool_)]), [1], [2])
    assert useful_states(dead_end).tolist() == [True, True, True, False] == L.useful(dead_end).tolist()


def test_new_symbols_are_in_the_signature_table_under_their_own_prefix(tmp_path):
    from genlm_backend_amd.engine import HipEngine

    new = {name for name in _lib.SYMBOLS if name.startswith("glb_lazy_")}
    assert new == {"glb_lazy_init", "glb_lazy_advance", "glb_lazy_serve"} == set(HipEngine.LAZY_CALLS)
    assert not new & HipEngine.DFA_CALLS and not new & HipEngine.FSA_CALLS and not new & HipEngine.NFA_CALLS and _lib.ABI_VERSION == 9
    for name in new:
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and args[0]._type_ is _lib.LazyArgs
    for name in ("glb_dfa_advance", "glb_fsa_live", "glb_nfa_closure", "glb_lazy_nothing", ""):  # (refused before the engine is looked at)
        with pytest.raises(ValueError):
            HipEngine.lazy_call(None, name, None)
    assert genlm_backend_amd.LazyConstraint is constraints.LazyConstraint and genlm_backend_amd.__all__[-1] == "minimize"
    # the block's size and its constants as a C compiler has them
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "glb.h"\nint main(void) { printf("%zu %zu %d %d %d", sizeof(glb_lazy_args), '
                   'offsetof(glb_lazy_args, force_wave), GLB_LAZY_STATUS, GLB_LAZY_OVERFLOW, GLB_LAZY_BUG); return 0; }\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "size")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "size")]).split()]
    assert out == [C.sizeof(_lib.LazyArgs), _lib.LazyArgs.force_wave.offset, _lib.LAZY_STATUS, _lib.LAZY_OVERFLOW, _lib.LAZY_BUG]
    assert out[2:] == [8, 1, 2]


def test_c_abi_refuses_before_any_launch():
    lib = _lib.load()
    keep = [np.zeros(64, np.int64) for _ in range(24)]
    ptr = lambda i: keep[i].ctypes.data

    def block(dfa=None, **over):
        p = _lib.LazyArgs()
        p.struct_size = C.sizeof(_lib.LazyArgs)
        d = p.dfa
        d.struct_size, d.n_states, d.eos_id, d.vocab, d.n_bytes, d.n, d.ld = C.sizeof(_lib.DfaArgs), 8, 2, 40, 64, 4, 2
        for i, k in enumerate(("tok_bytes", "tok_ptr", "skip", "tokens", "from_", "to", "state_in", "state_out", "bank", "row_of_state", "work",
                               "counters", "out_rows")):
            setattr(d, k, ptr(i))
        d.bank_ld, d.capacity, d.max_work = 2, 4, 2
        for k, v in (dfa or {}).items():
            setattr(d, k, v)
        p.n_nfa_states, p.nfa_start, p.n_important, p.n_words, p.n_arcs, p.max_states = 4, 0, 3, 1, 2, 8
        for i, k in enumerate(("arc_off", "arc_dst", "arc_bytes", "accepting_mask", "eclose", "table", "cand", "counts", "sets", "accepting_out")):
            setattr(p, k, ptr(13 + i))
        p.status, p.table_slots, p.cand_rows = ptr(23), 16, 8
        for k, v in over.items():
            setattr(p, k, v)
        return p

    shared = [("struct_size", 0), ("struct_size", C.sizeof(_lib.LazyArgs) - 8), ("max_states", 0), ("max_states", (1 << 22) + 1), ("n_important", 4097, "4096"),
              ("n_important", -1), ("n_important", 5), ("n_words", 2), ("n_words", 0), ("n_nfa_states", 0), ("nfa_start", 4), ("nfa_start", -1),
              ("n_arcs", -1), ("arc_off", None), ("arc_dst", None, "arc_dst"), ("arc_bytes", None, "arc_bytes"), ("accepting_mask", None),
              ("eclose", None), ("table_slots", 8), ("table_slots", 17), ("table", None), ("table", ptr(18) + 4, "aligned"), ("sets", None),
              ("accepting_out", None), ("status", None), ("epoch", ptr(0), "in part"), ("row_state", ptr(0), "in part")]
    inner = [("struct_size", 0, "glb_dfa_args"), ("struct_size", C.sizeof(_lib.DfaArgs) + 8, "glb_dfa_args"), ("vocab", 0, "vocab")]
    own = [
        (lib.glb_lazy_init, ([], [("bank", None, "bank"), ("bank_ld", 1, "bank_ld"), ("capacity", 1, "capacity"), ("counters", None, "bank")])),
        (lib.glb_lazy_advance, ([("cand", None), ("counts", None), ("cand_rows", 0), ("cand_rows", 9)],
                               [("n", 0, "n "), ("tokens", None, "null"), ("state_out", None, "null"), ("ld", 0, "ld"), ("tok_ptr", None, "vocabulary")])),
        (lib.glb_lazy_serve, ([], [("n", 0, "n "), ("state_in", None, "null"), ("out_rows", None, "null"), ("max_work", 0, "max_work"),
                                  ("skip", None, "vocabulary"), ("work", None, "bank")])),
    ]
    for fn, (outer, of_dfa) in own:
        assert fn(None, None) == _lib.GLB_EINVAL
        for field, value, *named in shared + outer:
            over = {field: value}
            if (field, value) == ("n_important", 4097):
                over.update(n_nfa_states=5000, n_words=65)
            assert fn(C.byref(block(**over)), None) == _lib.GLB_EINVAL, (field, value)
            assert (named or [field])[0] in _lib.last_error(), (field, value, _lib.last_error())
        for field, value, named in inner + of_dfa:
            assert fn(C.byref(block(dfa={field: value})), None) == _lib.GLB_EINVAL, (field, value)
            assert named in _lib.last_error(), (field, value, _lib.last_error())
    assert all(not k.any() for k in keep)  # nothing was written


def test_argument_errors_need_no_device():
    Lazy = LazyConstraint
    nfa = ByteNFA.from_regex(rb"ab*")
    vocab = [b"a", b"b", b"<eos>"]
    for bad in (None, "ab*", (1, 2)):
        with pytest.raises(ValueError, match="ByteNFA"):
            Lazy(None, bad, vocab, 2)
    with pytest.raises(ValueError, match="unweighted"):
        Lazy(None, ByteWFSA.from_dfa(ByteDFA.from_regex(rb"ab*")), vocab, 2)
    for bad in (0, -1, True, 1.5, None, "8", (1 << 22) + 1):
        with pytest.raises(ValueError, match="max_states"):
            Lazy(None, nfa, vocab, 2, max_states=bad)
    with pytest.raises(ValueError, match="on_full"):
        Lazy(None, nfa, vocab, 2, on_full="drop")
    with pytest.raises(ValueError, match="empty vocabulary"):
        Lazy(None, nfa, [], 0)
    with pytest.raises(ValueError, match="mask_bank_bytes=8"):
        Lazy(None, nfa, vocab, 2, mask_bank_bytes=8)
    n = 4097  # one important state past the cap: a chain of 4097 arcs
    wide = ByteNFA(n + 1, 0, np.zeros(n + 1, np.bool_), np.arange(n), np.arange(1, n + 1), np.ones((n, 256), np.bool_))
    with pytest.raises(ValueError, match="4096"):
        Lazy(None, wide, vocab, 2)
    # a ByteDFA passes the operand check: with no device the next thing missing is the engine itself
    with pytest.raises(AttributeError):
        Lazy(None, ByteDFA.from_regex(rb"ab*"), vocab, 2)
