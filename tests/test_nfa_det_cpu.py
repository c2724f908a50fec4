"""`ByteNFA` and `constraints.determinize` without a GPU: the restatement tests/nfa_det_ref.py (the yardstick of the GPU tests)
against `ByteNFA.accepts`, `re.fullmatch` and `ByteDFA.from_regex`; the constructors against brute force; the argument errors
that must be raised before a device is looked at; the new entries of the signature table and their block."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import genlm_backend_amd
from genlm_backend_amd import _lib, constraints
from genlm_backend_amd.constraints import ByteDFA, ByteNFA, ByteWFSA
from tests import dfa_min_ref as M
from tests import dfa_ref as R
from tests import nfa_det_ref as N
from tests.test_regex_cpu import PATTERNS as REGEX_PATTERNS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = list(REGEX_PATTERNS) + [rb"(a*)*", rb"(a|b)*a(a|b){3}"]  # (b"" is REGEX_PATTERNS[0]; (a*)*: a cycle of empty arcs)
assert b"" in PATTERNS


def _bytes(pattern):
    return pattern.encode("utf-8") if isinstance(pattern, str) else pattern


def _letters(pattern):
    """Four bytes to draw strings from: the pattern's own letters, digits and non-ASCII bytes first."""
    rank = lambda b: (0 if bytes([b]).isalnum() or b >= 128 else 1 if b in b"-. " else 2, b)
    return bytes((sorted(set(_bytes(pattern)), key=rank) + [97, 98, 48, 10])[:4])


def _all_strings(letters, upto):
    for n in range(upto + 1):
        for t in itertools.product(sorted(set(letters)), repeat=n):
            yield bytes(t)


def _samples(p, n, seed):
    """Up to n strings the restated automaton accepts: seeded walks over arcs into live states."""
    rng, out = np.random.default_rng(seed), []
    for _ in range(3 * n):
        s, text = 0, bytearray()
        while p["live"][s] and len(text) < 12:
            if p["accepting"][s] and rng.random() < 0.3:
                break
            arcs = [b for b in range(256) if p["delta"][s, b] >= 0 and p["live"][p["delta"][s, b]]]
            if not arcs:
                break
            text.append(int(rng.choice(arcs)))
            s = int(p["delta"][s, text[-1]])
        if N.accepts(p, bytes(text)):
            out.append(bytes(text))
    return out[:n]


@pytest.mark.parametrize("pattern", PATTERNS, ids=[repr(p) for p in PATTERNS])
def test_restatement_against_the_nfa_fullmatch_and_from_regex(pattern):
    nfa = ByteNFA.from_regex(pattern)
    p = N.determinize(nfa)
    rx = re.compile(_bytes(pattern))
    strings = list(_all_strings(_letters(pattern), 5)) + _samples(p, 40, len(_bytes(pattern)))
    rng = np.random.default_rng(7)
    strings += [bytes(rng.integers(0, 256, int(rng.integers(0, 8))).astype(np.uint8)) for _ in range(40)]
    for s in strings:
        want = rx.fullmatch(s) is not None
        assert N.accepts(p, s) == want, s
    for s in strings[::3]:
        assert nfa.accepts(s) == (rx.fullmatch(s) is not None), s
    # the same automaton as the host compiler's, whose states come in byte-group order: equal counts as they are, equal arrays
    # after a queue search in byte order
    host = ByteDFA.from_regex(pattern)
    assert host.n_states == len(p["accepting"])
    d, acc, old = N.renumber(host.delta, host.accepting, host.start)
    assert np.array_equal(d, p["delta"]) and np.array_equal(acc, p["accepting"]) and sorted(old.tolist()) == list(range(host.n_states))
    assert np.array_equal(p["live"], ByteDFA(p["delta"], p["accepting"], 0).live) and p["delta"].dtype == np.int32
    # the sets: W words, bits of important states alone, state 0 the closure of the start, accepting where the set says so
    n_imp = len(p["states"])
    assert p["sets"].dtype == np.uint64 and p["sets"].shape == (len(d), max(1, -(-n_imp // 64)))
    members = np.unpackbits(p["sets"].view(np.uint8), axis=1, bitorder="little").astype(np.bool_)
    assert not members[:, n_imp:].any() and len(set(map(bytes, p["sets"]))) == len(d)
    assert np.array_equal((members[:, :n_imp] & nfa.accepting[p["states"]]).any(axis=1), p["accepting"])
    assert N.important(nfa)[p["states"]].all() and N.important(nfa).sum() == n_imp


def test_an_empty_language_behind_concat():
    """`concat` with an automaton that accepts nothing: no string is left, and the restatement's start is not live."""
    nothing = ByteDFA(np.zeros((1, 256), np.int32), np.zeros(1, np.bool_), 0)
    for items in ([ByteDFA.from_regex(rb"ab*"), nothing], [nothing, ByteDFA.from_regex(rb"ab*")], [ByteNFA.from_regex(rb"a"), nothing, rb"b"]):
        nfa = ByteNFA.concat([ByteDFA.from_regex(x) if isinstance(x, bytes) else x for x in items])
        p = N.determinize(nfa)
        assert not p["live"].any() and not p["accepting"].any()
        assert not any(nfa.accepts(s) or N.accepts(p, s) for s in _all_strings(b"ab", 5))


def test_union_of_five_accepts_what_any_accepts():
    parts = [ByteDFA.from_regex(rb"a*b+c?"), ByteNFA.from_regex(rb"(ab)*(?:cd)+e?"), ByteDFA(*R.automata()["digits"]), ByteDFA.from_regex(rb"[a-cx-z]*"),
             ByteNFA.from_regex(rb"a{2,4}").star()]
    nfa = ByteNFA.union(parts)
    assert nfa.n_states == 1 + sum(x.n_states for x in parts) and nfa.start == 0
    p = N.determinize(nfa)
    as_nfa = [x if isinstance(x, ByteNFA) else ByteNFA.from_dfa(x) for x in parts]
    strings = list(_all_strings(b"abc0", 5)) + [s for i, x in enumerate(as_nfa) for s in _samples(N.determinize(x), 20, i)]
    some = 0
    for s in strings:
        want = any(x.accepts(s) for x in parts)
        assert N.accepts(p, s) == want, s
        some += want
    assert 0 < some < len(strings)
    for s in strings[::5]:
        assert nfa.accepts(s) == any(x.accepts(s) for x in parts), s
    assert ByteNFA.union([parts[0]]).accepts(b"bb") and not ByteNFA.union([parts[0]]).accepts(b"c")


def test_concat_star_plus_optional_against_splitting():
    a, b = ByteDFA.from_regex(rb"ab|a"), ByteNFA.from_regex(rb"b*c|")
    strings = list(_all_strings(b"abc", 6))
    in_a, in_b = {s for s in strings if a.accepts(s)}, {s for s in strings if b.accepts(s)}
    both, star, plus, opt = ByteNFA.concat([a, b]), ByteNFA.from_dfa(a).star(), ByteNFA.from_dfa(a).plus(), ByteNFA.from_dfa(a).optional()
    three = ByteNFA.concat([a, b, a])

    def splits(s, parts):  # s is one string of every language in turn
        if not parts:
            return s == b""
        return any(s[:i] in parts[0] and splits(s[i:], parts[1:]) for i in range(len(s) + 1))

    def repeats(s):  # s is one or more strings of a in a row
        return any(s[:i] in in_a and (i == len(s) or repeats(s[i:])) for i in range(1, len(s) + 1))

    det = {name: N.determinize(x) for name, x in (("both", both), ("star", star), ("plus", plus), ("opt", opt), ("three", three))}
    for s in strings:
        want = dict(both=splits(s, [in_a, in_b]), three=splits(s, [in_a, in_b, in_a]), star=s == b"" or repeats(s), plus=repeats(s),
                    opt=s == b"" or s in in_a)
        for name, w in want.items():
            assert N.accepts(det[name], s) == w, (name, s)
    for s in strings[::7]:
        assert both.accepts(s) == splits(s, [in_a, in_b]) and star.accepts(s) == (s == b"" or repeats(s))
    # word( word)*: a trie, then a separator and the trie again, any number of times
    words = [b"ab", b"b", b"cab"]
    trie = ByteDFA.from_strings(words)
    phrase = ByteNFA.concat([trie, ByteNFA.concat([ByteDFA.from_regex(rb" "), trie]).star()])
    p = N.determinize(phrase)
    for s in _all_strings(b"ab c", 6):
        assert N.accepts(p, s) == (s != b"" and all(w in words for w in s.split(b" "))), s


def test_from_dfa_gives_the_reachable_part_renumbered():
    for name in ("digits", "random37", "trap"):
        dfa = ByteDFA(*R.automata()[name])
        nfa = ByteNFA.from_dfa(dfa)
        assert nfa.n_states == dfa.n_states and nfa.start == dfa.start and len(nfa.eps_src) == 0
        assert np.array_equal(nfa.arc_set.any(axis=1), np.ones(len(nfa.arc_src), np.bool_))
        p = N.determinize(nfa)
        d, acc, old = N.renumber(dfa.delta, dfa.accepting, dfa.start)
        # a state without arcs that does not accept is no important state: the arcs into it lead to the empty set
        gone = ~N.important(nfa)[old]
        keep = np.nonzero(~gone)[0]
        assert not gone[0]
        to = np.full(len(old), -1, np.int32)
        to[keep] = np.arange(len(keep), dtype=np.int32)
        want = np.where(d[keep] >= 0, to[np.maximum(d[keep], 0)], -1)
        assert np.array_equal(p["delta"], want) and np.array_equal(p["accepting"], acc[keep])
        assert (np.unpackbits(p["sets"].view(np.uint8), axis=1, bitorder="little").sum(axis=1) == 1).all()  # every set is one state
    trie = ByteDFA.from_strings(M.lexicon_trie())
    p = N.determinize(ByteNFA.from_dfa(trie))
    d, acc, _ = N.renumber(trie.delta, trie.accepting, trie.start)
    assert np.array_equal(p["delta"], d) and np.array_equal(p["accepting"], acc) and len(acc) == trie.n_states
    with pytest.raises(ValueError, match="unweighted"):
        ByteNFA.from_dfa(ByteWFSA.from_dfa(trie))
    with pytest.raises(ValueError, match="unweighted"):
        ByteNFA.union([trie, ByteWFSA.from_dfa(trie)])
    with pytest.raises(ValueError, match="ByteDFA"):
        ByteNFA.from_dfa(None)


def test_restatement_numbering_and_overflow():
    """bc or ad, written in that order: the states come out breadth first, bytes ascending - a's target before b's; one state
    fewer than the count is the overflow."""
    p = N.determinize(ByteNFA.from_regex(rb"(bc|ad)e?"))
    order = [int(t) for row in p["delta"] for t in row if t >= 0]
    seen = []
    for t in order:
        if t not in seen:
            seen.append(t)
    assert seen == list(range(1, len(p["accepting"]))) and p["delta"][0, 97] == 1 and p["delta"][0, 98] == 2
    n = len(N.determinize(ByteNFA.from_regex(rb"(a|b)*a(a|b){3}"))["accepting"])
    assert n == 16
    with pytest.raises(ValueError, match="max_states"):
        N.determinize(ByteNFA.from_regex(rb"(a|b)*a(a|b){3}"), n - 1)
    assert len(N.determinize(ByteNFA.from_regex(rb"(a|b)*a(a|b){3}"), n)["accepting"]) == n


def test_constructor_validates():
    ok = dict(n_states=3, start=0, accepting=[0, 0, 1], arc_src=[0, 1], arc_dst=[1, 2], arc_set=np.zeros((2, 256), np.bool_), eps_src=[0], eps_dst=[2])
    x = ByteNFA(**ok)
    assert x.arc_src.dtype == np.int32 and x.accepting.dtype == np.bool_ and x.accepts(b"") and x.important.tolist() == [True, True, True]
    for field, bad in (("n_states", 0), ("n_states", 2.0), ("start", 3), ("start", True), ("accepting", [0, 1]), ("accepting", [0, 2, 1]),
                       ("arc_src", [0, 3]), ("arc_dst", [-1, 2]), ("arc_src", [0.0, 1.0]), ("arc_set", np.zeros((2, 255), np.bool_)),
                       ("arc_set", np.full((2, 256), 2)), ("arc_dst", [1]), ("eps_src", [0, 1]), ("eps_dst", [3])):
        with pytest.raises(ValueError, match=field.split("_")[0]):
            ByteNFA(**dict(ok, **{field: bad}))
    for refused, named in ((rb"^a", "anchor"), (rb"(a)\1", "backreference"), (rb"a*?", "lazy")):
        with pytest.raises(ValueError, match=named):
            ByteNFA.from_regex(refused)
    with pytest.raises(ValueError, match="at least one"):
        ByteNFA.union([])
    with pytest.raises(ValueError, match="ByteNFA or ByteDFA"):
        ByteNFA.concat([x, "abc"])


def test_argument_errors_need_no_device():
    nfa = ByteNFA.from_regex(rb"ab*")
    determinize = constraints.determinize
    assert genlm_backend_amd.determinize is determinize and genlm_backend_amd.ByteNFA is ByteNFA and genlm_backend_amd.__all__[-1] == "minimize"
    for bad in (ByteDFA.from_regex(rb"ab*"), None, "ab*", (1, 2)):
        with pytest.raises(ValueError, match="ByteNFA"):
            determinize(None, bad)
    with pytest.raises(ValueError, match="unweighted"):
        determinize(None, ByteWFSA.from_dfa(ByteDFA.from_regex(rb"ab*")))
    for bad in (0, -1, True, 1.5, None, "8"):
        with pytest.raises(ValueError, match="max_states"):
            determinize(None, nfa, max_states=bad)
        with pytest.raises(ValueError, match="max_states"):
            ByteDFA.from_regex(rb"ab*", max_states=bad, device=object())
    n = 4097  # one important state past the cap: a chain of 4097 arcs
    wide = ByteNFA(n + 1, 0, np.zeros(n + 1, np.bool_), np.arange(n), np.arange(1, n + 1), np.ones((n, 256), np.bool_))
    with pytest.raises(ValueError, match="4096"):
        determinize(None, wide)
    # without a device the default path is today's, bit for bit
    today = ByteDFA.from_regex(rb"-?(0|[1-9][0-9]*)(\.[0-9]+)?")
    d, acc = constraints._regex_dfa(rb"-?(0|[1-9][0-9]*)(\.[0-9]+)?", 65536)
    assert np.array_equal(today.delta, d) and np.array_equal(today.accepting, acc)


def test_what_the_device_reads():
    """`_nfa_arrays`: the CSRs, the byte sets as four words, the groups in the order of their lowest bytes."""
    from genlm_backend_amd.constraints.tables import _nfa_arrays

    nfa = ByteNFA(5, 1, [0, 0, 0, 1, 0], [2, 0, 2], [3, 2, 0], np.stack([np.arange(256) >= 200, np.arange(256) % 2 == 0, np.arange(256) == 7]), [1, 1, 4], [0, 2, 4])
    a = _nfa_arrays(nfa)
    assert a["states"].tolist() == [0, 2, 3] and a["bit_of"].tolist() == [0, -1, 1, 2, -1] and (a["n_important"], a["n_words"]) == (3, 1)
    assert a["eps_off"].tolist() == [0, 0, 2, 2, 2, 3] and a["eps_to"].tolist() == [0, 2, 4]
    assert a["arc_off"].tolist() == [0, 1, 3, 3] and a["arc_dst"].tolist() == [2, 3, 0]
    sets = np.unpackbits(a["arc_bytes"].view(np.uint8), axis=1, bitorder="little").astype(np.bool_)
    assert np.array_equal(sets, nfa.arc_set[[1, 0, 2]]) and a["arc_bytes"].dtype == np.uint64 and a["accepting_mask"].tolist() == [4]
    # groups: even below 200 | odd but 7 below 200 | 7 | even from 200 | odd from 200, named by their lowest bytes 0 1 7 200 201
    assert a["group_lo"].tolist() == [0, 1, 7, 200, 201] and a["group_of"][[0, 1, 2, 7, 9, 200, 201, 255]].tolist() == [0, 1, 0, 2, 1, 3, 4, 4]
    empty = _nfa_arrays(ByteNFA(1, 0, [0], [], [], []))
    assert (empty["n_important"], empty["n_words"], empty["n_arcs"], empty["n_groups"]) == (0, 1, 0, 1) and empty["arc_off"].tolist() == [0]
    assert all(len(empty[k]) >= 1 for k in ("eps_to", "arc_dst", "arc_bytes", "accepting_mask", "group_lo"))
    for n_imp, words in ((63, 1), (64, 1), (65, 2), (4096, 64)):
        chain = ByteNFA(n_imp, 0, np.arange(n_imp) == n_imp - 1, np.arange(n_imp - 1), np.arange(1, n_imp), np.ones((n_imp - 1, 256), np.bool_))
        assert (_nfa_arrays(chain)["n_important"], _nfa_arrays(chain)["n_words"]) == (n_imp, words)


def test_new_symbols_are_in_the_signature_table_under_their_own_prefix(tmp_path):
    from genlm_backend_amd.engine import HipEngine

    new = {name for name in _lib.SYMBOLS if name.startswith("glb_nfa_")}
    assert new == {"glb_nfa_closure", "glb_nfa_subset_round"} == set(HipEngine.NFA_CALLS)
    assert not new & HipEngine.DFA_CALLS and not new & HipEngine.FSA_CALLS and _lib.ABI_VERSION == 9
    for name in new:
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and args[0]._type_ is _lib.NfaArgs
    for name in ("glb_dfa_refine", "glb_fsa_live", "glb_nfa_nothing", ""):  # (refused before the engine is looked at)
        with pytest.raises(ValueError):
            HipEngine.nfa_call(None, name, None)
    # the block's size as a C compiler has it
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "glb.h"\nint main(void) { printf("%zu %d %d", sizeof(glb_nfa_args), GLB_NFA_STATUS, GLB_NFA_MAX_IMPORTANT); return 0; }\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "size")])
    out = subprocess.check_output([str(tmp_path / "size")]).split()
    assert [int(x) for x in out] == [C.sizeof(_lib.NfaArgs), _lib.NFA_STATUS, _lib.NFA_MAX_IMPORTANT] == [200, 16, 4096]


def test_c_abi_refuses_before_any_launch():
    lib = _lib.load()
    keep = [np.zeros(64, np.int64) for _ in range(16)]
    ptr = lambda i: keep[i].ctypes.data

    def block(**over):
        p = _lib.NfaArgs()
        p.struct_size, p.n_states, p.start, p.n_important, p.n_words, p.n_arcs, p.n_eps, p.n_groups = C.sizeof(_lib.NfaArgs), 4, 0, 3, 1, 2, 1, 2
        for i, k in enumerate(("eps_off", "eps_to", "bit_of", "arc_off", "arc_dst", "arc_bytes", "accepting_mask", "group_of", "group_lo", "eclose", "table",
                               "cand", "sets", "delta_out", "accepting_out", "counts")):
            setattr(p, k, ptr(i))
        p.status = ptr(0)
        p.max_states, p.chunk, p.table_slots, p.rounds, p.restart = 8, 8, 16, 1, 1
        for k, v in over.items():
            setattr(p, k, v)
        return p

    shared = [("struct_size", 0), ("struct_size", C.sizeof(_lib.NfaArgs) - 8), ("n_states", 0), ("n_states", -3), ("n_important", 4097, "4096"),
              ("n_important", -1), ("n_important", 5), ("n_words", 2), ("n_words", 0), ("start", 4), ("start", -1), ("rounds", 0), ("rounds", 65537),
              ("eclose", None), ("status", None)]
    closure = [("n_eps", -1), ("eps_off", None, "eps_off"), ("eps_to", None, "eps_to"), ("bit_of", None)]
    search = [("n_arcs", -1), ("n_groups", 0), ("n_groups", 257), ("max_states", 0), ("max_states", (1 << 22) + 1), ("chunk", 0), ("chunk", 9),
              ("arc_off", None), ("arc_dst", None, "arc_dst"), ("arc_bytes", None, "arc_bytes"), ("accepting_mask", None), ("group_of", None),
              ("group_lo", None, "group_lo"), ("table_slots", 8), ("table_slots", 17), ("table", None), ("table", ptr(10) + 4, "aligned"),
              ("cand", None), ("sets", None), ("delta_out", None), ("accepting_out", None), ("counts", None)]
    for fn, own in ((lib.glb_nfa_closure, closure), (lib.glb_nfa_subset_round, search)):
        assert fn(None, None) == _lib.GLB_EINVAL
        for field, value, *named in shared + own:
            over = {field: value}
            if (field, value) == ("n_important", 4097):
                over.update(n_states=5000, n_words=65)
            assert fn(C.byref(block(**over)), None) == _lib.GLB_EINVAL, (field, value)
            assert (named or [field])[0] in _lib.last_error(), (field, value, _lib.last_error())
    assert all(not k.any() for k in keep)  # nothing was written
