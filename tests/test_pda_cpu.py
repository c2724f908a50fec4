"""`constraints.BytePDA` and `constraints.PDAConstraint` without a GPU: the constructor's refusals; `from_dfa` against the
automaton it wraps; `dyck` against a counter-and-stack checker; `json()` against `json.loads` over a seeded corpus at four depth
bounds; `trim()` against a brute-force search over configurations; the restatement tests/pda_ref.py (the yardstick of the GPU
tests) against tests/lazy_ref.py and tests/dfa_ref.py; the block's size, constants, symbols and every GLB_EINVAL with no device;
the constraint's argument errors with `None` as the device."""
import ctypes as C
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

import genlm_backend_amd
from genlm_backend_amd import _lib, constraints
from genlm_backend_amd.constraints import ByteDFA, ByteNFA, BytePDA, ByteWFSA, PDAConstraint  # (no test here passes without the classes)
from genlm_backend_amd.constraints.pda import POP, _json_tables
from tests import dfa_ref as R
from tests import lazy_ref as L
from tests import pda_ref as P
from tests.test_regex_cpu import PATTERNS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bytes(pattern):
    return pattern.encode("utf-8") if isinstance(pattern, str) else pattern


# ---- the constructor ------------------------------------------------------------------------------------------------------------
def test_constructor_refusals_one_by_one():
    ok = np.full((2, 3, 256), -1, np.int32)
    ok[0, :, 40] = 0 | 1 << 24
    ok[0, 1, 41] = 1 | POP << 24
    acc = np.array([True, False])
    BytePDA(ok, acc, 0)

    def bad(match, delta=ok, accepting=acc, start=0, **cell):
        delta = delta.copy()
        for at, v in cell.items():
            delta[tuple(int(x) for x in at.split("_")[1:])] = v
        with pytest.raises(ValueError, match=match):
            BytePDA(delta, accepting, start)

    bad("pop in plane 0", c_0_0_41=1 | POP << 24)
    bad(r"op in \(2, 127\)", c_0_1_50=0 | 3 << 24)
    bad(r"op in \(2, 127\)", c_1_2_50=1 | 126 << 24)
    bad("next outside", c_1_2_50=2)
    bad("next outside", c_1_2_50=0xffffff | 1 << 24)
    bad("-1 or next", c_0_0_0=-2)
    bad("int32", delta=ok.astype(np.int64))
    bad(r"\[S, G \+ 1, 256\]", delta=ok[:, :, :255])
    bad(r"\[S, G \+ 1, 256\]", delta=ok[:, :1])
    bad(r"\[S, G \+ 1, 256\]", delta=ok[0])
    bad(r"\[S, G \+ 1, 256\]", delta=ok[:0])
    bad(r"\[S, G \+ 1, 256\]", delta=np.full((1, 128, 256), -1, np.int32))
    bad("accepting must be", accepting=np.array([True]))
    bad("accepting must be bool", accepting=np.array([1, 0]))
    for start in (2, -1, True, 0.0, None):
        bad("start", start=start)
    BytePDA(np.full((1, 127, 256), -1, np.int32), np.array([True]), 0)  # G = 126 is the most


@pytest.mark.parametrize("pattern", PATTERNS, ids=[repr(p) for p in PATTERNS])
def test_from_dfa_accepts_what_the_automaton_does(pattern):
    d = ByteDFA.from_regex(pattern)
    pda = BytePDA.from_dfa(d)
    assert pda.n_symbols == 1 and pda.n_states == d.n_states and np.array_equal(pda.delta[:, 0], pda.delta[:, 1])
    letters = np.frombuffer(bytes(dict.fromkeys(_bytes(pattern) + b"ab0\n\xff")), np.uint8)
    rng = np.random.default_rng(len(letters))
    for _ in range(300):
        s = bytes(rng.choice(letters, int(rng.integers(0, 7))))
        assert pda.accepts(s, 1) == d.accepts(s), s
    assert pda.accepts(b"", 1) == d.accepts(b"")


def test_from_dfa_refuses_weights():
    with pytest.raises(ValueError, match="unweighted"):
        BytePDA.from_dfa(ByteWFSA.from_dfa(ByteDFA.from_regex(rb"ab*")))
    with pytest.raises(ValueError, match="ByteDFA"):
        BytePDA.from_dfa(ByteNFA.from_regex(rb"ab*"))


# ---- dyck -------------------------------------------------------------------------------------------------------------------------
def _balanced(s, max_depth):
    stack = []
    for ch in s:
        if ch in b"([":
            if len(stack) == max_depth:
                return False
            stack.append(ch)
        elif ch in b")]":
            if not stack or stack.pop() != {41: 40, 93: 91}[ch]:
                return False
    return not stack


def test_dyck_against_a_stack_checker():
    pda = BytePDA.dyck([(b"(", b")"), (b"[", b"]")], b"x")
    assert pda.n_states == 1 and pda.n_symbols == 2
    rng = np.random.default_rng(3)
    strings = [bytes(rng.choice(np.frombuffer(b"()[]x", np.uint8), int(rng.integers(0, 13)), p=[.27, .27, .18, .18, .1])) for _ in range(2000)]
    strings += [b"", b"()", b"(]", b"([)]", b"((((((((()))))))))", b"(((((((((())))))))))", b"y"]
    for depth in (1, 2, 9):
        got = [pda.accepts(s, depth) for s in strings]
        assert got == [_balanced(s, depth) and b"y" not in s for s in strings]
        assert 50 < sum(got) < len(got) - 50
    assert sum(pda.accepts(s, 9) for s in strings) > sum(pda.accepts(s, 2) for s in strings) > sum(pda.accepts(s, 1) for s in strings)
    for pairs, other in (([], b""), ([(b"(", b"(")], b""), ([(b"(", b")")], b")"), ([(b"((", b")")], b"")):
        with pytest.raises(ValueError, match="dyck"):
            BytePDA.dyck(pairs, other)


# ---- json -------------------------------------------------------------------------------------------------------------------------
HAND = [b"01", b"1.", b".5", b"+1", b"-", b"1e", b'"\\x"', b'"a\nb"', b'"\\ud800"', b'"\xc0\xaf"', b"[1,]", b'{"a"}', b"{,}", b" 1 ", b"nul",
        b"NaN", b"-Infinity", b"Infinity", b"", b" ", b"0", b"-0", b"-0.0e-0", b"1E+2", b"[]", b"{}", b"[ ]", b"{ }", b'""', b'"\\u00e9\\n\\/"',
        b'"\xf4\x90\x80\x80"', b'"\xed\xa0\x80"', b'"\xf0\x9f\x98\x80"', b'"\xe0\x80\x80"', b'"\x7f"', b'"\x1f"', b"\xef\xbb\xbf1", b"[1 2]",
        b'{"a":1,}', b'{"a":1 "b":2}', b'{1:2}', b"[[[[[[[[1]]]]]]]]", b"[[[[[[[[[1]]]]]]]]]", b"true false", b"\t\r\n true\n", b"tru", b"nulll",
        b'{"a":{"b":{"c":[]}}}', b"1\x0b", b"[1]]", b"[[1]", b'"abc', b'{"a":"b"}x']


def _random_value(rng, depth):
    kind = int(rng.integers(0, 13 if depth > 0 else 7))  # (with depth to spare, a container every other time)
    chars = ["a", "b", "é", "€", "😀", '"', "\\", "\n", " ", " ", "/", "\x7f", "0"]
    text = lambda: "".join(chars[int(i)] for i in rng.integers(0, len(chars), int(rng.integers(0, 5))))
    if kind == 0:
        return None
    if kind == 1:
        return bool(rng.integers(0, 2))
    if kind == 2:
        return int(rng.integers(-1000, 1000))
    if kind == 3:
        return float(rng.normal()) * 10.0 ** int(rng.integers(-12, 12))
    if kind in (4, 5, 6):
        return text()
    if kind % 2:
        return [_random_value(rng, depth - 1) for _ in range(int(rng.integers(0, 4)))]
    return {text(): _random_value(rng, depth - 1) for _ in range(int(rng.integers(0, 4)))}


def _corpus():
    rng = np.random.default_rng(8259)
    good = []
    for i in range(160):
        v = _random_value(rng, i % 6)
        seps = (",", ":") if i % 2 else None
        good.append(json.dumps(v, ensure_ascii=bool(i // 2 % 2), separators=seps).encode("utf-8"))
    out = list(good)
    pool = np.frombuffer(b'{}[]",:\\ 0123456789-+.eEtfnu\n\x00\x80\xe2\xff', np.uint8)
    for s in good:
        if not s:
            continue
        for kind in range(3):
            at = int(rng.integers(0, len(s)))
            b = bytes([int(rng.choice(pool))])
            out.append(s[:at] + (b"" if kind == 0 else b) + s[at + (kind != 1):])
    return list(dict.fromkeys(out + HAND))


def _raises(name):
    raise ValueError(name)


def _nesting(text):
    """The deepest nesting of brackets outside strings in a text that `json.loads` took."""
    depth = most = 0
    in_string = escaped = False
    for ch in text:
        if in_string:
            if escaped:
                escaped = False
            elif ch == "\\":
                escaped = True
            elif ch == '"':
                in_string = False
        elif ch == '"':
            in_string = True
        elif ch in "[{":
            depth += 1
            most = max(most, depth)
        elif ch in "]}":
            depth -= 1
    return most


def _json_depth(s):
    """The nesting depth of the value `s` holds, or None where `json.loads` refuses it."""
    try:
        text = s.decode("utf-8", "strict")
        json.loads(text, parse_constant=_raises)
    except ValueError:  # (UnicodeDecodeError and JSONDecodeError are ValueErrors)
        return None
    return _nesting(text)


CORPUS = _corpus()
DEPTHS = [_json_depth(s) for s in CORPUS]


def test_json_against_json_loads():
    pda = BytePDA.json()
    assert 24 <= pda.n_states <= 60 and pda.n_symbols == 2
    assert len(CORPUS) >= 300
    for max_depth in (0, 1, 3, 8):
        for s, d in zip(CORPUS, DEPTHS):
            assert pda.accepts(s, max_depth) == (d is not None and d <= max_depth), (s, d, max_depth)
    accepted = sum(d is not None and d <= 8 for d in DEPTHS)
    assert accepted >= 100 and len(CORPUS) - accepted >= 100
    assert sum(d is not None and d > 3 for d in DEPTHS) > 5 and DEPTHS[CORPUS.index(b"[[[[[[[[[1]]]]]]]]]")] == 9
    assert DEPTHS[CORPUS.index(b'"\\ud800"')] == 0 and DEPTHS[CORPUS.index(b"NaN")] is None  # (what json.loads itself says of the two)


# ---- trim -------------------------------------------------------------------------------------------------------------------------
def _hand_automata():
    """Two small automata with a dead-end branch: brackets with a state that never returns and a push nobody pops; a^n b^n
    with a sink that pops but never accepts."""
    e = lambda nxt, op=0: nxt | op << 24
    d = np.full((3, 3, 256), -1, np.int32)
    d[0, :, ord("(")], d[0, 1, ord(")")], d[0, :, ord("x")] = e(0, 1), e(0, POP), e(0)
    d[0, :, ord("d")], d[1, :, ord("d")] = e(1), e(1)  # state 1: a keep loop that never accepts
    d[0, :, ord("p")], d[2, :, ord("x")] = e(2, 2), e(2)  # state 2: under a symbol that nothing pops
    one = BytePDA(d, np.array([True, False, False]), 0)
    d = np.full((3, 2, 256), -1, np.int32)
    d[0, :, ord("a")], d[0, 1, ord("b")], d[1, 1, ord("b")] = e(0, 1), e(1, POP), e(1, POP)
    d[0, :, ord("c")], d[2, :, ord("c")], d[2, 1, ord("b")] = e(2), e(2), e(2, POP)  # state 2 pops, and accepts nothing
    two = BytePDA(d, np.array([True, True, False]), 0)
    return one, two


def _reaches_acceptance(pda, depth=3):
    """The configurations of at most `depth` symbols from which an accepting state on the empty stack is reachable through
    such configurations: a search backwards over every configuration and every distinct entry."""
    G = pda.n_symbols
    stacks = [bytes(t) for n in range(depth + 1) for t in itertools.product(range(1, G + 1), repeat=n)]
    back = {}
    for q in range(pda.n_states):
        for stack in stacks:
            row = pda.delta[q, stack[-1] if stack else 0]
            for b in np.unique(row, return_index=True)[1]:
                nxt = pda.step((q, stack), int(b), depth)
                if nxt is not None:
                    back.setdefault(nxt, []).append((q, stack))
    good = {(q, b"") for q in range(pda.n_states) if pda.accepting[q]}
    todo = list(good)
    while todo:
        for c in back.get(todo.pop(), ()):
            if c not in good:
                good.add(c)
                todo.append(c)
    return good


@pytest.mark.parametrize("which", ["json", "brackets", "anbn"])
def test_trim_keeps_only_entries_that_can_reach_acceptance(which):
    raw = BytePDA(*_json_tables()) if which == "json" else _hand_automata()[which == "anbn"]
    cut = raw.trim()
    assert cut is not raw and (cut.delta >= 0).sum() < (raw.delta >= 0).sum() and not (cut.delta[raw.delta < 0] >= 0).any()
    good = _reaches_acceptance(cut)
    pairs = {(q, stack[-1] if stack else 0) for q, stack in good}
    on = cut.delta >= 0
    op = cut.delta >> 24
    for q, g, b in zip(*np.nonzero(on & (op != POP))):
        target = (int(cut.delta[q, g, b]) & 0xffffff, int(op[q, g, b]) or int(g))
        assert target in pairs, (q, g, b, target)
    assert np.array_equal(cut.delta[op == POP], raw.delta[op == POP]) and ((raw.delta >> 24 == POP) & (raw.delta >= 0)).sum() == (on & (op == POP)).sum()
    again = cut.trim()
    assert np.array_equal(again.delta, cut.delta)
    if which == "json":
        assert np.array_equal(cut.delta, BytePDA.json().delta)
        strings = CORPUS
    else:
        rng = np.random.default_rng(1)
        strings = [bytes(rng.choice(np.frombuffer(b"()xdpabc", np.uint8), int(rng.integers(0, 9)))) for _ in range(1500)] + [b"", b"ab", b"aabb", b"(x)"]
        assert raw.accepts(b"(x)(())", 3) or raw.accepts(b"aaabbb", 3)
    for depth in (1, 3, 8):
        assert [cut.accepts(s, depth) for s in strings] == [raw.accepts(s, depth) for s in strings]


# ---- the restatement against the restatements of the existing paths -------------------------------------------------------------------
def _small_vocab(pattern):
    rank = lambda b: (0 if bytes([b]).isalnum() or b >= 128 else 1 if b in b"-. " else 2, b)
    letters = list(dict.fromkeys(sorted(set(_bytes(pattern)), key=rank) + [97, 98, 48, 10]))[:6]
    vocab = [bytes([b]) for b in letters]
    vocab += [bytes([a, b]) for a in letters[:4] for b in letters[:4]] + [bytes([a, b, a]) for a in letters[:3] for b in letters[:3]]
    vocab += [b"", bytes(letters[:1]), b"<eos>"]
    return vocab, len(vocab) - 1, (len(vocab) - 2, len(vocab) - 1)


def _live_dfa(pattern):
    """The pattern's automaton with the arcs into states that accept nothing removed: what is left of it is reached only
    while something can still be accepted, as a set of `lazy_ref` is."""
    d = ByteDFA.from_regex(pattern)
    delta = d.delta.copy()
    delta[(delta >= 0) & ~d.live[np.maximum(delta, 0)]] = -1
    return ByteDFA(delta, d.accepting, d.start)


@pytest.mark.parametrize("pattern", PATTERNS[1::2], ids=[repr(p) for p in PATTERNS[1::2]])
def test_restatement_over_from_dfa_is_the_existing_restatements(pattern):
    d = _live_dfa(pattern)
    assert d.live[d.start]
    vocab, eos, skip = _small_vocab(pattern)
    pref = P.Ref(BytePDA.from_dfa(d), vocab, eos, skip, max_depth=1)
    lref, dref = L.Ref(ByteNFA.from_dfa(d), vocab, eos, skip), R.Ref(d.delta, d.accepting, d.start, vocab, eos, skip)
    rng = np.random.default_rng(len(_bytes(pattern)))
    n, ld = 300, 6
    tokens = rng.integers(0, len(vocab) - 2, (n, ld)).astype(np.int32)
    tokens[rng.random((n, ld)) < 0.02] = len(vocab) - 2
    tokens[rng.random((n, ld)) < 0.01] = len(vocab)
    to = rng.integers(0, ld + 1, n).astype(np.int32)
    cut = np.minimum(to, rng.integers(0, ld + 1, n)).astype(np.int32)
    zero = np.zeros(n, np.int32)
    first, first_l = pref.advance(None, tokens, zero, cut), lref.advance(None, tokens, zero, cut)
    assert np.array_equal(first, first_l)
    out = pref.advance(first, tokens, cut, to)
    assert np.array_equal(out, lref.advance(first_l, tokens, cut, to)) and pref.n_states == lref.n_states and not pref.overflow
    assert np.array_equal(pref.accepting(), lref.accepting())
    for i in range(n):  # the automaton's own particle
        s = dref.advance(d.start, tokens[i, :to[i]])
        assert (out[i] < 0) == (s < 0) and (s < 0 or pref.configs()[out[i]] == (s, b""))
    for s in range(min(pref.n_states, 6)):  # rows
        assert np.array_equal(pref.mask(s), lref.mask(s)) and np.array_equal(pref.mask(s), dref.mask(pref.configs()[s][0]))
    words = pref.words()
    assert words.shape == (pref.n_states, 2) and not words[:, 1].any() and words[:, 0].tolist() == [c[0] for c in pref.configs()]


def test_restatement_overflow_cut_and_degenerate_ranges():
    d = _live_dfa(rb"(a|b)*a(a|b){3}")
    vocab, eos, skip = _small_vocab(rb"ab")
    nfa = ByteNFA.from_dfa(d)
    tokens = np.array([[0], [1], [0], [4], [5], [8], [9]], np.int32)  # a b a aa ab ba bb
    frm, to = np.zeros(7, np.int32), np.ones(7, np.int32)
    make = lambda **kw: (P.Ref(BytePDA.from_dfa(d), vocab, eos, skip, max_depth=1, **kw), L.Ref(nfa, vocab, eos, skip, **kw))
    whole, whole_l = make()
    want = whole.advance(None, tokens, frm, to)
    assert np.array_equal(want, whole_l.advance(None, tokens, frm, to)) and not whole.overflow and whole.n_states == 4
    tight, tight_l = make(max_states=3)
    got = tight.advance(None, tokens, frm, to)
    assert np.array_equal(got, tight_l.advance(None, tokens, frm, to)) and tight.overflow and tight_l.overflow
    assert got.tolist() == [1, 0, 1, 2, -1, 1, 0] and tight.n_states == 3 and tight.configs() == whole.configs()[:3]
    exact, _ = make(max_states=4)
    assert exact.advance(None, tokens, frm, to).tolist() == want.tolist() and not exact.overflow
    r, r_l = make()
    t2 = np.array([[0, 1]] * 6, np.int32)
    args = (np.array([0, 0, 0, -1, 1, 0], np.int32), t2, np.array([1, 2, 0, 0, 0, -1], np.int32), np.array([1, 1, 3, 1, 1, 1], np.int32))
    assert r.advance(*args).tolist() == r_l.advance(*args).tolist() == [0, -1, -1, -1, -1, -1]


def test_restatement_walks_a_stack():
    """What no regular restatement has: pushes, pops below where a token began, the depth bound, acceptance on the empty stack."""
    pda = BytePDA.dyck([(b"(", b")"), (b"[", b"]")], b"x")
    vocab = [b"(", b")", b"[", b"]", b"x", b"()", b"))[[[", b"((((", b"", b"<eos>"]
    ref = P.Ref(pda, vocab, 9, (9,), max_depth=4)
    z = lambda *v: np.array(v, np.int32)
    got = ref.advance(None, z(0, 2, 7, 5, 1, 8, 10).reshape(-1, 1), np.zeros(7, np.int32), np.ones(7, np.int32))
    assert got.tolist() == [1, 2, 3, 0, -1, -1, -1]
    assert ref.configs() == [(0, b""), (0, b"\x01"), (0, b"\x02"), (0, b"\x01\x01\x01\x01")]
    assert ref.accepting().tolist() == [True, False, False, False]
    deep = ref.advance(z(1, 3), z(0, 2, 6, 6).reshape(2, 2), z(0, 0), z(2, 2))  # ( [ from "(": 3 deep; ))[[[ from 4 deep: 5 deep
    assert deep.tolist() == [4, -1] and ref.configs()[4] == (0, b"\x01\x01\x02")
    again = ref.advance(z(3), z(1, 6).reshape(1, 2), z(0), z(2))  # ) then ))[[[ : pops three below where it began, pushes three
    assert ref.configs()[again[0]] == (0, b"\x01\x02\x02\x02")
    assert ref.allowed(0).tolist() == [True, False, True, False, True, True, False, True, False, True]
    assert ref.allowed(3).tolist() == [False, True, False, False, True, False, False, False, False, False]
    assert np.array_equal(ref.words()[4], np.array([3 << 32, 0x020101], np.uint64)) and ref.words().shape[1] == 2


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_in_the_signature_table_under_their_own_prefix(tmp_path):
    from genlm_backend_amd.engine import HipEngine

    new = {name for name in _lib.SYMBOLS if name.startswith("glb_pda_")}
    assert new == {"glb_pda_init", "glb_pda_advance", "glb_pda_serve"} == set(HipEngine.PDA_CALLS)
    for other in (HipEngine.DFA_CALLS, HipEngine.FSA_CALLS, HipEngine.NFA_CALLS, HipEngine.LAZY_CALLS):
        assert not new & other
    assert len(HipEngine.LAZY_CALLS) == 3 and len(HipEngine.DFA_CALLS) == 13 and _lib.ABI_VERSION == 9
    for name in new:
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and args[0]._type_ is _lib.PdaArgs
    for name in ("glb_dfa_advance", "glb_lazy_serve", "glb_nfa_closure", "glb_pda_nothing", ""):  # (refused before the engine is looked at)
        with pytest.raises(ValueError):
            HipEngine.pda_call(None, name, None)
    assert genlm_backend_amd.BytePDA is constraints.BytePDA and genlm_backend_amd.PDAConstraint is constraints.PDAConstraint
    assert genlm_backend_amd.__all__[-1] == "minimize"
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "glb.h"\nint main(void) { printf("%zu %zu %d %d %d %d", sizeof(glb_pda_args), '
                   'offsetof(glb_pda_args, max_token_bytes), GLB_PDA_MAX_DEPTH, GLB_PDA_STATUS, GLB_PDA_OVERFLOW, GLB_PDA_BUG); return 0; }\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "size")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "size")]).split()]
    assert out == [C.sizeof(_lib.PdaArgs), _lib.PdaArgs.max_token_bytes.offset, _lib.PDA_MAX_DEPTH, _lib.PDA_STATUS, _lib.PDA_OVERFLOW, _lib.PDA_BUG]
    assert out[2:] == [504, 8, 1, 2]


def test_c_abi_refuses_before_any_launch():
    lib = _lib.load()
    keep = [np.zeros(64, np.int64) for _ in range(22)]
    ptr = lambda i: keep[i].ctypes.data

    def block(dfa=None, **over):
        p = _lib.PdaArgs()
        p.struct_size = C.sizeof(_lib.PdaArgs)
        d = p.dfa
        d.struct_size, d.n_states, d.eos_id, d.vocab, d.n_bytes, d.n, d.ld = C.sizeof(_lib.DfaArgs), 8, 2, 40, 64, 4, 2
        for i, k in enumerate(("tok_bytes", "tok_ptr", "skip", "tokens", "from_", "to", "state_in", "state_out", "bank", "row_of_state", "work",
                               "counters", "out_rows")):
            setattr(d, k, ptr(i))
        d.bank_ld, d.capacity, d.max_work = 2, 4, 2
        for k, v in (dfa or {}).items():
            setattr(d, k, v)
        p.n_pda_states, p.n_symbols, p.start, p.max_depth, p.n_words, p.max_states, p.max_token_bytes = 4, 2, 0, 9, 3, 8, 4
        for i, k in enumerate(("delta", "accepting", "table", "cand", "counts", "configs", "accepting_out", "status")):
            setattr(p, k, ptr(13 + i))
        p.table_slots, p.cand_rows = 16, 8
        for k, v in over.items():
            setattr(p, k, v)
        return p

    shared = [("struct_size", 0), ("struct_size", C.sizeof(_lib.PdaArgs) - 8), ("max_states", 0), ("max_states", (1 << 22) + 1),
              ("n_pda_states", 0), ("n_pda_states", (1 << 24) + 1), ("n_symbols", 0), ("n_symbols", 127), ("start", 4), ("start", -1),
              ("max_depth", 0), ("max_depth", 505, "504"), ("n_words", 2), ("n_words", 4), ("delta", None), ("accepting", None, "accepting is null"),
              ("table_slots", 8), ("table_slots", 17), ("table", None), ("table", ptr(15) + 4, "aligned"), ("configs", None),
              ("configs", ptr(18) + 4, "configs is not aligned"), ("accepting_out", None), ("status", None), ("epoch", ptr(0), "in part"),
              ("row_state", ptr(0), "in part")]
    inner = [("struct_size", 0, "glb_dfa_args"), ("struct_size", C.sizeof(_lib.DfaArgs) + 8, "glb_dfa_args"), ("vocab", 0, "vocab")]
    own = [
        (lib.glb_pda_init, ([], [("bank", None, "bank"), ("bank_ld", 1, "bank_ld"), ("capacity", 1, "capacity"), ("counters", None, "bank")])),
        (lib.glb_pda_advance, ([("cand", None), ("cand", ptr(16) + 4, "cand is not aligned"), ("counts", None), ("cand_rows", 0), ("cand_rows", 9)],
                              [("n", 0, "n "), ("tokens", None, "null"), ("state_out", None, "null"), ("ld", 0, "ld"), ("tok_ptr", None, "vocabulary")])),
        (lib.glb_pda_serve, ([("max_token_bytes", 0)], [("n", 0, "n "), ("state_in", None, "null"), ("out_rows", None, "null"),
                                                        ("max_work", 0, "max_work"), ("skip", None, "vocabulary"), ("work", None, "bank")])),
    ]
    for fn, (outer, of_dfa) in own:
        assert fn(None, None) == _lib.GLB_EINVAL
        for field, value, *named in shared + outer:
            assert fn(C.byref(block(**{field: value})), None) == _lib.GLB_EINVAL, (field, value)
            assert (named or [field])[0] in _lib.last_error(), (field, value, _lib.last_error())
        for field, value, named in inner + of_dfa:
            assert fn(C.byref(block(dfa={field: value})), None) == _lib.GLB_EINVAL, (field, value)
            assert named in _lib.last_error(), (field, value, _lib.last_error())
    for depth, words in ((1, 2), (8, 2), (9, 3), (16, 3), (17, 4), (504, 64)):  # the byte-to-word boundaries: one word off is refused
        assert lib.glb_pda_init(C.byref(block(max_depth=depth, n_words=words + 1)), None) == _lib.GLB_EINVAL and "n_words" in _lib.last_error()
        assert lib.glb_pda_init(C.byref(block(max_depth=depth, n_words=words, table=None)), None) == _lib.GLB_EINVAL and "table" in _lib.last_error()
    assert all(not k.any() for k in keep)  # nothing was written


def test_argument_errors_need_no_device():
    pda = BytePDA.dyck([(b"(", b")")])
    vocab = [b"(", b")", b"<eos>"]
    for bad in (None, "()", ByteDFA.from_regex(rb"ab*"), ByteNFA.from_regex(rb"ab*")):
        with pytest.raises(ValueError, match="BytePDA"):
            PDAConstraint(None, bad, vocab, 2)
    for bad in (0, -1, True, 1.5, None, "8", 505):
        with pytest.raises(ValueError, match="max_depth"):
            PDAConstraint(None, pda, vocab, 2, max_depth=bad)
    for bad in (0, -1, True, 1.5, None, "8", (1 << 22) + 1):
        with pytest.raises(ValueError, match="max_states"):
            PDAConstraint(None, pda, vocab, 2, max_states=bad)
    with pytest.raises(ValueError, match="on_full"):
        PDAConstraint(None, pda, vocab, 2, on_full="drop")
    with pytest.raises(ValueError, match="empty vocabulary"):
        PDAConstraint(None, pda, [], 0)
    with pytest.raises(ValueError, match="mask_bank_bytes=8"):
        PDAConstraint(None, pda, vocab, 2, mask_bank_bytes=8)
    assert PDAConstraint.weighted is False and PDAConstraint.start_logw == 0.0
    # every argument passes: with no device the next thing missing is the engine itself
    with pytest.raises(AttributeError):
        PDAConstraint(None, pda, vocab, 2, max_depth=504, max_states=1 << 22)
