"""`constraints.product` without a GPU: the NumPy restatement tests/fsa_product_ref.py (the yardstick of the GPU tests) against
the operands' own `accepts` and `path_logw`, the argument errors that must be raised before a device is looked at, and the
new entries of the signature table."""
import ctypes as C
import itertools

import numpy as np
import pytest

import genlm_backend_amd
from genlm_backend_amd import _lib, constraints
from genlm_backend_amd.constraints import ByteDFA, ByteWFSA
from tests import dfa_min_ref as M
from tests import dfa_ref as R
from tests import fsa_product_ref as F
from tests.test_regex_cpu import PATTERNS

OPS = {"and": lambda x, y: x and y, "or": lambda x, y: x or y, "sub": lambda x, y: x and not y}
# (a, b, the four letters the strings are drawn from): patterns of tests/test_regex_cpu.PATTERNS and automata of dfa_ref
PAIRS = [
    (rb"a*b+c?", rb"[abc]+", b"abcd"),
    (rb"(ab)*(?:cd)+e?", rb"[a-cx-z]*", b"abcd"),
    (rb"-?(0|[1-9][0-9]*)(\.[0-9]+)?", "digits", b"-0.7"),
    ("random37", rb".*a.{2}", b"0a9y"),
    ("trap", "everything", b"yn01"),
    ("random37", "digits", b"0a9y"),
    (rb"a{2,4}", rb"a{2,}b", b"ab01"),
    (rb"((a|b)*c)+|()", rb"(a(b(c|d)*)?)+", b"abcd"),
    (rb"( yes| no| maybe)", rb"[^a-c]", b" yno"),
]
assert all(p in PATTERNS for pair in PAIRS for p in pair[:2] if isinstance(p, bytes))


def _dfa(x):
    return ByteDFA.from_regex(x) if isinstance(x, bytes) else ByteDFA(*R.automata()[x])


def _samples(dfa, n, seed):
    """Up to n strings that `dfa` accepts: seeded walks over the arcs into live states."""
    rng, out = np.random.default_rng(seed), []
    for _ in range(4 * n):
        s, text = dfa.start, bytearray()
        while dfa.live[s] and len(text) < 12:
            if dfa.accepting[s] and rng.random() < 0.3:
                break
            arcs = [b for b in range(256) if dfa.delta[s, b] >= 0 and dfa.live[dfa.delta[s, b]]]
            if not arcs:
                break
            b = int(rng.choice(arcs))
            text.append(b)
            s = int(dfa.delta[s, b])
        if dfa.accepts(bytes(text)):
            out.append(bytes(text))
    return out[:n]


def _strings(a, b, letters):
    for n in range(6):
        for t in itertools.product(letters, repeat=n):
            yield bytes(t)
    yield from _samples(a, 40, 1)
    yield from _samples(b, 40, 2)


@pytest.mark.parametrize("pa,pb,letters", PAIRS, ids=[f"{a!r}-{b!r}" for a, b, _ in PAIRS])
def test_restatement_accepts_what_the_operands_say(pa, pb, letters):
    a, b = _dfa(pa), _dfa(pb)
    strings = list(_strings(a, b, letters))
    in_a, in_b = [a.accepts(s) for s in strings], [b.accepts(s) for s in strings]
    for op, rule in OPS.items():
        p = F.product(a, b, op)
        assert [F.accepts(p, s) for s in strings] == [rule(x, y) for x, y in zip(in_a, in_b)], op
        # state 0 is the start; after the trim every state is reachable and live (an empty language: state 0 alone, not live)
        S = len(p["accepting"])
        host = ByteDFA(p["delta"], p["accepting"], 0)
        assert p["start"] == 0 and M.reachable(p["delta"], 0).all() and np.array_equal(host.live, p["live"])
        assert np.array_equal(p["live"], R.live(p["delta"].astype(np.int64), p["accepting"]))
        assert p["live"].all() or (S == 1 and not p["accepting"][0] and (p["delta"] == -1).all() and p["pairs"].tolist() in ([[-1, -1]], [[a.start, b.start]]))
        assert p["pairs"].shape == (S, 2) and p["pairs"].dtype == np.int32 and S <= p["untrimmed"]
        # the pairs are what the operands reach: walk every sample through all three
        for s in strings[-80:]:
            x, y, z = a.start, b.start, 0
            for byte in s:
                x = int(a.delta[x, byte]) if x >= 0 else -1
                y = int(b.delta[y, byte]) if y >= 0 else -1
                z = int(p["delta"][z, byte]) if z >= 0 else -1
                if z >= 0:
                    want = [x if x >= 0 and a.live[x] else -1, y if y >= 0 and b.live[y] else -1]
                    assert p["pairs"][z].tolist() == want


def test_numbering_is_the_queue_order():
    """[ab] then anything of two letters, against itself: the states come out breadth first, bytes ascending."""
    a = ByteDFA.from_regex(rb"(a|b)(c|d)")
    p = F.search(F.side(a), F.side(a), "and")
    first = p["delta"][0][p["delta"][0] >= 0]
    assert first.tolist() == sorted(first.tolist()) and first[0] == 1
    order = [int(t) for row in p["delta"] for t in row if t >= 0]
    seen = []
    for t in order:
        if t not in seen:
            seen.append(t)
    assert seen == list(range(1, len(p["accepting"])))


def _weights(dfa, k, m):
    arc = np.where(dfa.delta >= 0, -np.float32(k) * (1 + np.arange(256) % 7).astype(np.float32), -np.inf).astype(np.float32)
    fin = np.where(dfa.accepting, -np.float32(m) * (1 + np.arange(dfa.n_states) % 3).astype(np.float32), -np.inf).astype(np.float32)
    return ByteWFSA(dfa.delta, arc, fin, dfa.start)


WEIGHTED = [PAIRS[i] for i in (0, 2, 3, 7)]  # (pairs whose languages meet)


@pytest.mark.parametrize("pa,pb,letters", WEIGHTED, ids=[f"{a!r}-{b!r}" for a, b, _ in WEIGHTED])
def test_restated_weights_are_one_float32_addition_an_arc(pa, pb, letters):
    a, b = _weights(_dfa(pa), 0.1, 0.3), _weights(_dfa(pb), 0.2, 0.7)
    p = F.product(a, b, "and")
    both = 0
    for s in _strings(a, b, letters):
        x, y, w = a.start, b.start, np.float32(0.0)
        for byte in s:  # the order the restatement states: each arc's float32(wa + wb), summed left to right, then the final
            if x < 0 or y < 0 or a.delta[x, byte] < 0 or b.delta[y, byte] < 0:
                x = -1
                break
            w = np.float32(w + np.float32(a.arc_logw[x, byte] + b.arc_logw[y, byte]))
            x, y = int(a.delta[x, byte]), int(b.delta[y, byte])
        want = np.float32(w + np.float32(a.final_logw[x] + b.final_logw[y])) if x >= 0 else np.float32(-np.inf)
        got = F.path_logw(p, s)
        assert got.tobytes() == want.tobytes(), s
        assert np.isfinite(got) == (a.accepts(s) and b.accepts(s))
        both += bool(np.isfinite(got))
    assert both > 0
    # one side's weights pass through: the product with the other side unweighted weighs every string as that side does
    plain_b = ByteDFA(b.delta, b.accepting, b.start)
    for op in ("and", "sub"):
        q = F.product(a, plain_b, op)
        for s in _samples(a, 40, 3):
            inside = plain_b.accepts(s) == (op == "and")
            assert F.path_logw(q, s).tobytes() == (a.path_logw(s) if inside else np.float32(-np.inf)).tobytes()
    q = F.product(plain_b, a, "and")
    for s in _samples(a, 40, 3):
        assert F.path_logw(q, s).tobytes() == (a.path_logw(s) if plain_b.accepts(s) else np.float32(-np.inf)).tobytes()


def test_restatement_overflow():
    a, b = _dfa(rb"a{2,4}"), _dfa(rb"[abc]+")
    n = len(F.search(F.side(a), F.side(b), "or")["accepting"])
    with pytest.raises(ValueError, match="max_states"):
        F.search(F.side(a), F.side(b), "or", n - 1)
    assert len(F.search(F.side(a), F.side(b), "or", n)["accepting"]) == n


def test_argument_errors_need_no_device():
    a, b = _dfa(rb"abc"), _dfa(rb"[abc]+")
    wa = ByteWFSA.from_dfa(a)
    product = constraints.product
    assert genlm_backend_amd.product is product and genlm_backend_amd.__all__[-1] == "minimize"
    with pytest.raises(ValueError, match="op"):
        product(None, a, b, op="xor")
    with pytest.raises(ValueError, match="unweighted"):
        product(None, wa, b, op="or")
    with pytest.raises(ValueError, match="unweighted"):
        product(None, a, wa, op="or")
    with pytest.raises(ValueError, match="unweighted"):
        product(None, a, wa, op="sub")
    for bad in ((a.delta, a.accepting, 0), None, "abc"):
        with pytest.raises(ValueError, match="ByteDFA"):
            product(None, bad, b)
        with pytest.raises(ValueError, match="ByteDFA"):
            product(None, a, bad, op="sub")
    for bad in (0, -1, True, 1.5, None, "8"):
        with pytest.raises(ValueError, match="max_states"):
            product(None, a, b, max_states=bad)


def test_private_constructor_searches_nothing(monkeypatch):
    monkeypatch.setattr(ByteDFA, "_live", lambda self: pytest.fail("_live ran"))
    d = np.full((2, 256), -1, np.int32)
    d[0, 97] = 1
    x = ByteDFA._from_device(d, np.array([0, 1], np.uint8), 0, np.array([1, 1], np.uint8))
    assert type(x) is ByteDFA and x.accepts(b"a") and not x.accepts(b"") and x.live.dtype == np.bool_ and x.n_states == 2 and x.reachable.all()
    arc, fin = np.where(d >= 0, -0.5, -np.inf).astype(np.float32), np.array([-np.inf, -1.0], np.float32)
    w = ByteWFSA._from_device(d, fin > -np.inf, 0, np.ones(2, np.bool_), arc, fin)
    assert type(w) is ByteWFSA and w.path_logw(b"a") == np.float32(-1.5) and isinstance(w, ByteDFA)


def test_new_symbols_are_in_the_signature_table_under_their_own_prefix():
    from genlm_backend_amd.engine import HipEngine

    new = {name for name in _lib.SYMBOLS if name.startswith("glb_fsa_")}
    assert new == {"glb_fsa_product_round", "glb_fsa_live"} == set(HipEngine.FSA_CALLS)
    assert not any(name.startswith("glb_dfa_") for name in new) and not new & HipEngine.DFA_CALLS
    for name in new:
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and args[0]._type_ is _lib.FsaProductArgs
    assert C.sizeof(_lib.FsaProductArgs) == 200 and _lib.ABI_VERSION == 9  # (sizeof in C, include/glb.h compiled with gcc)
    for name in ("glb_dfa_refine", "glb_fsa_nothing", ""):  # (refused before the engine is looked at)
        with pytest.raises(ValueError):
            HipEngine.fsa_call(None, name, None)
    lib = _lib.load()
    p = _lib.FsaProductArgs()
    for fn in (lib.glb_fsa_product_round, lib.glb_fsa_live):
        assert fn(None, None) == _lib.GLB_EINVAL
        assert fn(C.byref(p), None) == _lib.GLB_EINVAL and "struct_size" in _lib.last_error()
