"""`constraints.ConstraintProduct` without a GPU: the constructor's refusals one by one, over parts that are the real classes with
nothing but the attributes the checks read; the block's size, last offset, constants, symbols and every GLB_EINVAL with no
device; and the restatement tests/conj_ref.py (the yardstick of the GPU tests) - over two DFAs against tests/dfa_ref.py on
tests/fsa_product_ref.py's conjunction, its numbering order, its overflow cut and the zero half word of an odd K."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import genlm_backend_amd
from genlm_backend_amd import _lib, constraints
from genlm_backend_amd.constraints import ByteDFA, BytePDA, ConstraintProduct, DeviceConstraint, LazyConstraint, PDAConstraint
from tests import conj_ref as J
from tests import dfa_ref as R
from tests import fsa_product_ref as F
from tests import pda_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the constructor ------------------------------------------------------------------------------------------------------------
def _stub(cls, eng, vocab=(b"a", b"b", b"<eos>"), eos_id=2, **over):
    """An object of a real constraint class that holds what the product's checks read and nothing else."""
    c = cls.__new__(cls)
    ptr = np.zeros(len(vocab) + 1, np.int32)
    np.cumsum([len(t) for t in vocab], out=ptr[1:])
    c.eng, c.dev, c.vocab, c.eos_id, c.words, c.n_bytes = eng, eng.device, len(vocab), eos_id, (len(vocab) + 31) // 32, int(ptr[-1])
    c._ptr, c._bytes = torch.from_numpy(ptr), torch.from_numpy(np.frombuffer(b"".join(vocab), np.uint8).copy())
    c.weighted, c.start_logw = False, 0.0
    for k, v in over.items():
        setattr(c, k, v)
    return c


def test_constructor_refusals_one_by_one():
    eng, other = SimpleNamespace(device=torch.device("cpu")), SimpleNamespace(device=torch.device("cpu"))
    a, b = _stub(DeviceConstraint, eng), _stub(PDAConstraint, eng)

    def bad(match, parts, engine=eng, **kw):
        with pytest.raises(ValueError, match=match):
            ConstraintProduct(engine, parts, **kw)

    bad("2 to 8 parts, got 1", [a])
    bad("2 to 8 parts, got 0", [])
    bad("2 to 8 parts, got 9", [_stub(LazyConstraint, eng) for _ in range(9)])
    bad("part 1 is a ByteDFA", [a, ByteDFA.from_regex(rb"ab*")])
    bad("part 0 is a NoneType", [None, a])
    bad("part 1 is the same object", [a, a])
    bad("part 2 is the same object", [a, b, a])
    bad("part 1 was made on a different engine", [a, _stub(DeviceConstraint, other)])
    bad("part 0 was made on a different engine", [a, b], engine=other)
    bad("part 1 was made on a different engine", [a, _stub(DeviceConstraint, eng, dev=torch.device("meta"))])
    bad("part 1 has vocab=4", [a, _stub(LazyConstraint, eng, vocab=(b"a", b"b", b"<eos>", b"c"))])
    bad("part 1 has vocab=3, eos_id=1", [a, _stub(LazyConstraint, eng, eos_id=1)])
    bad("part 1's vocabulary bytes differ", [a, _stub(LazyConstraint, eng, vocab=(b"a", b"c", b"<eos>"))])
    bad("part 2's vocabulary bytes differ", [a, b, _stub(LazyConstraint, eng, vocab=(b"ab", b"", b"<eos>"))])  # (the same bytes, other offsets)
    bad("part 1's vocabulary bytes differ", [a, _stub(LazyConstraint, eng, vocab=(b"a", b"bb", b"<eos"))])  # (the same offsets' count, other lengths)
    bad("on_full", [a, b], on_full="drop")
    for value in (0, -1, True, 1.5, None, "8", (1 << 22) + 1):
        bad("max_states", [a, b], max_states=value)
    bad("mask_bank_bytes=8", [a, b], mask_bank_bytes=8)
    bad(r"mask_bank_bytes=8 .*float32 weights", [a, _stub(DeviceConstraint, eng, weighted=True)], mask_bank_bytes=8)
    # every argument passes, a nested product's class among them: with no device the next thing missing is a part's automaton
    with pytest.raises(AttributeError):
        ConstraintProduct(eng, [a, b, _stub(LazyConstraint, eng), _stub(ConstraintProduct, eng)], max_states=1 << 22)
    assert "lifetime of its row ids" in ConstraintProduct.__doc__


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_in_the_signature_table_under_their_own_prefix(tmp_path):
    from genlm_backend_amd.engine import HipEngine

    new = {name for name in _lib.SYMBOLS if name.startswith("glb_conj_")}
    assert new == {"glb_conj_init", "glb_conj_unpack", "glb_conj_number", "glb_conj_serve"} == set(HipEngine.CONJ_CALLS)
    for other in (HipEngine.DFA_CALLS, HipEngine.FSA_CALLS, HipEngine.NFA_CALLS, HipEngine.LAZY_CALLS, HipEngine.PDA_CALLS):
        assert not new & other
    assert len(HipEngine.PDA_CALLS) == 3 and len(HipEngine.LAZY_CALLS) == 3 and len(HipEngine.DFA_CALLS) == 13 and _lib.ABI_VERSION == 9
    for name in new:
        res, args = _lib.SYMBOLS[name]
        assert res is C.c_int and args[0]._type_ is _lib.ConjArgs
    for name in ("glb_dfa_advance", "glb_pda_serve", "glb_lazy_serve", "glb_conj_nothing", ""):  # (refused before the engine is looked at)
        with pytest.raises(ValueError):
            HipEngine.conj_call(None, name, None)
    assert genlm_backend_amd.ConstraintProduct is constraints.ConstraintProduct
    assert genlm_backend_amd.__all__[-1] == "minimize"
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "glb.h"\nint main(void) { printf("%zu %zu %d %d %d %d %d", '
                   'sizeof(glb_conj_args), offsetof(glb_conj_args, epoch), GLB_CONJ_MAX_PARTS, GLB_CONJ_STATUS, GLB_CONJ_OVERFLOW, '
                   'GLB_CONJ_BUG, GLB_ABI_VERSION); return 0; }\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "size")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "size")]).split()]
    assert out == [C.sizeof(_lib.ConjArgs), _lib.ConjArgs.epoch.offset, _lib.CONJ_MAX_PARTS, _lib.CONJ_STATUS, _lib.CONJ_OVERFLOW, _lib.CONJ_BUG,
                   _lib.ABI_VERSION]
    assert out[2:] == [8, 8, 1, 2, 9] and _lib.ConjArgs._fields_[-1][0] == "epoch"


def test_c_abi_refuses_before_any_launch():
    lib = _lib.load()
    keep = [np.zeros(64, np.int64) for _ in range(24)]
    ptr = lambda i: keep[i].ctypes.data
    K = 3

    def block(dfa=None, part=None, **over):
        p = _lib.ConjArgs()
        p.struct_size = C.sizeof(_lib.ConjArgs)
        d = p.dfa
        d.struct_size, d.n_states, d.eos_id, d.vocab, d.n = C.sizeof(_lib.DfaArgs), 8, 2, 40, 4
        for i, k in enumerate(("state_in", "state_out", "bank", "row_of_state", "work", "counters", "out_rows")):
            setattr(d, k, ptr(i))
        d.bank_ld, d.capacity, d.max_work = 2, 4, 2
        for k, v in (dfa or {}).items():
            setattr(d, k, v)
        p.n_parts, p.n_words, p.max_states, p.table_slots, p.cand_rows, p.part_ld = K, 2, 8, 16, 8, 4
        for i, k in enumerate(("table", "tuples", "status", "counts", "part_states", "claim_states", "rep")):
            setattr(p, k, ptr(7 + i))
        for k in range(K):
            p.part_rows[k], p.part_bank[k], p.part_bank_ld[k], p.part_capacity[k] = ptr(14 + k), ptr(17 + k), 2, 3
        for k, v in over.items():
            setattr(p, k, v)
        for (name, k), v in (part or {}).items():
            getattr(p, name)[k] = v
        return p

    shared = [("struct_size", 0), ("struct_size", C.sizeof(_lib.ConjArgs) - 8), ("n_parts", 1), ("n_parts", 9), ("n_parts", 0),
              ("n_words", 1), ("n_words", 3), ("max_states", 0), ("max_states", (1 << 22) + 1), ("table_slots", 8), ("table_slots", 17),
              ("table", None), ("table", ptr(7) + 4, "table is not aligned"), ("tuples", None), ("tuples", ptr(8) + 4, "tuples is not aligned"),
              ("status", None), ("rep", None), ("epoch", ptr(0), "in part"), ("row_state", ptr(0), "in part")]
    inner = [("struct_size", 0, "glb_dfa_args"), ("struct_size", C.sizeof(_lib.DfaArgs) + 8, "glb_dfa_args"), ("vocab", 0, "vocab")]
    bank = [("bank", None, "bank"), ("bank_ld", 1, "bank_ld"), ("capacity", 1, "capacity"), ("counters", None, "bank"), ("work", None, "bank"),
            ("row_of_state", None, "bank")]
    particles = [("n", 0, "n "), ("n", (1 << 30) + 1, "n ")]
    states = [("part_states", None), ("part_ld", 3)]
    own = [
        (lib.glb_conj_init, [], inner + bank, [(("part_start", 2), -1, "part_start[2]"), (("part_start", 0), -5, "part_start[0]")]),
        (lib.glb_conj_unpack, states, inner + particles, []),
        (lib.glb_conj_number, states + [("counts", None), ("cand_rows", 0), ("cand_rows", 9)], inner + particles + [("state_out", None, "state_out")], []),
        (lib.glb_conj_serve, [("claim_states", None), ("wbank", ptr(2), "wbank_ld")],
         inner + bank + particles + [("state_in", None, "state_in"), ("out_rows", None, "out_rows"), ("max_work", 0, "max_work")],
         [(("part_rows", 1), None, "part_rows[1]"), (("part_bank", 2), None, "part_bank[2]"), (("part_bank_ld", 0), 1, "part_bank_ld[0]"),
          (("part_capacity", 1), 1, "part_capacity[1]"), (("part_weighted", 2), 1, "part_weighted[2]")]),
    ]
    for fn, outer, of_dfa, of_part in own:
        assert fn(None, None) == _lib.GLB_EINVAL
        for field, value, *named in shared + outer:
            assert fn(C.byref(block(**{field: value})), None) == _lib.GLB_EINVAL, (field, value)
            assert (named or [field])[0] in _lib.last_error(), (field, value, _lib.last_error())
        for field, value, named in of_dfa:
            assert fn(C.byref(block(dfa={field: value})), None) == _lib.GLB_EINVAL, (field, value)
            assert named in _lib.last_error(), (field, value, _lib.last_error())
        for key, value, named in of_part:
            assert fn(C.byref(block(part={key: value})), None) == _lib.GLB_EINVAL, (key, value)
            assert named in _lib.last_error(), (key, value, _lib.last_error())
    for parts, words in ((2, 1), (3, 2), (4, 2), (5, 3), (7, 4), (8, 4)):  # W = ceil(K / 2): one word off is refused
        assert lib.glb_conj_unpack(C.byref(block(n_parts=parts, n_words=words + 1)), None) == _lib.GLB_EINVAL and "n_words" in _lib.last_error()
        assert lib.glb_conj_unpack(C.byref(block(n_parts=parts, n_words=words, table=None)), None) == _lib.GLB_EINVAL and "table" in _lib.last_error()
    # a float bank: the row's elements are the tokens
    assert lib.glb_conj_init(C.byref(block(wbank=ptr(2), wbank_ld=39)), None) == _lib.GLB_EINVAL and "wbank_ld 39 < 40" in _lib.last_error()
    assert lib.glb_conj_serve(C.byref(block(wbank=ptr(2), wbank_ld=40, part={("part_weighted", 0): 1})), None) == _lib.GLB_EINVAL
    assert "part_bank_ld[0] 2 < 40" in _lib.last_error()
    assert all(not k.any() for k in keep)  # nothing was written


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
def _vocab(letters):
    """The single bytes of `letters`, their pairs, an empty token, a skipped one and the EOS."""
    singles = [bytes([b]) for b in letters]
    vocab = singles + [a + b for a in singles for b in singles] + [b"", singles[0], b"<eos>"]
    return vocab, len(vocab) - 1, (len(vocab) - 2, len(vocab) - 1)


def _random_calls(V, sizes, seed, ld=4):
    rng = np.random.default_rng(seed)
    for n in sizes:
        tokens = rng.integers(0, V, (n, ld)).astype(np.int32)
        frm = rng.integers(0, 2, n).astype(np.int32)
        yield tokens, frm, np.minimum(frm + rng.integers(0, 4, n), ld).astype(np.int32)


@pytest.mark.parametrize("patterns", [(rb"(a|b)*abb(a|b)*", rb"a*(ba*ba*)*"), (rb"a*(ba*ba*)*", rb"(a|b)*a(a|b)(a|b)")],
                         ids=["abb-even-b", "even-b-third-last"])
def test_two_dfas_against_the_product_automaton(patterns):
    """Two DFAs: the tuple states of the restatement and the states of fsa_product_ref's conjunction under dfa_ref serve equal
    rows and die together; the ids correspond one to one (the product automaton numbers by search, the tuples by particle).
    The patterns are such that every pair of live states can still be completed together: `product` trims the pairs that cannot,
    which a conjunction of constraints - a bit says that every PART survives the token - does not."""
    a, b = (ByteDFA.from_regex(p) for p in patterns)
    vocab, eos, skip = _vocab(b"ab")
    V = len(vocab)
    p = F.product(a, b, "and")
    auto = J.DfaPart(ByteDFA(p["delta"], p["accepting"], 0), vocab, eos, skip)
    conj = J.Product([J.DfaPart(a, vocab, eos, skip), J.DfaPart(b, vocab, eos, skip)], V, eos)
    sa, sc = np.zeros(200, np.int32), np.zeros(200, np.int32)
    to_auto, to_conj = {0: 0}, {0: 0}
    for tokens, frm, to in _random_calls(V, [200] * 6, 4):
        sa, sc = auto.advance(sa, tokens, frm, to), conj.advance(sc, tokens, frm, to)
        assert np.array_equal(sa < 0, sc < 0)
        for x, y in zip(sc[sc >= 0].tolist(), sa[sa >= 0].tolist()):
            assert to_auto.setdefault(x, y) == y and to_conj.setdefault(y, x) == x  # (a bijection between the states met)
        for x in set(sc[sc >= 0].tolist()):
            assert np.array_equal(conj.row(x), auto.row(to_auto[x])), x
            assert conj.accepts(x) == bool(p["accepting"][to_auto[x]])
        # the pair behind the tuple is the pair behind the automaton's state
        assert all(tuple(p["pairs"][to_auto[x]]) == conj.tuples()[x] for x in set(sc[sc >= 0].tolist()))
        sa, sc = np.where(sa < 0, 0, sa).astype(np.int32), np.where(sc < 0, 0, sc).astype(np.int32)
    assert len(to_auto) > 6 and not conj.overflow


def _three(max_states=65536):
    vocab, eos, skip = _vocab(b"()x")
    V = len(vocab)
    short = ByteDFA.from_regex(rb"[()x]?[()x]?[()x]?[()x]?[()x]?[()x]?")
    evens = ByteDFA.from_regex(rb"([()]*x[()]*x)*[()]*")
    parts = [J.NumberedPart(P.Ref(BytePDA.dyck([(b"(", b")")], b"x"), vocab, eos, skip, max_depth=3)), J.DfaPart(short, vocab, eos, skip),
             J.DfaPart(evens, vocab, eos, skip)]
    return J.Product(parts, V, eos, max_states=max_states), vocab


def test_numbering_order_overflow_cut_and_the_zero_half_word():
    conj, vocab = _three()
    tok = vocab.index
    z = lambda *v: np.array(v, np.int32)
    tokens = z(tok(b"x"), tok(b"("), tok(b")"), tok(b"x"), tok(b"(("), tok(b"("), len(vocab) - 3, len(vocab) - 2).reshape(-1, 1)
    frm, to = np.zeros(8, np.int32), np.ones(8, np.int32)
    got = conj.advance(None, tokens, frm, to)
    # new tuples in the order of the smallest particle that reached them; ) from the empty stack, the empty and the skipped token: dead
    assert got.tolist() == [1, 2, -1, 1, 3, 2, -1, -1] and conj.n_states == 4
    assert conj.tuples()[0] == (0, conj.parts[1].start, conj.parts[2].start) and all(len(t) == 3 and min(t) >= 0 for t in conj.tuples())
    words = conj.words()
    assert words.shape == (4, 2) and words.dtype == np.uint64 and not (words[:, 1] >> np.uint64(32)).any()  # K = 3: the upper half of word 1
    assert [(int(w[0]) & 0xffffffff, int(w[0]) >> 32, int(w[1])) for w in words] == conj.tuples()
    # states from -1 to past the count: all parts -1, so dead; an empty range gives the state back
    again = conj.advance(z(-1, 4, 1 << 30, 1, 3), tokens[:5], z(0, 0, 0, 1, 0), z(1, 1, 1, 1, 0))
    assert again.tolist() == [-1, -1, -1, 1, 3] and conj.n_states == 4
    assert conj.unpack(z(-1, 0, 4), 3).T.tolist() == [[-1, -1, -1], list(conj.tuples()[0]), [-1, -1, -1]]
    # the cut: one id fewer than the call needs - the extra particles are -1, the ids before the cut are the same
    tight, _ = _three(max_states=3)
    cut = tight.advance(None, tokens, frm, to)
    assert cut.tolist() == [1, 2, -1, 1, -1, 2, -1, -1] and tight.overflow and tight.n_states == 3 and tight.tuples() == conj.tuples()[:3]
    exact, _ = _three(max_states=4)
    assert exact.advance(None, tokens, frm, to).tolist() == got.tolist() and not exact.overflow
    # rows: the AND of the parts', the EOS bit the AND of theirs
    for s in range(conj.n_states):
        rows = [p.row(v) for p, v in zip(conj.parts, conj.tuples()[s])]
        assert np.array_equal(conj.row(s), rows[0] & rows[1] & rows[2])
    assert conj.accepts(0) and not conj.accepts(1) and not conj.accepts(2)  # one x: odd; one (: open
    assert np.array_equal(conj.row_eos(), conj.parts[0].ref.row_eos()) and not conj.row_dead().any()


def test_weighted_rows_are_the_ordered_sum_with_minus_infinity_under_cleared_bits():
    from genlm_backend_amd.constraints import ByteWFSA
    from tests import wfsa_ref as WR

    vocab, eos, skip = _vocab(b"ab")
    V = len(vocab)
    da, db, dc = ByteDFA.from_regex(rb"(a|b)*"), ByteDFA.from_regex(rb"(a|b)*b"), ByteDFA.from_regex(rb"a(a|b)*")
    wa, wb = (ByteWFSA(d.delta, *WR.random_weights(d.delta, d.accepting, seed), d.start) for seed, d in ((1, da), (2, db)))
    parts = [J.DfaPart(wa, vocab, eos, skip), J.DfaPart(dc, vocab, eos, skip), J.DfaPart(wb, vocab, eos, skip)]
    conj = J.Product(parts, V, eos)
    assert conj.weighted and conj.row_dead().dtype == np.float32 and conj.row_eos()[eos] == 0.0
    row = conj.row(0)
    ra, rc, rb = (p.row(p.start) for p in parts)
    want = ((np.float32(0.0) + ra).astype(np.float32) + rb).astype(np.float32)
    allowed = J.bits_of(rc, V)
    assert np.array_equal(row[allowed], want[allowed]) and np.isneginf(row[~allowed]).all() and allowed.any() and not allowed.all()
    assert np.isfinite(row).any() and row.dtype == np.float32
    assert conj.final_logw(0) == np.float32(np.float32(np.float32(0.0) + wa.final_logw[wa.start]) + wb.final_logw[wb.start])
