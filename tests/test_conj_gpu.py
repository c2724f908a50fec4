"""Conjunctions of constraints on the GPU (glb_conj_*, constraints.ConstraintProduct): state ids, tuples, raw words and the count
after every `advance` call and every bank row bit for bit against the restatement tests/conj_ref.py - K = 2, 3 and 8 parts (W =
1, 2, 4 words, the zero half word of an odd K), vocabularies of 1, 33, 127 and 257 tokens, 1, 64, 65 and 1000 particles, nearly
every hash colliding, canaries behind every buffer at exactly the rows needed, the overflow cut, weighted rows, banks that
evict, two DFAs against their product automaton, a nested product, and JSON with a pattern under DeviceSIS.  Everything is
exact."""
import json

import numpy as np
import pytest
import torch

from genlm_backend_amd.constraints import (ByteDFA, ByteNFA, BytePDA, ByteWFSA, ConstraintProduct, DeviceConstraint, LazyConstraint,
                                           PDAConstraint, product)
from tests import conj_ref as J
from tests import dfa_ref as R
from tests import lazy_ref as L
from tests import pda_ref as P
from tests import wfsa_ref as WR
from tests.test_pda_cpu import _json_depth
from tests.test_wfsa_gpu import _model

pytestmark = pytest.mark.gpu
_CACHE = {}
CANARY = {torch.uint8: 0x5a, torch.int32: 0x5a5a5a5a, torch.int64: 0x5a5a5a5a5a5a5a5a}
SIS_SEED = 2
HASHES = pytest.mark.parametrize("hash_mask", [0, 0xF], ids=["hash", "hash&0xF"])
DEPTH = 5


def vocabulary(V):
    """(vocab, eos, skip) over ()[]x: V = 1 is the one token ( which is the EOS too; else tokens that push, that pop, that do
    both, seeded strings of 1 .. 4 bytes, an empty token (V - 3), a skipped one (V - 2) and the EOS (V - 1)."""
    if V == 1:
        return [b"("], 0, ()
    fixed = [b"(", b")", b"[", b"]", b"x", b"((", b"))", b"()", b"(x)", b")(", b"][", b"([", b"])", b"xx", b"x(", b")x", b"[]", b"(((((("]
    rng = np.random.default_rng(V)
    letters = np.frombuffer(b"()[]x", np.uint8)
    more = [bytes(rng.choice(letters, int(rng.integers(1, 5)), p=[.25, .25, .15, .15, .2])) for _ in range(V - 3 - len(fixed))]
    vocab = fixed + more + [b"", b"((", b"<eos>"]
    assert len(vocab) == V
    return vocab, V - 1, (V - 2, V - 1)


def automaton(name):
    if name not in _CACHE:
        rx = {"short": rb"[()\[\]x]{0,6}", "evenx": rb"([()\[\]]*x[()\[\]]*x)*[()\[\]]*", "noxx": rb"(x?[()\[\]])*x?", "any": rb"[()\[\]x]*",
              "round": rb"[()x]*", "open": rb"([(\[][()\[\]x]*)?", "three": rb"([()\[\]x]{3})*[()\[\]x]?[()\[\]x]?", "noend": rb"[()\[\]x]*[)\]x]"}
        if name == "dyck":
            _CACHE[name] = BytePDA.dyck([(b"(", b")"), (b"[", b"]")], b"x")
        elif name == "lazy":
            _CACHE[name] = ByteNFA.from_regex(rb"[()\[\]x]*[(\[][()\[\]x][()\[\]x]?")
        elif name.startswith("w:"):
            d = automaton(name[2:])
            _CACHE[name] = ByteWFSA(d.delta, *WR.random_weights(d.delta, d.accepting, len(name)), d.start)
        else:
            _CACHE[name] = ByteDFA.from_regex(rx[name])
    return _CACHE[name]


def make_part(engine, name, voc, hash_mask, **kw):
    """(the constraint on the device, its restatement)"""
    vocab, eos, skip = voc
    a = automaton(name)
    if name == "dyck":
        return (PDAConstraint(engine, a, vocab, eos, skip_ids=skip, max_depth=DEPTH, max_states=4096, _hash_mask=hash_mask, **kw),
                J.NumberedPart(P.Ref(a, vocab, eos, skip, max_depth=DEPTH, max_states=4096)))
    if name == "lazy":
        return (LazyConstraint(engine, a, vocab, eos, skip_ids=skip, max_states=4096, _hash_mask=hash_mask, **kw),
                J.NumberedPart(L.Ref(a, vocab, eos, skip, max_states=4096)))
    return DeviceConstraint(engine, a, vocab, eos, skip_ids=skip, **kw), J.DfaPart(a, vocab, eos, skip)


def ref_parts(names, voc):
    vocab, eos, skip = voc
    out = []
    for name in names:
        a = automaton(name)
        if name == "dyck":
            out.append(J.NumberedPart(P.Ref(a, vocab, eos, skip, max_depth=DEPTH, max_states=4096)))
        elif name == "lazy":
            out.append(J.NumberedPart(L.Ref(a, vocab, eos, skip, max_states=4096)))
        else:
            out.append(J.DfaPart(a, vocab, eos, skip))
    return out


def _canaried(shape, dtype, dev, extra=8):
    """(whole, view): `view` of `shape` at the front of a buffer whose `extra` elements behind it hold the canary."""
    n = int(np.prod(shape))
    whole = torch.full((n + extra,), CANARY[dtype], dtype=dtype, device=dev)
    return whole, whole[:n].view(shape)


class Dev:
    """A ConstraintProduct whose every buffer lies in front of a canary, started over in them, beside its restatement."""

    def __init__(self, engine, names, voc, max_states, n_most, hash_mask=0, bank_rows=None, on_full="error", part_kw=None):
        vocab, eos, skip = voc
        self.V = V = len(vocab)
        made = [make_part(engine, name, voc, hash_mask, **((part_kw or {}).get(name, {}))) for name in names]
        self.weighted = any(p.weighted for _, p in made)
        self.elems = V if self.weighted else (V + 31) // 32
        row_bytes = 4 * ((V + 63) // 64 * 64 if self.weighted else (V + 31) // 32)
        kw = {} if bank_rows is None else dict(mask_bank_bytes=bank_rows * row_bytes)
        c = self.c = ConstraintProduct(engine, [d for d, _ in made], max_states=max_states, on_full=on_full, _hash_mask=hash_mask, **kw)
        self.ref = J.Product([r for _, r in made], V, eos, max_states=max_states)
        dev = self.dev = c.dev
        self.whole = {}
        c._chunk = int(max(1, min(n_most, c._slots - max_states)))
        for name, shape, dtype in (("_tuples", (max_states, c.W), torch.int64), ("_rep", (max_states,), torch.int32),
                                   ("_table", (c._slots * 12 // 8,), torch.int64), ("_row_of_state", (max_states,), torch.int32),
                                   ("_status", (8,), torch.int32), ("_part_states", (c.K, n_most), torch.int32),
                                   ("_claim", (n_most,), torch.int32), ("_counts", (-(-c._chunk // 256),), torch.int32),
                                   ("_counters", (4,), torch.int32), ("_work", (c.capacity, 2), torch.int32)):
            self.whole[name], view = _canaried(shape, dtype, dev)
            setattr(c, name, view)
        rows = c.capacity
        self.big = torch.full((rows + 2, self.elems + 3), CANARY[torch.int32], dtype=torch.int32, device=dev)
        c.bank = self.big[:rows].view(torch.float32) if self.weighted else self.big[:rows]
        if c._evicting:
            self.whole["_evict_tables"], c._evict_tables = _canaried((4 * rows + 5,), torch.int32, dev)
        c._call("glb_conj_init", c._block())

    def canaries_intact(self):
        c = self.c
        for name, whole in self.whole.items():
            if not bool((whole[getattr(c, name).numel():] == CANARY[whole.dtype]).all()):
                return False
        return bool((self.big[c.capacity:] == CANARY[torch.int32]).all()) and bool((self.big[:, self.elems:] == CANARY[torch.int32]).all())

    def up(self, a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.dev)

    def advance(self, states, tokens, frm, to):
        """One call on the device and in the restatement: the ids, the count, the tuples and their raw words are equal."""
        got = self.c.advance(self.up(states), self.up(tokens), self.up(frm), self.up(to)).cpu().numpy()
        want = self.ref.advance(states, tokens, frm, to)
        assert np.array_equal(got, want), (np.nonzero(got != want)[0][:8], got[got != want][:8], want[got != want][:8])
        n = self.ref.n_states
        assert self.c.n_states == n and self.c.tuples() == self.ref.tuples()
        assert np.array_equal(self.c._tuples[:n].cpu().numpy().view(np.uint64), self.ref.words())  # (odd K: the zero half word)
        assert self.canaries_intact()
        return got

    def bank_rows(self):
        return self.big[:self.c.capacity, :self.elems].cpu().numpy().view(np.uint32)

    def same_row(self, got, want):
        return np.array_equal(got, np.ascontiguousarray(want).view(np.uint32))

    def rows(self, states, done=None):
        """`mask_rows`: the row of every distinct state served bit for bit, rows 0 and 1 for the dead and the done."""
        ids = self.c.mask_rows(self.up(states), done=self.up(done)).cpu().numpy()
        bank = self.bank_rows()
        assert self.same_row(bank[0], self.ref.row_dead()) and self.same_row(bank[1], self.ref.row_eos())
        seen = {}
        for i, s in enumerate(states):
            ok = 0 <= s < self.ref.n_states
            if done is not None and done[i]:
                assert ids[i] == (1 if ok and self.ref.accepts(int(s)) else 0), i
            elif not ok:
                assert ids[i] == 0, i
            else:
                assert ids[i] >= 2 and seen.setdefault(int(s), ids[i]) == ids[i], i
        for s, r in seen.items():
            assert self.same_row(bank[r], self.ref.row(s)), (s, self.ref.tuples()[s])
        assert self.canaries_intact()
        return ids, seen


SIZES = (1, 64, 65, 1000, 1000)
PARTS = {2: ("dyck", "short"), 3: ("lazy", "dyck", "evenx"), 8: ("dyck", "short", "evenx", "noxx", "any", "open", "three", "noend")}
CASES = [(2, 33), (2, 257), (3, 127), (3, 1), (8, 257), (8, 33), (2, 1)]


def _calls(ref, V, sizes, seed, ld=4):
    """Random calls over the restatement `ref` as it grows: states from -1 to past the states known, tokens of the whole
    vocabulary, an id past V and -1, ranges inside [0, ld] and a few outside; in the fourth call 700 particles walk one range
    from state 0."""
    rng = np.random.default_rng(seed)
    out = []
    for k, n in enumerate(sizes):
        tokens = rng.integers(0, V, (n, ld)).astype(np.int32)
        singles = np.array([0, 0, 2, 4, 4, 1, 3, 5, 7], np.int32) % V
        tokens = np.where(rng.random((n, ld)) < 0.6, rng.choice(singles, (n, ld)), tokens).astype(np.int32)
        tokens[rng.random((n, ld)) < 0.01] = V
        tokens[rng.random((n, ld)) < 0.01] = -1
        frm = rng.integers(0, 3, n).astype(np.int32)
        to = np.minimum(frm + rng.integers(0, 4, n), ld).astype(np.int32)
        odd = rng.random(n)
        to[odd < 0.03] = ld + 1
        frm[(odd > 0.03) & (odd < 0.06)] = 3
        to[(odd > 0.03) & (odd < 0.06)] = 2
        frm[(odd > 0.06) & (odd < 0.08)] = -1
        if k == 0:
            states = None
        else:
            states = rng.integers(0, ref.n_states, n).astype(np.int32)
            states[rng.random(n) < 0.05] = -1
            states[rng.random(n) < 0.03] = ref.n_states
            states[rng.random(n) < 0.01] = 1 << 30
        if k == 3:  # the claim race: 700 particles, one range, one tuple (new where the script's earlier calls have not met it)
            states[100:800], tokens[100:800], frm[100:800], to[100:800] = 0, np.array([2, 0, 4, 2], np.int32) % V, 0, ld
        out.append((states, tokens, frm, to))
        ref.advance(states, tokens, frm, to)
    return out


def _script(case):
    """The calls of a case, the states they number, the most particles that reach one new state in a call and the most new
    states of a call."""
    if ("script", case) not in _CACHE:
        K, V = case
        voc = vocabulary(V)
        ref = J.Product(ref_parts(PARTS[K], voc), V, voc[1], max_states=1 << 22)
        calls = _calls(ref, V, SIZES, 11 + K + V)
        again = J.Product(ref_parts(PARTS[K], voc), V, voc[1], max_states=1 << 22)
        crowd = most = 0
        for call in calls:
            before = again.n_states
            out = again.advance(*call)
            most = max(most, again.n_states - before)
            fresh = out[out >= before]
            if len(fresh):
                crowd = max(crowd, int(np.bincount(fresh - before).max()))
        _CACHE[("script", case)] = (calls, ref.n_states, crowd, most)
    return _CACHE[("script", case)]


def test_what_the_cases_exercise():
    """From the restatement alone: every K and V, 700 particles that reach one new tuple, more than 64 new tuples in a call."""
    assert {k for k, _ in CASES} == {2, 3, 8} and {v for _, v in CASES} == {1, 33, 127, 257}
    crowds = [_script(case)[2] for case in CASES]
    assert sum(c >= 700 for c in crowds) >= 3
    assert max(_script(case)[3] for case in CASES) > 64  # (one serve call with more work entries than its grid has side by side)


@HASHES
@pytest.mark.parametrize("case", CASES, ids=[f"K{k}-V{v}" for k, v in CASES])
def test_states_tuples_and_rows_call_by_call(engine, case, hash_mask):
    K, V = case
    calls, total, _, _ = _script(case)
    # exactly the states the calls number and the particles of the largest call: one more of either lands in a canary
    dv = Dev(engine, PARTS[K], vocabulary(V), total, max(SIZES), hash_mask)
    assert dv.c.W == (K + 1) // 2 and dv.c.K == K and not dv.c.weighted
    for states, tokens, frm, to in calls:
        got = dv.advance(states, tokens, frm, to)
        done = (np.arange(len(got)) % 7 == 0).astype(np.int32)
        dv.rows(got, done)
        dv.rows(got)
    assert dv.c.n_states == total and not dv.ref.overflow and dv.c.stats()["states"] == total
    dv.c.check()
    engine.check()


@HASHES
def test_degenerate_calls(engine, hash_mask):
    """ld == 0, n == 0, an empty range, a dead state, a state past the count; an id that no tuple has yet."""
    voc = vocabulary(33)
    dv = Dev(engine, PARTS[3], voc, 16, 8, hash_mask)
    tok = voc[0].index
    z = lambda *v: np.array(v, np.int32)
    first = dv.advance(None, z(tok(b"("), tok(b"["), tok(b"x")).reshape(3, 1), z(0, 0, 0), z(1, 1, 1))
    assert first.tolist() == [1, 2, 3]
    none = np.zeros((4, 0), np.int32)
    assert dv.advance(z(0, 1, -1, dv.c.n_states), none, z(0, 0, 0, 0), z(0, 0, 0, 0)).tolist() == [0, 1, -1, -1]
    empty = dv.c.advance(None, torch.zeros((0, 3), dtype=torch.int32, device=dv.dev), torch.zeros(0, dtype=torch.int32, device=dv.dev),
                         torch.zeros(0, dtype=torch.int32, device=dv.dev))
    assert empty.shape == (0,) and dv.c.mask_rows(empty).shape == (0,)
    dv.c.check()
    # an id that no tuple has yet is served row 0 and claims nothing: the tuple that takes the id is served its own row
    k = dv.c.n_states
    ids = dv.c.mask_rows(dv.up(z(k, 0, k))).cpu().numpy()
    assert ids[0] == 0 and ids[2] == 0 and ids[1] >= 2 and dv.canaries_intact()
    assert int(dv.c._row_of_state[k].item()) == -1 and dv.c.stats()["rows_in_use"] == 3
    got = dv.advance(z(1, 2), z(tok(b"("), tok(b"x"), tok(b"x"), tok(b"x")).reshape(2, 2), z(0, 0), z(2, 2))
    assert k in got.tolist()
    dv.rows(got)
    dv.c.check()


@HASHES
def test_overflow_cuts_in_particle_order_and_the_exact_count_passes(engine, hash_mask):
    voc = vocabulary(33)
    rng = np.random.default_rng(5)
    pool = np.array([voc[0].index(t) for t in (b"(", b"[", b"((", b"x", b"()", b")", b"([")], np.int32)
    tokens, frm, to = rng.choice(pool, (1000, 4)).astype(np.int32), np.zeros(1000, np.int32), rng.integers(1, 5, 1000).astype(np.int32)
    need = J.Product(ref_parts(PARTS[2], voc), 33, voc[1])
    need.advance(None, tokens, frm, to)
    n = need.n_states
    assert 40 < n < 600
    tight = Dev(engine, PARTS[2], voc, n - 1, 1000, hash_mask)
    got = tight.advance(None, tokens, frm, to)  # (equal to the restatement's cut: ids, tuples and the count)
    assert tight.ref.overflow and (got == -1).any() and tight.c.n_states == n - 1
    ids, _ = tight.rows(got)
    assert (ids[got < 0] == 0).all()
    with pytest.raises(RuntimeError, match=f"max_states={n - 1}") as e:
        tight.c.check()
    assert "empty mask" in str(e.value)
    again = tight.advance(got, tokens, to, np.minimum(to + 1, 4).astype(np.int32))  # full from the start: nothing is numbered
    assert tight.c.n_states == n - 1 and (again[got < 0] == -1).all()
    exact = Dev(engine, PARTS[2], voc, n, 1000, hash_mask)
    exact.advance(None, tokens, frm, to)
    assert not exact.ref.overflow
    exact.c.check()
    engine.check()


# ---- two DFAs against their product automaton -------------------------------------------------------------------------------------------
@HASHES
def test_two_dfas_against_their_product_automaton(engine, hash_mask):
    """The same language served two ways: rows bit-equal and dead flags equal at every step.  Every pair of live states of the
    two patterns can be completed together, so `product`'s joint trim drops nothing that the conjunction keeps."""
    vocab, eos, skip = R.synth_vocab(300, 300)
    vocab = list(vocab)
    vocab[290:300] = [b"ab", b"ba", b"aab", b"bb", b"abab", b"ab" * 20, b"xa", b"ax", b"xx", b"a" * 5]
    a, b = ByteDFA.from_regex(rb"(a|b)*abb(a|b)*"), ByteDFA.from_regex(rb"(a|b)*a(a|b){3}")
    whole = DeviceConstraint(engine, product(engine, a, b, "and")[0], vocab, eos, skip_ids=skip)
    conj = ConstraintProduct(engine, [DeviceConstraint(engine, a, vocab, eos, skip_ids=skip), DeviceConstraint(engine, b, vocab, eos, skip_ids=skip)],
                             _hash_mask=hash_mask)
    rng = np.random.default_rng(21)
    n, steps = 256, 24
    tokens = rng.choice(np.array([97, 98, 290, 291, 292, 293, 294], np.int32), (n, steps)).astype(np.int32)
    tokens[rng.random((n, steps)) < 0.01] = 48  # (a byte the patterns do not read: the particle dies)
    tok = torch.from_numpy(tokens).to(engine.device)
    sw, sc = whole.states0(n), conj.states0(n)
    for t in range(steps):
        frm, to = (torch.full((n,), v, dtype=torch.int32, device=engine.device) for v in (t, t + 1))
        sw, sc = whole.advance(sw, tok, frm, to), conj.advance(sc, tok, frm, to)
        done = torch.full((n,), int(t == steps - 1), dtype=torch.int32, device=engine.device)
        rw, rc = whole.mask_rows(sw, done=done), conj.mask_rows(sc, done=done)
        assert torch.equal(sw < 0, sc < 0), t
        assert torch.equal(whole.bank[rw.long(), :whole.words], conj.bank[rc.long(), :conj.words]), t
    assert int((sc < 0).sum()) > 0 and int((sc >= 0).sum()) > 100 and 8 < conj.n_states <= whole.dfa.n_states
    assert int((rc == 1).sum()) > 0 and int((rc == 0).sum()) > 0
    whole.check()
    conj.check()
    engine.check()


# ---- a nested product ---------------------------------------------------------------------------------------------------------------
@HASHES
def test_a_nested_product_serves_the_rows_of_the_flat_one(engine, hash_mask):
    voc = vocabulary(127)
    V = 127
    flat = ConstraintProduct(engine, [make_part(engine, name, voc, hash_mask)[0] for name in PARTS[3]], _hash_mask=hash_mask)
    a, b, c = (make_part(engine, name, voc, hash_mask)[0] for name in PARTS[3])
    nested = ConstraintProduct(engine, [ConstraintProduct(engine, [a, b], _hash_mask=hash_mask), c], _hash_mask=hash_mask)
    rng = np.random.default_rng(3)
    n, steps = 200, 8
    tokens = rng.choice(np.array([0, 2, 4, 1, 3, 7, 11], np.int32), (n, steps)).astype(np.int32)
    tok = torch.from_numpy(tokens).to(engine.device)
    sf, sn = flat.states0(n), nested.states0(n)
    for t in range(steps):
        frm, to = (torch.full((n,), v, dtype=torch.int32, device=engine.device) for v in (t, t + 1))
        sf, sn = flat.advance(sf, tok, frm, to), nested.advance(sn, tok, frm, to)
        done = torch.from_numpy((np.arange(n) % 5 == 0).astype(np.int32)).to(engine.device)
        rf, rn = flat.mask_rows(sf, done=done), nested.mask_rows(sn, done=done)
        assert torch.equal(sf, sn), t  # (the same tuples in the same particle order: the same ids)
        assert torch.equal(flat.bank[rf.long(), :flat.words], nested.bank[rn.long(), :nested.words]), t
        sf, sn = (torch.where(s < 0, torch.zeros_like(s), s) for s in (sf, sn))
    assert 20 < flat.n_states == nested.n_states
    assert [(x, y, z) for (x, y), z in ((nested.parts[0].tuples()[p], z) for p, z in nested.tuples())] == flat.tuples()
    flat.check()
    nested.check()
    engine.check()


# ---- weighted ------------------------------------------------------------------------------------------------------------------------
@HASHES
@pytest.mark.parametrize("names,V", [(("dyck", "w:short"), 257), (("w:any", "w:noxx", "short"), 33), (("w:evenx", "dyck"), 1)],
                         ids=["pda-wfsa-V257", "wfsa-wfsa-dfa-V33", "wfsa-pda-V1"])
def test_weighted_rows_are_the_ordered_float32_sum(engine, names, V, hash_mask):
    voc = vocabulary(V)
    ref = J.Product(ref_parts(names, voc), V, voc[1], max_states=1 << 22)
    calls = _calls(ref, V, (1, 64, 65, 300), 5 + V)
    dv = Dev(engine, names, voc, ref.n_states, 300, hash_mask)
    assert dv.c.weighted and dv.c.bank.dtype == torch.float32 and dv.c.start_logw == 0.0
    finite = 0
    for states, tokens, frm, to in calls:
        got = dv.advance(states, tokens, frm, to)
        done = (np.arange(len(got)) % 3 == 0).astype(np.int32)
        ids, seen = dv.rows(got, done)
        finite += sum(int(np.isfinite(dv.ref.row(s)).sum()) for s in seen)
        forced = torch.from_numpy((ids == 1) & (done > 0)).to(dv.dev)
        fw = dv.c.forced_final_logw(dv.up(got), forced).cpu().numpy()
        want = np.array([dv.ref.final_logw(int(s)) if f else 0.0 for s, f in zip(got, forced.cpu().numpy())], np.float32)
        assert fw.tobytes() == want.tobytes()
    assert finite > 0
    dv.c.check()
    engine.check()


def test_start_logw_is_the_sum_of_the_parts(engine):
    voc = vocabulary(33)
    vocab, eos, skip = voc
    wa, wb = automaton("w:any"), automaton("w:noxx")
    a = DeviceConstraint(engine, wa, vocab, eos, skip_ids=skip, push="log")
    b = DeviceConstraint(engine, wb, vocab, eos, skip_ids=skip, push="max")
    c = make_part(engine, "short", voc, 0)[0]
    conj = ConstraintProduct(engine, [a, c, b])
    assert conj.weighted and a.start_logw != 0.0 and b.start_logw != 0.0
    assert conj.start_logw == float(sum([a.start_logw, c.start_logw, b.start_logw]))


# ---- eviction --------------------------------------------------------------------------------------------------------------------------
def _walk_until(dv, voc, n_states, particles=3):
    rng = np.random.default_rng(9)
    pool = np.array([voc[0].index(t) for t in (b"(", b"[", b"x", b")", b"]")], np.int32)
    states = np.zeros(particles, np.int32)
    for _ in range(200):
        tokens = rng.choice(pool, (particles, 1)).astype(np.int32)
        nxt = dv.advance(states, tokens, np.zeros(particles, np.int32), np.ones(particles, np.int32))
        states = np.where(nxt >= 0, nxt, 0).astype(np.int32)  # (a dead particle starts over)
        ids, _ = dv.rows(states)
        assert (ids >= 2).all()
        if dv.c.n_states >= n_states:
            break
    assert dv.c.n_states >= n_states


@HASHES
def test_a_product_bank_of_five_rows_evicts_and_serves_right_rows(engine, hash_mask):
    voc = vocabulary(33)
    dv = Dev(engine, ("dyck", "evenx"), voc, 64, 8, hash_mask, bank_rows=5, on_full="evict")
    assert dv.c._evicting and dv.c.capacity == 5
    _walk_until(dv, voc, 40)
    st = dv.c.stats()
    assert st["evictions"] > 0 and st["rows_in_use"] == 5 and st["states"] == dv.c.n_states
    dv.c.check()
    ids = dv.c.mask_rows(dv.up(np.array([0, 1, 2, 3], np.int32))).cpu().numpy()  # four distinct states in one call: one is left without a row
    bank = dv.bank_rows()
    assert (ids == 0).sum() == 1 and all(dv.same_row(bank[r], dv.ref.row(s)) for s, r in enumerate(ids) if r) and dv.canaries_intact()
    with pytest.raises(RuntimeError, match="smaller than one step's working set"):
        dv.c.check()


@HASHES
def test_a_part_that_evicts_inside_a_product(engine, hash_mask):
    """The PDA part's bank holds one step's working set (three particles: three rows and the bank's two) and evicts; the
    product's own bank holds everything: its rows, combined when the part's rows were there, stay right."""
    voc = vocabulary(33)
    words = (33 + 31) // 32
    dv = Dev(engine, ("dyck", "evenx"), voc, 64, 8, hash_mask, part_kw={"dyck": dict(mask_bank_bytes=5 * words * 4, on_full="evict")})
    part = dv.c.parts[0]
    assert part._evicting and part.capacity == 5 and not dv.c._evicting
    _walk_until(dv, voc, 40)
    assert part.stats()["evictions"] > 0 and dv.c.stats()["evictions"] == 0
    dv.c.check()


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
@HASHES
def test_json_with_a_pattern_is_served_under_sis(engine, hash_mask):
    """`BytePDA.json()` at max_depth = 4 together with "only the bytes []0-9, and the space" under a DeviceSIS of 64 particles for 48
    steps: a text has finite weight exactly when `json.loads` takes it, it nests at most 4 deep and it matches the pattern.
    SIS_SEED is one under which a finite-weight text holds a bracket: the model's logits are made on the device, so it was
    picked from a scan of seeds there."""
    import re

    from genlm_backend_amd.sis import DeviceSIS

    vocab, eos, skip = R.synth_vocab(300, 300)
    vocab = list(vocab)
    vocab[290:300] = [b"[[", b"]]", b"[1", b", ", b"],", b"[]", b"12", b"0]", b" [", b"null"]
    m = _model(engine, 300)
    pattern = rb"[\[\]0-9, ]*"
    grammar = PDAConstraint(m, BytePDA.json(), vocab, eos, skip_ids=skip, max_depth=4, _hash_mask=hash_mask)
    only = DeviceConstraint(m, ByteDFA.from_regex(pattern), vocab, eos, skip_ids=skip)
    c = ConstraintProduct(m, [grammar, only], _hash_mask=hash_mask)
    sis = DeviceSIS(m, 64, [5, 17, 99], 48, eos, seed=SIS_SEED, constraint=c)
    sis.run()
    c.check()
    assert 1 < c.n_states < 64 * 48 + 1
    ctx, lw = sis.results()
    assert int(sis.active.sum().item()) == 0
    finite = bracket = 0
    for cx, w in zip(ctx, lw):
        text = b"".join(vocab[t] for t in cx if t != eos)
        depth = _json_depth(text)
        good = depth is not None and depth <= 4 and re.fullmatch(pattern, text) is not None
        if np.isfinite(w):
            assert good, text
            json.loads(text.decode())
            finite += 1
            bracket += b"[" in text
        else:
            assert not good, text
    assert finite > 0 and bracket > 0
    engine.check()
