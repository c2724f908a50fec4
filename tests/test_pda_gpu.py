"""Pushdown constraints on the GPU (glb_pda_*, constraints.PDAConstraint): state ids, configurations, accepting bits and the
count, array for array after every `advance` call, and every bank row bit for bit, against the restatement tests/pda_ref.py - at
the byte-to-word boundaries of a stack and the full wave, with one, two and 126 stack symbols, vocabularies of 1, 33 and 257
tokens, nearly every hash colliding, canaries behind every buffer at exactly the rows needed, the overflow cut, a bank that
evicts, the existing device path over the same regular language, and JSON served under DeviceSIS.  Everything is exact."""
import itertools

import numpy as np
import pytest
import torch

from genlm_backend_amd.constraints import BytePDA, PDAConstraint  # (at import: no test of this file passes without the classes)
from genlm_backend_amd.constraints.pda import POP
from tests import dfa_ref as R
from tests import pda_ref as P
from tests.test_pda_cpu import _json_depth
from tests.test_wfsa_gpu import _model

pytestmark = pytest.mark.gpu
_CACHE = {}
CANARY = {torch.uint8: 0x5a, torch.int32: 0x5a5a5a5a, torch.int64: 0x5a5a5a5a5a5a5a5a}
SIS_SEED = 11


def nest(G):
    """Two states over ()[]{}x": state 0 reads brackets - ( ) symbol 1; with G >= 2 [ ] symbol 2 (G = 126: symbol 64); with G
    = 126 { } symbol 126 - and keeps on x; a quote leads to state 1, which keeps on everything and goes back on a quote.
    State 0 accepts."""
    if ("nest", G) not in _CACHE:
        e = lambda nxt, op=0: nxt | op << 24
        pairs = {1: [(b"()", 1)], 2: [(b"()", 1), (b"[]", 2)], 126: [(b"()", 1), (b"[]", 64), (b"{}", 126)]}[G]
        d = np.full((2, G + 1, 256), -1, np.int32)
        for (o, c), g in pairs:
            d[0, :, o], d[0, g, c] = e(0, g), e(0, POP)
        d[0, :, ord("x")], d[0, :, ord('"')], d[1, :, ord('"')] = e(0), e(1), e(0)
        d[1, :, list(b"()[]{}x")] = e(1)
        _CACHE[("nest", G)] = BytePDA(d, np.array([True, False]), 0)
    return _CACHE[("nest", G)]


def vocabulary(V, depth):
    """(vocab, eos, skip) over ()[]{}x": V = 1 is the one token ( which is the EOS too; else a token that only pushes, one that
    only pops, one that pushes then pops inside itself, one that pops two below where it began and pushes three, one of
    `depth` + 1 pushes (dead), one of `depth` pushes (alive from the empty stack only), tokens of quotes, an empty token (V -
    3), a skipped one (V - 2) and the EOS (V - 1); the rest are seeded strings of 1 .. 6 bytes."""
    if V == 1:
        return [b"("], 0, ()
    fixed = [b"(", b")", b"[", b"]", b"{", b"}", b"x", b'"', b"((", b"))", b"()", b"(x)", b"))(((", b"))[[(", b"]]]]", b"[[", b"{[(", b")]}", b'"(("',
             b'x"', b"(" * (depth + 1), b"(" * depth, b"[" * depth, b"(()", b"[]]", b"{}}", b"([{"]
    rng = np.random.default_rng(V)
    letters = np.frombuffer(b'()[]{}x"', np.uint8)
    more = [bytes(rng.choice(letters, int(rng.integers(1, 7)), p=[.2, .2, .15, .15, .08, .08, .09, .05])) for _ in range(V - 3 - len(fixed))]
    vocab = fixed + more + [b"", b"((", b"<eos>"]
    assert len(vocab) == V
    return vocab, V - 1, (V - 2, V - 1)


# (max_depth, G, V): every depth with its W, every G, every V
CASES = [(1, 1, 33), (7, 2, 257), (8, 126, 33), (9, 1, 257), (16, 2, 33), (17, 126, 257), (504, 2, 257), (9, 2, 1)]
WORDS = {1: 2, 7: 2, 8: 2, 9: 3, 16: 3, 17: 4, 504: 64}
SIZES = (1, 64, 65, 1000, 1000)


def _canaried(shape, dtype, dev, extra=8):
    """(whole, view): `view` of `shape` at the front of a buffer whose `extra` elements behind it hold the canary."""
    n = int(np.prod(shape))
    whole = torch.full((n + extra,), CANARY[dtype], dtype=dtype, device=dev)
    return whole, whole[:n].view(shape)


class Dev:
    """A PDAConstraint whose every buffer lies in front of a canary, started over in them, beside its restatement."""

    def __init__(self, engine, pda, voc, max_depth, max_states, cand_rows, hash_mask=0, bank_rows=None, on_full="error"):
        vocab, eos, skip = voc
        words = (len(vocab) + 31) // 32
        kw = {} if bank_rows is None else dict(mask_bank_bytes=bank_rows * words * 4)
        c = self.c = PDAConstraint(engine, pda, vocab, eos, skip_ids=skip, max_depth=max_depth, max_states=max_states, on_full=on_full,
                                   _hash_mask=hash_mask, **kw)
        self.ref = P.Ref(pda, vocab, eos, skip, max_depth=max_depth, max_states=max_states)
        dev, self.dev, self.words = c.dev, c.dev, words
        self.whole = {}
        cand_rows = int(max(1, min(cand_rows, c._slots - max_states)))
        for name, shape, dtype in (("_configs", (max_states, c.W), torch.int64), ("_accepting", (max_states,), torch.uint8),
                                   ("_table", (c._slots * 12 // 8,), torch.int64), ("_row_of_state", (max_states,), torch.int32),
                                   ("_status", (8,), torch.int32), ("_cand", (cand_rows, c.W), torch.int64),
                                   ("_counts", (-(-cand_rows // 256),), torch.int32), ("_counters", (4,), torch.int32),
                                   ("_work", (c.capacity, 2), torch.int32)):
            self.whole[name], view = _canaried(shape, dtype, dev)
            setattr(c, name, view)
        rows = c.capacity
        self.big = torch.full((rows + 2, words + 3), CANARY[torch.int32], dtype=torch.int32, device=dev)
        c.bank = self.big[:rows]
        if c._evicting:
            self.whole["_evict_tables"], c._evict_tables = _canaried((4 * rows + 5,), torch.int32, dev)
        c._call("glb_pda_init", c._block())
        self._rows = {}

    def canaries_intact(self):
        c = self.c
        for name, whole in self.whole.items():
            if not bool((whole[getattr(c, name).numel():] == CANARY[whole.dtype]).all()):
                return False
        return bool((self.big[c.capacity:] == CANARY[torch.int32]).all()) and bool((self.big[:, self.words:] == CANARY[torch.int32]).all())

    def up(self, a):
        return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.dev)

    def advance(self, states, tokens, frm, to):
        """One call on the device and in the restatement: the ids, the count, the configurations and the accepting bits are
        equal."""
        got = self.c.advance(self.up(states), self.up(tokens), self.up(frm), self.up(to)).cpu().numpy()
        want = self.ref.advance(states, tokens, frm, to)
        assert np.array_equal(got, want), (np.nonzero(got != want)[0][:8], got[got != want][:8], want[got != want][:8])
        assert self.c.n_states == self.ref.n_states
        assert self.c.configs() == self.ref.configs()
        n = self.ref.n_states
        assert np.array_equal(self.c._configs[:n].cpu().numpy().view(np.uint64), self.ref.words())  # (zero above every depth)
        assert np.array_equal(self.c._accepting[:n].cpu().numpy().astype(np.bool_), self.ref.accepting())
        assert self.canaries_intact()
        return got

    def want_row(self, s):
        if s not in self._rows:
            self._rows[s] = self.ref.mask(s)
        return self._rows[s]

    def rows(self, states, done=None):
        """`mask_rows`: the row of every distinct state served bit for bit, rows 0 and 1 for the dead and the done."""
        ids = self.c.mask_rows(self.up(states), done=self.up(done)).cpu().numpy()
        bank = self.c.bank[:, :self.words].cpu().numpy().view(np.uint32)
        acc = self.ref.accepting()
        assert np.array_equal(bank[0], self.ref.row_dead()) and np.array_equal(bank[1], self.ref.row_eos())
        seen = {}
        for i, s in enumerate(states):
            ok = 0 <= s < self.ref.n_states
            if done is not None and done[i]:
                assert ids[i] == (1 if ok and acc[s] else 0), i
            elif not ok and s < 0:
                assert ids[i] == 0, i
            elif ok:
                assert ids[i] >= 2 and seen.setdefault(int(s), ids[i]) == ids[i], i
        for s, r in seen.items():
            assert np.array_equal(bank[r], self.want_row(s)), (s, self.ref.configs()[s])
        assert self.canaries_intact()
        return ids, seen


def _calls(ref, sizes, seed, ld=5):
    """Random calls over the restatement `ref` as it grows: states from -1 to one past the states known, tokens of the whole
    vocabulary, an id past V and -1, ranges inside [0, ld] and a few outside; (states, tokens, frm, to) per call."""
    rng = np.random.default_rng(seed)
    V = ref.V
    out = []
    for k, n in enumerate(sizes):
        tokens = rng.integers(0, V, (n, ld)).astype(np.int32)
        singles = np.array([0, 0, 2, 2, 4, 6, 7, 1, 3, 5], np.int32) % V  # (the single bytes, the openers twice)
        tokens = np.where(rng.random((n, ld)) < 0.6, rng.choice(singles, (n, ld)), tokens).astype(np.int32)
        tokens[rng.random((n, ld)) < 0.01] = V
        tokens[rng.random((n, ld)) < 0.01] = -1
        frm = rng.integers(0, 3, n).astype(np.int32)
        to = np.minimum(frm + rng.integers(0, 5, n), ld).astype(np.int32)
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
        if k == 3:  # the claim race: 700 particles walk one range to one configuration that no call has met (where there is one left)
            for seq in itertools.product(range(min(V, 8)), repeat=ld):
                config = ref.order[0]
                for t in seq:
                    config = ref.token(config, t) if config is not None else None
                if config is not None and config not in ref.ids:
                    states[100:800], tokens[100:800], frm[100:800], to[100:800] = 0, np.array(seq, np.int32), 0, ld
                    break
        out.append((states, tokens, frm, to))
        ref.advance(states, tokens, frm, to)
    return out


def _script(case):
    """The calls of a case, the states they number, the most a call numbers and the most particles that reach one new state."""
    if ("script", case) not in _CACHE:
        depth, G, V = case
        voc = vocabulary(V, depth)
        ref = P.Ref(nest(G), *voc, max_depth=depth, max_states=1 << 22)
        calls = _calls(ref, SIZES, 7 + depth + G)
        again = P.Ref(nest(G), *voc, max_depth=depth, max_states=1 << 22)
        most = crowd = 0
        for states, tokens, frm, to in calls:
            before = again.n_states
            out = again.advance(states, tokens, frm, to)
            most = max(most, again.n_states - before)
            fresh = out[out >= before]
            if len(fresh):
                crowd = max(crowd, int(np.bincount(fresh - before).max()))
        _CACHE[("script", case)] = (calls, ref.n_states, most, crowd)
    return _CACHE[("script", case)]


def test_what_the_cases_exercise():
    """From the restatement alone: every W and G, a call that numbers more than 64 new states, 700 particles that reach one new
    state, a token that pops below where it began and pushes again, the depth bound, every kind of particle."""
    assert sorted({d for d, _, _ in CASES}) == sorted(WORDS) and {g for _, g, _ in CASES} == {1, 2, 126} and {v for _, _, v in CASES} == {1, 33, 257}
    big = 0
    for case in CASES:
        depth, G, V = case
        calls, total, most, crowd = _script(case)
        big += most > 64 and crowd >= 700
        if V == 1:
            continue
        vocab, eos, skip = vocabulary(V, depth)
        ref = P.Ref(nest(G), vocab, eos, skip, max_depth=depth)
        at = lambda stack: (0, bytes(stack))
        tok = vocab.index
        assert ref.token(at([]), tok(b"(" * depth)) == at([1] * depth) and ref.token(at([1]), tok(b"(" * depth)) is None
        assert ref.token(at([]), tok(b"(" * (depth + 1))) is None and ref.token(at([]), tok(b"()")) == at([])
        assert ref.token(at([]), V - 3) is None and ref.token(at([]), V - 2) is None and vocab[V - 2] == b"(("  # empty, skipped
        if depth >= 7:
            assert ref.token(at([1, 1, 1, 1]), tok(b"))(((")) == at([1, 1, 1, 1, 1]) and ref.token(at([1]), tok(b"))(((")) is None
        for states, tokens, frm, to in calls:
            if len(frm) == 1000:
                assert (frm == to).any() and (frm > to).any() and (to > tokens.shape[1]).any() and (tokens >= V).any() and (tokens < 0).any()
        final = P.Ref(nest(G), vocab, eos, skip, max_depth=depth)
        for call in calls:
            final.advance(*call)
        assert max(len(s) for _, s in final.configs()) == min(depth, 8) or depth > 9 or G == 1  # the bound is reached
        if depth == 504:  # the full wave: a stack in the last lane's word
            assert final.token(at([]), tok(b"[" * depth)) == at([2] * depth)
    assert big >= 2


# ---- ids, configurations, accepting bits and rows, call by call ---------------------------------------------------------------------------
@pytest.mark.parametrize("hash_mask", [0, 0xF], ids=["hash", "hash&0xF"])
@pytest.mark.parametrize("case", CASES, ids=[f"depth{d}-G{g}-V{v}" for d, g, v in CASES])
def test_states_configs_and_rows_call_by_call(engine, case, hash_mask):
    depth, G, V = case
    calls, total, most, _ = _script(case)
    # exactly the states the calls number and the particles of the largest call: one more of either lands in a canary
    dv = Dev(engine, nest(G), vocabulary(V, depth), depth, total, max(SIZES), hash_mask)
    assert dv.c.W == WORDS[depth] and dv.c.max_token_bytes == max(len(t) for t in dv.ref.vocab)
    served = 0
    for states, tokens, frm, to in calls:
        before = dv.ref.n_states
        got = dv.advance(states, tokens, frm, to)
        done = (np.arange(len(got)) % 7 == 0).astype(np.int32)
        ids, seen = dv.rows(got, done)
        served = max(served, sum(s >= before for s in seen))
    assert dv.c.n_states == total and not dv.ref.overflow
    assert served > 64 or most <= 64  # one fill served more work entries than its grid has side by side
    dv.c.check()
    engine.check()


@pytest.mark.parametrize("hash_mask", [0, 0xF], ids=["hash", "hash&0xF"])
def test_the_deepest_stack_is_numbered_and_served(engine, hash_mask):
    """504 symbols: the last byte of the last lane's word; from it only pops and keeps are allowed."""
    depth = 504
    voc = vocabulary(33, depth)
    dv = Dev(engine, nest(2), voc, depth, 4, 8, hash_mask)
    tok = voc[0].index
    z = lambda *v: np.array(v, np.int32)
    got = dv.advance(None, z(tok(b"[" * depth), tok(b"(" * depth), tok(b"(" * (depth + 1))).reshape(3, 1), z(0, 0, 0), z(1, 1, 1))
    assert got.tolist() == [1, 2, -1] and dv.c.configs()[1] == (0, b"\x02" * depth)
    _, seen = dv.rows(z(0, 1, 2))
    allowed = dv.ref.allowed(1)
    assert allowed[tok(b"]")] and allowed[tok(b"]]]]")] and allowed[tok(b"x")] and allowed[tok(b'"')]
    assert not allowed[tok(b"(")] and not allowed[tok(b")")] and not allowed[tok(b"[]]")] and not allowed[tok(b"[")]
    back = dv.advance(z(1, 1), z(tok(b"]]]]"), tok(b"]"), tok(b"]"), tok(b"[")).reshape(2, 2), z(0, 0), z(2, 2))
    assert back.tolist() == [3, 1] and dv.c.configs()[3] == (0, b"\x02" * (depth - 5))  # popped five; popped one and pushed it again
    dv.rows(back)
    dv.c.check()


@pytest.mark.parametrize("hash_mask", [0, 0xF], ids=["hash", "hash&0xF"])
def test_degenerate_calls(engine, hash_mask):
    """ld == 0, n == 0, an empty range on a state, a dead state, a state past the count; an id that no configuration has."""
    voc = vocabulary(33, 9)
    dv = Dev(engine, nest(2), voc, 9, 16, 8, hash_mask)
    tok = voc[0].index
    z = lambda *v: np.array(v, np.int32)
    first = dv.advance(None, z(tok(b"("), tok(b"["), tok(b'"')).reshape(3, 1), z(0, 0, 0), z(1, 1, 1))
    assert first.tolist() == [1, 2, 3]
    none = np.zeros((4, 0), np.int32)
    assert dv.advance(z(0, 1, -1, dv.c.n_states), none, z(0, 0, 0, 0), z(0, 0, 0, 0)).tolist() == [0, 1, -1, -1]
    assert dv.advance(z(0, 1, 0, 0), none, z(0, 0, 0, 1), z(0, 1, 1, 1)).tolist() == [0, -1, -1, -1]  # to > ld == 0
    empty = dv.c.advance(None, torch.zeros((0, 3), dtype=torch.int32, device=dv.dev), torch.zeros(0, dtype=torch.int32, device=dv.dev),
                         torch.zeros(0, dtype=torch.int32, device=dv.dev))
    assert empty.shape == (0,) and dv.c.mask_rows(empty).shape == (0,)
    two = z(tok(b"("), tok(b")")).reshape(1, 2).repeat(5, axis=0)
    got = dv.advance(z(1, 1, -1, 1, 0), two, z(1, 2, 0, 0, 2), z(1, 1, 1, 3, 2))
    assert got.tolist() == [1, -1, -1, -1, 0]
    assert dv.advance(z(1, 0), two[:2], z(1, 1), z(2, 2)).tolist() == [0, -1]  # a pop to the empty stack; a pop from it
    dv.c.check()
    # an id that no configuration has yet is served row 0 and keeps no row: the one that takes the id is served its own row
    k = dv.c.n_states
    ids = dv.c.mask_rows(dv.up(z(k, 0, k))).cpu().numpy()
    assert ids[0] == 0 and ids[2] == 0 and ids[1] >= 2 and dv.canaries_intact()
    got = dv.advance(z(1, 2), z(tok(b"("), tok(b"["), tok(b"x"), tok(b"x")).reshape(2, 2), z(0, 0), z(2, 2))
    assert k in got.tolist()
    dv.rows(got)
    assert dv.c.stats()["states"] == dv.c.n_states
    dv.c.check()


def _overflow_tokens(V, depth):
    vocab, eos, skip = vocabulary(V, depth)
    rng = np.random.default_rng(5)
    pool = np.array([vocab.index(t) for t in (b"(", b"[", b"((", b"[[", b"x", b'"', b"()", b")")], np.int32)
    return rng.choice(pool, (1000, 4)).astype(np.int32), np.zeros(1000, np.int32), rng.integers(1, 5, 1000).astype(np.int32)


@pytest.mark.parametrize("hash_mask", [0, 0xF], ids=["hash", "hash&0xF"])
def test_overflow_cuts_in_particle_order_and_the_exact_count_passes(engine, hash_mask):
    voc = vocabulary(33, 9)
    tokens, frm, to = _overflow_tokens(33, 9)
    need = P.Ref(nest(2), *voc, max_depth=9)
    need.advance(None, tokens, frm, to)
    n = need.n_states
    assert 40 < n < 400
    tight = Dev(engine, nest(2), voc, 9, n - 1, 1000, hash_mask)
    got = tight.advance(None, tokens, frm, to)  # (equal to the restatement's cut: ids, configurations and the count)
    assert tight.ref.overflow and (got == -1).any() and tight.c.n_states == n - 1
    ids, _ = tight.rows(got)
    assert (ids[got < 0] == 0).all()
    with pytest.raises(RuntimeError, match=f"max_states={n - 1}") as e:
        tight.c.check()
    assert "empty mask" in str(e.value)
    again = tight.advance(got, tokens, to, np.minimum(to + 1, 4).astype(np.int32))  # full from the start: nothing is numbered
    assert tight.c.n_states == n - 1 and (again[got < 0] == -1).all()
    exact = Dev(engine, nest(2), voc, 9, n, 1000, hash_mask)
    exact.advance(None, tokens, frm, to)
    assert not exact.ref.overflow
    exact.c.check()
    engine.check()


@pytest.mark.parametrize("hash_mask", [0, 0xF], ids=["hash", "hash&0xF"])
def test_a_bank_of_five_rows_evicts_and_serves_right_rows(engine, hash_mask):
    voc = vocabulary(33, 9)
    dv = Dev(engine, nest(2), voc, 9, 64, 8, hash_mask, bank_rows=5, on_full="evict")
    assert dv.c._evicting and dv.c.capacity == 5
    rng = np.random.default_rng(9)
    pool = np.array([voc[0].index(t) for t in (b"(", b"[", b"x", b'"')], np.int32)
    states = np.zeros(3, np.int32)
    for step in range(80):
        tokens = rng.choice(pool, (3, 1)).astype(np.int32)
        nxt = dv.advance(states, tokens, np.zeros(3, np.int32), np.ones(3, np.int32))
        states = np.where(nxt >= 0, nxt, 0).astype(np.int32)  # (a particle at the depth bound starts over)
        ids, seen = dv.rows(states)
        assert (ids >= 2).all()
        if dv.c.n_states >= 40:
            break
    assert dv.c.n_states >= 40
    st = dv.c.stats()
    assert st["evictions"] > 0 and st["rows_in_use"] == 5 and st["states"] == dv.c.n_states
    dv.c.check()
    k = dv.c.n_states  # an id that no configuration has yet: row 0, and its claim taken back
    assert dv.c.mask_rows(dv.up(np.array([k, 0], np.int32))).cpu().numpy()[0] == 0 and int(dv.c._row_of_state[k].item()) == -1
    dv.c.check()
    ids = dv.c.mask_rows(dv.up(np.array([0, 1, 2, 3], np.int32))).cpu().numpy()  # four distinct states in one call: one is left without a row
    bank = dv.c.bank[:, :dv.words].cpu().numpy().view(np.uint32)
    assert (ids == 0).sum() == 1 and all(np.array_equal(bank[r], dv.want_row(s)) for s, r in enumerate(ids) if r) and dv.canaries_intact()
    with pytest.raises(RuntimeError, match="smaller than one step's working set"):
        dv.c.check()


def _byte_vocab():
    """About 300 tokens: the 256 single bytes, an empty token (256), a skipped one (257), the EOS (258), tokens of up to 70
    bytes, and in the last ten places tokens that the automata here can read."""
    if "bytes" not in _CACHE:
        vocab, eos, skip = R.synth_vocab(300, 300)
        _CACHE["bytes"] = (list(vocab), eos, skip)
    return _CACHE["bytes"]


@pytest.mark.parametrize("hash_mask", [0, 0xF], ids=["hash", "hash&0xF"])
def test_from_dfa_against_device_constraint(engine, hash_mask):
    """The new path crossed with an existing device path: the same regular language, mask rows as bit vectors and dead flags
    equal at every step."""
    from genlm_backend_amd.constraints import ByteDFA, DeviceConstraint

    vocab, eos, skip = _byte_vocab()
    vocab = list(vocab)
    vocab[290:300] = [b"ab", b"ba", b"aab", b"bb", b"abab", b"ab" * 20, b"xa", b"ax", b"xx", b"a" * 5]
    d = ByteDFA.from_regex(rb"(a|b)*a(a|b){9}")
    assert d.live.all()
    eager = DeviceConstraint(engine, d, vocab, eos, skip_ids=skip)
    pda = PDAConstraint(engine, BytePDA.from_dfa(d), vocab, eos, skip_ids=skip, max_depth=1, max_states=8192, _hash_mask=hash_mask)
    rng = np.random.default_rng(21)
    n, steps = 256, 24
    tokens = rng.choice(np.array([97, 98, 290, 291, 292, 293, 294], np.int32), (n, steps)).astype(np.int32)
    tokens[rng.random((n, steps)) < 0.01] = 48  # (a byte the pattern does not read: the particle dies)
    tok = torch.from_numpy(tokens).to(engine.device)
    se, sp = eager.states0(n), pda.states0(n)
    for t in range(steps):
        frm, to = (torch.full((n,), v, dtype=torch.int32, device=engine.device) for v in (t, t + 1))
        se, sp = eager.advance(se, tok, frm, to), pda.advance(sp, tok, frm, to)
        done = torch.full((n,), int(t == steps - 1), dtype=torch.int32, device=engine.device)
        re, rp = eager.mask_rows(se, done=done), pda.mask_rows(sp, done=done)
        assert torch.equal(se < 0, sp < 0), t
        assert torch.equal(eager.bank[re.long(), :eager.words], pda.bank[rp.long(), :pda.words]), t
    assert int((sp < 0).sum()) > 0 and int((sp >= 0).sum()) > 100 and 200 < pda.n_states <= 1024
    alive = sp >= 0
    assert torch.equal(torch.tensor([pda.configs()[s][0] for s in sp[alive].tolist()], dtype=torch.int32), se[alive].cpu())
    eager.check()
    pda.check()
    engine.check()


@pytest.mark.parametrize("hash_mask", [0, 0xF], ids=["hash", "hash&0xF"])
def test_json_is_served_under_sis(engine, hash_mask):
    """`BytePDA.json()` at max_depth = 4 under a DeviceSIS of 64 particles for 48 steps: a text has finite weight exactly when
    `json.loads` takes it and it nests at most 4 deep.  SIS_SEED is one under which a finite-weight text is an array or an
    object: the model's logits are made on the device, so it was picked from a scan of seeds there."""
    from genlm_backend_amd.sis import DeviceSIS

    vocab, eos, skip = _byte_vocab()
    vocab = list(vocab)
    vocab[290:300] = [b'{"', b'":', b"[[", b"]]", b"},", b"[1", b", ", b'"}', b"null", b"true"]
    m = _model(engine, 300)
    c = PDAConstraint(m, BytePDA.json(), vocab, eos, skip_ids=skip, max_depth=4, _hash_mask=hash_mask)
    assert c.W == 2 and not c._evicting
    sis = DeviceSIS(m, 64, [5, 17, 99], 48, eos, seed=SIS_SEED, constraint=c)
    sis.run()
    c.check()
    assert 1 < c.n_states < 64 * 48 + 1 and max(len(stack) for _, stack in c.configs()) <= 4
    ctx, lw = sis.results()
    assert int(sis.active.sum().item()) == 0
    finite = nested = 0
    for cx, w in zip(ctx, lw):
        text = b"".join(vocab[t] for t in cx if t != eos)
        depth = _json_depth(text)
        if np.isfinite(w):
            assert depth is not None and depth <= 4, text
            finite += 1
            nested += depth >= 1  # (an array or an object, not a bracket inside a string)
        else:
            assert depth is None or depth > 4, text
    assert finite > 0 and nested > 0
    engine.check()
