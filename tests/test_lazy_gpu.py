"""Lazy determinisation on the GPU (glb_lazy_*, constraints.LazyConstraint): state ids, sets, accepting bits and the count,
array for array after every `advance` call, and every bank row bit for bit, against the restatement tests/lazy_ref.py - at the
word boundaries of a set, with nearly every hash colliding, canaries behind every buffer at exactly the rows needed, the
overflow cut, a bank that evicts, the existing path over the determinised automaton, and a pattern `determinize` refuses served
under DeviceSIS.  Everything is exact."""
import itertools

import numpy as np
import pytest
import torch

from genlm_backend_amd.constraints import LazyConstraint  # (at import: no test of this file passes without the class)
from tests import dfa_ref as R
from tests import lazy_ref as L
from tests.test_wfsa_gpu import _model

pytestmark = pytest.mark.gpu
_CACHE = {}
CANARY = {torch.uint8: 0x5a, torch.int32: 0x5a5a5a5a, torch.int64: 0x5a5a5a5a5a5a5a5a}
A, B, X, HI = 97, 98, 120, 200  # single-byte tokens: the arcs of `ring`


def ring(n):
    """n important states in a ring, all useful: a moves every state one up (the last to state 0, across the words of a set),
    x keeps it, b keeps it and adds the state seven up (sets grow), the bytes from 200 keep the multiples of three alone
    (sets shrink, or die); an empty arc crosses every word boundary; the start - no arc of its own: not important - leads to
    state 0 and to the last state, the top bit of the last word, which accepts, as does the middle one."""
    from genlm_backend_amd.constraints import ByteNFA

    i = np.arange(n)
    third = i[i % 3 == 0]
    src, dst = np.concatenate([i, i, i, third]), np.concatenate([(i + 1) % n, i, (i + 7) % n, third])
    arc_set = np.zeros((len(src), 256), np.bool_)
    arc_set[:n, A] = True
    arc_set[n:2 * n, [B, X]] = True
    arc_set[2 * n:3 * n, B] = True
    arc_set[3 * n:, HI:] = True
    cross = i[(i % 64 == 63) & (i + 1 < n)]
    acc = np.zeros(n + 1, np.bool_)
    acc[[n - 1, n // 2]] = True
    return ByteNFA(n + 1, n, acc, src, dst, arc_set, np.concatenate([[n, n], cross]), np.concatenate([[0, n - 1], cross + 1]))


def _vocab():
    """About 300 tokens: the 256 single bytes, an empty token (256), a skipped one (257), the EOS (258), tokens of up to 70
    bytes, and tokens of a and b alone - one of them 40 bytes - that the automata here can read."""
    if "vocab" not in _CACHE:
        vocab, eos, skip = R.synth_vocab(300, 300)
        vocab = list(vocab)
        vocab[290:300] = [b"ab", b"ba", b"aab", b"bb", b"abab", b"ab" * 20, b"xa", b"ax", b"xx", b"a" * 5]
        _CACHE["vocab"] = (vocab, eos, skip)
    return _CACHE["vocab"]


POOL = np.array([A, B, X, HI, 255, 290, 291, 292, 293, 294, 295, 296, 297, 298, 299, 256, 257, 258, 48, 300, -1], np.int32)
WEIGHT = np.array([8, 8, 6, 3, 1, 2, 2, 1, 1, 1, 1, 2, 2, 1, 1, 0.3, 0.3, 0.3, 0.3, 0.3, 0.3])


def _nfa(name):
    from genlm_backend_amd.constraints import ByteNFA

    if name not in _CACHE:
        _CACHE[name] = ByteNFA.from_regex(name) if isinstance(name, bytes) else ring(int(name[4:]))
    return _CACHE[name]


def _canaried(shape, dtype, dev, extra=8):
    """(whole, view): `view` of `shape` at the front of a buffer whose `extra` elements behind it hold the canary."""
    n = int(np.prod(shape))
    whole = torch.full((n + extra,), CANARY[dtype], dtype=dtype, device=dev)
    return whole, whole[:n].view(shape)


class Dev:
    """A LazyConstraint whose every buffer lies in front of a canary, started over in them, beside its restatement."""

    def __init__(self, engine, nfa, max_states, cand_rows, hash_mask=0, force_wave=False, bank_rows=None, on_full="error"):
        vocab, eos, skip = _vocab()
        words = (len(vocab) + 31) // 32
        kw = {} if bank_rows is None else dict(mask_bank_bytes=bank_rows * words * 4)
        c = self.c = LazyConstraint(engine, nfa, vocab, eos, skip_ids=skip, max_states=max_states, on_full=on_full, _hash_mask=hash_mask,
                                    _force_wave=force_wave, **kw)
        self.ref = L.Ref(nfa, vocab, eos, skip, max_states=max_states)
        dev, self.dev, self.words = c.dev, c.dev, words
        self.whole = {}
        cand_rows = int(max(1, min(cand_rows, c._slots - max_states)))
        for name, shape, dtype in (("_sets", (max_states, c.W), torch.int64), ("_accepting", (max_states,), torch.uint8),
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
        c._call("glb_lazy_init", c._block())
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
        """One call on the device and in the restatement: the ids, the count, the sets and the accepting bits are equal."""
        got = self.c.advance(self.up(states), self.up(tokens), self.up(frm), self.up(to)).cpu().numpy()
        want = self.ref.advance(states, tokens, frm, to)
        assert np.array_equal(got, want), (np.nonzero(got != want)[0][:8], got[got != want][:8], want[got != want][:8])
        assert self.c.n_states == self.ref.n_states
        sets = self.c.sets()
        assert sets.dtype == np.uint64 and np.array_equal(sets, self.ref.sets())
        assert np.array_equal(self.c._accepting[:len(sets)].cpu().numpy().astype(np.bool_), self.ref.accepting())
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
            assert np.array_equal(bank[r], self.want_row(s)), s
        assert self.canaries_intact()
        return ids, seen


def _calls(ref, sizes, seed, ld=4):
    """Random calls over the restatement `ref` as it grows: states from -1 to one past the states known, tokens from POOL,
    ranges inside [0, ld] and a few outside; (states, tokens, frm, to) per call."""
    rng = np.random.default_rng(seed)
    out = []
    for k, n in enumerate(sizes):
        tokens = rng.choice(POOL, (n, ld), p=WEIGHT / WEIGHT.sum()).astype(np.int32)
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
        if k == 3:  # the claim race: 700 particles walk one range to one set that no call has met (ring1 has no such set)
            for seq in itertools.product((295, B, A, HI, 292), repeat=ld):
                row = ref.order[0]
                for t in seq:
                    row = ref.token(row, t)
                if row.any() and row.tobytes() not in ref.ids:
                    break
            states[100:800], tokens[100:800], frm[100:800], to[100:800] = 0, np.array(seq, np.int32), 0, ld
        out.append((states, tokens, frm, to))
        ref.advance(states, tokens, frm, to)
    return out


SIZES = (1, 64, 65, 1000, 1000)
BOUNDARIES = ["ring1", "ring63", "ring64", "ring65", "ring4096"]


def _script(name):
    """The calls of a boundary case and the states they number, from the restatement alone."""
    if ("script", name) not in _CACHE:
        vocab, eos, skip = _vocab()
        ref = L.Ref(_nfa(name), vocab, eos, skip, max_states=1 << 22)
        _CACHE[("script", name)] = (_calls(ref, SIZES, 7 + len(name)), ref.n_states)
    return _CACHE[("script", name)]


# ---- ids, sets, accepting bits and rows, call by call, at the word boundaries of a set ---------------------------------------------------
@pytest.mark.parametrize("hash_mask", [0, 0xF], ids=["hash", "hash&0xF"])
@pytest.mark.parametrize("case", BOUNDARIES)
def test_states_sets_and_rows_call_by_call(engine, case, hash_mask):
    calls, total = _script(case)
    nfa = _nfa(case)
    # exactly the states the calls number and the particles of the largest call: one more of either lands in a canary
    dv = Dev(engine, nfa, total, max(SIZES), hash_mask)
    assert dv.c.W == {"ring1": 1, "ring63": 1, "ring64": 1, "ring65": 2, "ring4096": 64}[case] and np.array_equal(dv.c.bit_state, dv.ref.states)
    other = Dev(engine, nfa, total, max(SIZES), hash_mask, force_wave=True) if dv.c.W == 1 else None
    if other is not None:
        other._rows = dv._rows  # (one restatement's rows for both)
    most = 0
    for states, tokens, frm, to in calls:
        before = dv.ref.n_states
        got = dv.advance(states, tokens, frm, to)
        done = (np.arange(len(got)) % 7 == 0).astype(np.int32)
        ids, seen = dv.rows(got, done)
        most = max(most, dv.ref.n_states - before)
        if other is not None:  # the wave form of the fill, bit for bit the lane form's rows
            assert np.array_equal(other.advance(states, tokens, frm, to), got)
            _, seen_w = other.rows(got, done)
            lane, wave = dv.c.bank[:, :dv.words].cpu().numpy(), other.c.bank[:, :dv.words].cpu().numpy()
            assert seen_w.keys() == seen.keys() and all(np.array_equal(lane[seen[s]], wave[seen_w[s]]) for s in seen)
    assert dv.c.n_states == total and not dv.ref.overflow
    assert most > 64 or case == "ring1"  # one fill served more work entries than its grid has side by side
    dv.c.check()
    engine.check()


def test_what_the_cases_exercise():
    """From the restatement alone: a 1000-particle call in which hundreds of particles reach the same new set, sets with
    members in many words, and every kind of particle a call can hold."""
    for case in BOUNDARIES:
        calls, total = _script(case)
        vocab, eos, skip = _vocab()
        ref = L.Ref(_nfa(case), vocab, eos, skip)
        crowd = 0
        for states, tokens, frm, to in calls:
            before = ref.n_states
            out = ref.advance(states, tokens, frm, to)
            fresh = out[out >= before]
            if len(fresh):
                crowd = max(crowd, int(np.bincount(fresh - before).max()))
            if len(out) == 1000:
                assert (out < 0).any() and (frm == to).any() and (frm > to).any() and (to > tokens.shape[1]).any() and (out >= 0).sum() > 300
        assert ref.n_states == total and (crowd >= 700 or case == "ring1")
        if case != "ring1":
            assert total > 200 and (ref.sets()[:, -1] >> np.uint64((int(case[4:]) - 1) % 64) & np.uint64(1)).any()  # the top bit of the last word
        if case == "ring4096":
            assert ref.sets().shape[1] == 64 and ((ref.sets() != 0).sum(axis=1) > 8).any()  # a set with members in many words


@pytest.mark.parametrize("hash_mask", [0, 0xF], ids=["hash", "hash&0xF"])
def test_degenerate_calls(engine, hash_mask):
    """ld == 0, n == 0, an empty range on a state, a dead state, a state past the count; `to_dfa`; an id that no set has."""
    dv = Dev(engine, _nfa("ring65"), 16, 8, hash_mask)
    z = lambda *v: np.array(v, np.int32)
    first = dv.advance(None, z(A, X, B).reshape(3, 1), z(0, 0, 0), z(1, 1, 1))
    assert (first >= 0).all() and dv.c.n_states > 1
    none = np.zeros((4, 0), np.int32)
    assert dv.advance(z(0, 1, -1, dv.c.n_states), none, z(0, 0, 0, 0), z(0, 0, 0, 0)).tolist() == [0, 1, -1, -1]
    assert dv.advance(z(0, 1, 0, 0), none, z(0, 0, 0, 1), z(0, 1, 1, 1)).tolist() == [0, -1, -1, -1]  # to > ld == 0
    empty = dv.c.advance(None, torch.zeros((0, 3), dtype=torch.int32, device=dv.dev), torch.zeros(0, dtype=torch.int32, device=dv.dev),
                         torch.zeros(0, dtype=torch.int32, device=dv.dev))
    assert empty.shape == (0,) and dv.c.mask_rows(empty).shape == (0,)
    two = z(A, A).reshape(1, 2).repeat(5, axis=0)
    got = dv.advance(z(1, 1, -1, 1, 0), two, z(1, 2, 0, 0, 2), z(1, 1, 1, 3, 2))
    assert got.tolist()[:4] == [1, -1, -1, -1] and got[4] == 0
    assert dv.canaries_intact()
    dv.c.check()
    # the partial automaton over the sets numbered so far: its arcs agree with the restatement's steps
    dfa, sets = dv.c.to_dfa(), dv.c.sets()
    assert dfa.n_states == len(sets) == dv.ref.n_states and dfa.start == 0
    for s in range(len(sets)):
        for byte in (A, B, X, HI, 48):
            t = dv.ref.step(sets[s], byte)
            assert dfa.delta[s, byte] == dv.ref.ids.get(t.tobytes(), -1) if t.any() else dfa.delta[s, byte] == -1
    assert np.array_equal(dfa.accepting, dv.ref.accepting())
    # an id that no set has yet is served row 0 and keeps no row: the set that takes the id is served its own row
    k = dv.c.n_states
    ids = dv.c.mask_rows(dv.up(z(k, 0, k))).cpu().numpy()
    assert ids[0] == 0 and ids[2] == 0 and ids[1] >= 2 and dv.canaries_intact()
    got = dv.advance(z(1, 2), z(A, HI, B, A).reshape(2, 2), z(0, 0), z(2, 2))
    assert k in got.tolist()
    dv.rows(got)
    dv.c.check()


@pytest.mark.parametrize("hash_mask", [0, 0xF], ids=["hash", "hash&0xF"])
def test_overflow_cuts_in_particle_order_and_the_exact_count_passes(engine, hash_mask):
    nfa = _nfa(rb"(a|b)*a(a|b){9}")
    rng = np.random.default_rng(5)
    tokens = rng.choice(np.array([A, B, 290, 291, 293], np.int32), (1000, 4)).astype(np.int32)
    frm, to = np.zeros(1000, np.int32), rng.integers(1, 5, 1000).astype(np.int32)
    vocab, eos, skip = _vocab()
    need = L.Ref(nfa, vocab, eos, skip)
    need.advance(None, tokens, frm, to)
    n = need.n_states
    assert 40 < n < 400
    tight = Dev(engine, nfa, n - 1, 1000, hash_mask)
    got = tight.advance(None, tokens, frm, to)  # (equal to the restatement's cut: ids, sets and the count)
    assert tight.ref.overflow and (got == -1).any() and tight.c.n_states == n - 1
    ids, _ = tight.rows(got)
    assert (ids[got < 0] == 0).all()
    with pytest.raises(RuntimeError, match=f"max_states={n - 1}") as e:
        tight.c.check()
    assert "empty mask" in str(e.value)
    again = tight.advance(got, tokens, to, np.minimum(to + 1, 4).astype(np.int32))  # full from the start: no set is numbered
    assert tight.c.n_states == n - 1 and (again[got < 0] == -1).all()
    exact = Dev(engine, nfa, n, 1000, hash_mask)
    exact.advance(None, tokens, frm, to)
    assert not exact.ref.overflow
    exact.c.check()
    engine.check()


@pytest.mark.parametrize("hash_mask", [0, 0xF], ids=["hash", "hash&0xF"])
def test_a_bank_of_five_rows_evicts_and_serves_right_rows(engine, hash_mask):
    nfa = _nfa(rb"(a|b)*a(a|b){9}")
    dv = Dev(engine, nfa, 64, 8, hash_mask, bank_rows=5, on_full="evict")
    assert dv.c._evicting and dv.c.capacity == 5
    rng = np.random.default_rng(9)
    states = np.zeros(3, np.int32)
    for step in range(60):
        tokens = rng.choice(np.array([A, B], np.int32), (3, 1)).astype(np.int32)
        states = dv.advance(states, tokens, np.zeros(3, np.int32), np.ones(3, np.int32))
        ids, seen = dv.rows(states)
        assert (ids >= 2).all()
        if dv.c.n_states >= 40:
            break
    assert dv.c.n_states >= 40
    st = dv.c.stats()
    assert st["evictions"] > 0 and st["rows_in_use"] == 5 and st["states"] == dv.c.n_states
    dv.c.check()
    k = dv.c.n_states  # an id that no set has yet: row 0, and its claim taken back
    assert dv.c.mask_rows(dv.up(np.array([k, 0], np.int32))).cpu().numpy()[0] == 0 and int(dv.c._row_of_state[k].item()) == -1
    dv.c.check()
    ids = dv.c.mask_rows(dv.up(np.array([0, 1, 2, 3], np.int32))).cpu().numpy()  # four distinct sets in one call: one is left without a row
    bank = dv.c.bank[:, :dv.words].cpu().numpy().view(np.uint32)
    assert (ids == 0).sum() == 1 and all(np.array_equal(bank[r], dv.want_row(s)) for s, r in enumerate(ids) if r) and dv.canaries_intact()
    with pytest.raises(RuntimeError, match="smaller than one step's working set"):
        dv.c.check()


@pytest.mark.parametrize("hash_mask", [0, 0xF], ids=["hash", "hash&0xF"])
def test_against_the_determinised_automaton_served_by_device_constraint(engine, hash_mask):
    from genlm_backend_amd.constraints import DeviceConstraint, determinize

    vocab, eos, skip = _vocab()
    nfa = _nfa(rb"(a|b)*a(a|b){9}")
    eager = DeviceConstraint(engine, determinize(engine, nfa)[0], vocab, eos, skip_ids=skip)
    lazy = LazyConstraint(engine, nfa, vocab, eos, skip_ids=skip, max_states=8192, _hash_mask=hash_mask)
    rng = np.random.default_rng(21)
    n, steps = 256, 24
    tokens = rng.choice(np.array([A, B, 290, 291, 292, 293, 294], np.int32), (n, steps)).astype(np.int32)
    tokens[rng.random((n, steps)) < 0.01] = 48  # (a byte the pattern does not read: the particle dies)
    tok = torch.from_numpy(tokens).to(engine.device)
    se, sl = eager.states0(n), lazy.states0(n)
    for t in range(steps):
        frm, to = (torch.full((n,), v, dtype=torch.int32, device=engine.device) for v in (t, t + 1))
        se, sl = eager.advance(se, tok, frm, to), lazy.advance(sl, tok, frm, to)
        done = torch.full((n,), int(t == steps - 1), dtype=torch.int32, device=engine.device)
        re, rl = eager.mask_rows(se, done=done), lazy.mask_rows(sl, done=done)
        assert torch.equal(se < 0, sl < 0), t
        assert torch.equal(eager.bank[re.long(), :eager.words], lazy.bank[rl.long(), :lazy.words]), t
    assert int((sl < 0).sum()) > 0 and int((sl >= 0).sum()) > 100 and 200 < lazy.n_states <= 1024
    eager.check()
    lazy.check()
    engine.check()


@pytest.mark.parametrize("hash_mask", [0, 0xF], ids=["hash", "hash&0xF"])
def test_a_pattern_determinize_refuses_is_served_under_sis(engine, hash_mask):
    from genlm_backend_amd.constraints import ByteNFA, determinize
    from genlm_backend_amd.sis import DeviceSIS

    vocab, eos, skip = _vocab()
    m = _model(engine, 300)
    nfa = ByteNFA.from_regex(rb"(a|b)*a(a|b){40}")
    with pytest.raises(ValueError, match="max_states=65536"):
        determinize(m, nfa, max_states=65536)
    c = LazyConstraint(m, nfa, vocab, eos, skip_ids=skip, max_states=65536, _hash_mask=hash_mask)
    assert c.W == 2 and not c._evicting
    sis = DeviceSIS(m, 64, [5, 17, 99], 48, eos, seed=11, constraint=c)
    sis.run()
    c.check()
    assert 1 < c.n_states < 64 * 48 + 1
    ctx, lw = sis.results()
    assert int(sis.active.sum().item()) == 0
    finished = 0
    for cx, w in zip(ctx, lw):
        if np.isfinite(w):
            text = b"".join(vocab[t] for t in cx if t != eos)
            assert nfa.accepts(text), text
            finished += 1
    assert finished > 0
    engine.check()
