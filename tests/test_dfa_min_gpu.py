"""Minimisation on the GPU (glb_dfa_refine / glb_dfa_quotient, constraints.minimize, DeviceConstraint(minimize=True)): `cls`
bit for bit against the NumPy restatement tests/dfa_min_ref.py, the quotient against the restatement's, weights and served
rows bit for bit before and after, and DeviceSIS under a minimised constraint against the unminimised one.  Everything is
exact.  The flag word's path (a hash collision) has no test: the table is cleared by every round, so no state of it can be
preloaded."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dfa_min_ref as M
from tests import dfa_ref as R
from tests.test_regex_cpu import PATTERNS
from tests.test_wfsa_gpu import _model, _spread_vocab

pytestmark = pytest.mark.gpu
CANARY = 12345.0
ICANARY = 0x5a5a5a5a
_CACHE = {}


def _automaton(name):
    """(delta, accepting, start), made once."""
    from genlm_backend_amd.constraints import ByteDFA

    if name not in _CACHE:
        if name == "trie":
            t = ByteDFA.from_strings(M.lexicon_trie())
            _CACHE[name] = (t.delta, t.accepting, t.start)
        elif name == "chain":
            t = ByteDFA.from_regex(rb"a{200}")
            _CACHE[name] = (t.delta, t.accepting, t.start)
        elif name == "doubled":
            _CACHE[name] = M.doubled(*R.automata()["random37"])
        else:
            _CACHE[name] = R.automata()[name]
    return _CACHE[name]


def _reference(name):
    """(keep, cls, rounds) of the restatement for an unweighted automaton, made once."""
    key = ("ref", name)
    if key not in _CACHE:
        d, acc, start = _automaton(name)
        keep = M.keep_of(d, acc, start)
        _CACHE[key] = (keep,) + M.refine(d, keep, np.asarray(acc).astype(np.int64))
    return _CACHE[key]


def _vocab(V):
    if V not in _CACHE:
        _CACHE[V] = R.synth_vocab(V, V)
    return _CACHE[V]


class Dev:
    """The tables of one glb_dfa_min_args on the device, a canary behind every output."""

    def __init__(self, engine, d, keep, final_bits, arc_bits=None, arc_logw=None, final_logw=None, accepting=None):
        self.eng, dev = engine, engine.device
        self.S = S = len(keep)
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.delta, self.keep = up(np.asarray(d, np.int32)), up(np.asarray(keep, np.uint8))
        self.final_bits = up(np.asarray(final_bits).astype(np.uint32).view(np.int32))
        self.arc_bits = up(None if arc_bits is None else np.asarray(arc_bits).astype(np.uint32).view(np.int32))
        self.arc_logw, self.final_logw = up(arc_logw), up(final_logw)
        self.accepting = up(None if accepting is None else np.asarray(accepting, np.uint8))
        i = lambda n: torch.full((n,), ICANARY, dtype=torch.int32, device=dev)
        self.cls, self.scratch, self.status = i(S + 8), i(S + 8), i(16)
        self.slots = 1 << max(1, (2 * S - 1).bit_length())
        self.table = torch.zeros(self.slots * 12 // 8 + 2, dtype=torch.int64, device=dev)
        self.table[-2:] = ICANARY
        self.outs = None

    def args(self, rounds=64, restart=0):
        from genlm_backend_amd import _lib

        p = _lib.DfaMinArgs()
        p.struct_size, p.n_states = C.sizeof(_lib.DfaMinArgs), self.S
        p.delta, p.keep, p.final_bits = self.delta.data_ptr(), self.keep.data_ptr(), self.final_bits.data_ptr()
        p.arc_bits = None if self.arc_bits is None else self.arc_bits.data_ptr()
        p.cls, p.scratch, p.table, p.table_slots = self.cls.data_ptr(), self.scratch.data_ptr(), self.table.data_ptr(), self.slots
        p.status, p.rounds, p.restart = self.status.data_ptr(), rounds, restart
        return p

    def refine(self, rounds=64, restart=0):
        """One call; (rounds since the restart, converged, flags, classes, rounds of this call)."""
        self.eng.dfa_call("glb_dfa_refine", self.args(rounds, restart))
        st = self.status.cpu().tolist()
        assert st[4:7] == [0, 0, 0]  # the counts are zero between calls
        return tuple(st[:4]) + (st[7],)

    def converge(self, batch=64, limit=4096):
        st = self.refine(batch, 1)
        while not st[1] and st[0] < limit:
            st = self.refine(batch, 0)
        return st

    def cls_host(self):
        return self.cls[:self.S].cpu().numpy()

    def quotient(self, new_id, rep):
        from genlm_backend_amd import _lib  # noqa: F401

        dev, n = self.eng.device, len(rep)
        self.new_id, self.rep = torch.from_numpy(new_id).to(dev), torch.from_numpy(rep).to(dev)
        f = lambda k: torch.full((k,), CANARY, dtype=torch.float32, device=dev)
        self.outs = [torch.full((n * 256 + 8,), ICANARY, dtype=torch.int32, device=dev), f(n * 256 + 8), f(n + 8),
                     torch.full((n + 8,), 0x5a, dtype=torch.uint8, device=dev)]
        p = self.args()
        p.new_id, p.rep, p.n_new, p.delta_out = self.new_id.data_ptr(), self.rep.data_ptr(), n, self.outs[0].data_ptr()
        if self.arc_logw is not None:
            p.arc_logw, p.final_logw = self.arc_logw.data_ptr(), self.final_logw.data_ptr()
            p.arc_out, p.final_out = self.outs[1].data_ptr(), self.outs[2].data_ptr()
        if self.accepting is not None:
            p.accepting, p.accepting_out = self.accepting.data_ptr(), self.outs[3].data_ptr()
        self.n_new, self.qargs = n, p
        self.eng.dfa_call("glb_dfa_quotient", p)
        return (self.outs[0][:n * 256].cpu().numpy().reshape(n, 256), self.outs[1][:n * 256].cpu().numpy().reshape(n, 256),
                self.outs[2][:n].cpu().numpy(), self.outs[3][:n].cpu().numpy())

    def canaries_intact(self):
        S = self.S
        ok = bool((self.cls[S:] == ICANARY).all()) and bool((self.scratch[S:] == ICANARY).all()) and bool((self.status[8:] == ICANARY).all())
        ok = ok and bool((self.table[-2:] == ICANARY).all())
        if self.outs is not None:
            n = self.n_new
            ok = ok and bool((self.outs[0][n * 256:] == ICANARY).all()) and bool((self.outs[3][n:] == 0x5a).all())
            ok = ok and bool((self.outs[1][n * 256 if self.arc_logw is not None else 0:] == CANARY).all())
            ok = ok and bool((self.outs[2][n if self.arc_logw is not None else 0:] == CANARY).all())
        return ok


def _same(a, b):
    return np.ascontiguousarray(a, np.float32).tobytes() == np.ascontiguousarray(b, np.float32).tobytes()


# ---- the partition and the quotient ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["digits", "everything", "trap", "random37", "trie", "chain", "doubled"])
def test_classes_bit_for_bit(engine, name):
    d, acc, start = _automaton(name)
    keep, want, rounds = _reference(name)
    dv = Dev(engine, d, keep, np.asarray(acc).astype(np.uint32), accepting=acc)
    got = dv.converge()
    cls = dv.cls_host()
    n_classes = len(np.unique(want[want >= 0]))
    assert got == (rounds, 1, 0, n_classes, got[4]) and cls.dtype == np.int32 and np.array_equal(cls, want)
    assert (cls[~keep] == -1).all() and (cls[keep] <= np.nonzero(keep)[0]).all() and dv.canaries_intact()
    # rounds past convergence change nothing: a later call performs nothing
    assert dv.refine(8) == (rounds, 1, 0, n_classes, 0) and np.array_equal(dv.cls_host(), want)
    # a second run gives the same bits, and so does one call of 256 rounds
    dv2 = Dev(engine, d, keep, np.asarray(acc).astype(np.uint32))
    one = dv2.refine(256, 1) if rounds <= 256 else dv2.converge(256)
    assert one[:4] == (rounds, 1, 0, n_classes) and np.array_equal(dv2.cls_host(), want) and dv2.canaries_intact()
    # an odd number of rounds: the result is copied out of `scratch`
    dv3 = Dev(engine, d, keep, np.asarray(acc).astype(np.uint32))
    part = dv3.refine(1, 1)
    assert part[0] == 1 and part[4] == 1 and np.array_equal(dv3.cls_host(), M.refine(d, keep, np.asarray(acc).astype(np.int64), max_rounds=1)[0])
    # the quotient
    new_id, rep = M.new_ids(cls)
    q, _, _, qacc = dv.quotient(new_id, rep)
    wq, _, _, wacc = M.quotient(d, keep, new_id, rep, accepting=acc)
    assert np.array_equal(q, wq) and np.array_equal(qacc.astype(np.bool_), wacc) and dv.canaries_intact()
    expected = {"digits": (2, 2), "everything": (1, 1), "trap": (4, 2), "random37": (37, 37), "trie": (1440, 406), "chain": (201, 201),
                "doubled": (84, 37)}
    assert (len(acc), len(rep)) == expected[name]
    if name == "chain":
        assert rounds == 200
    if name == "doubled":
        assert M.isomorphic((q, qacc, int(new_id[start])), R.automata()["random37"])


def test_every_compiled_pattern_minimises_to_the_restatements_automaton(engine):
    from genlm_backend_amd.constraints import ByteDFA, minimize

    merged = 0
    for pattern in PATTERNS:
        dfa = ByteDFA.from_regex(pattern)
        small, state_map = minimize(engine, dfa)
        wd, wacc, wstart, wmap, _ = M.minimize(dfa.delta, dfa.accepting, dfa.start)
        assert type(small) is ByteDFA and small.n_states == len(wacc) and small.start == wstart == 0, pattern
        assert state_map.dtype == np.int32 and np.array_equal(state_map, wmap), pattern
        assert M.isomorphic((small.delta, small.accepting, small.start), (wd, wacc, wstart)), pattern
        assert np.array_equal(small.delta, wd) and np.array_equal(small.accepting, wacc) and small.live.all(), pattern
        merged += dfa.n_states - small.n_states
    assert merged > 0
    engine.check()


def test_max_rounds_exhausted_raises(engine):
    from genlm_backend_amd.constraints import ByteDFA, minimize

    chain = ByteDFA(*_automaton("chain"))
    with pytest.raises(RuntimeError, match="max_rounds=70"):
        minimize(engine, chain, max_rounds=70)
    small, state_map = minimize(engine, chain, max_rounds=200)
    assert small.n_states == 201 and np.array_equal(state_map, np.arange(201))


# ---- weights --------------------------------------------------------------------------------------------------------------------
def _lexicon(equal_suffix_weights, n=300, seed=4):
    rng = np.random.default_rng(seed)
    chars = np.frombuffer(b"abc", np.uint8)
    words = sorted({bytes(rng.choice(chars, int(rng.integers(1, 8)))) for _ in range(n)})
    if equal_suffix_weights:  # a word's weight depends on its last two letters alone: shared suffixes carry equal bits
        return {w: float(-1.0 - (w[-1] % 3) - 0.25 * (w[-2:][0] % 3)) for w in words}
    return {w: -0.5 * float(rng.integers(1, 5)) for w in words}  # four seeded levels: suffixes merge only where they happen to agree


@pytest.mark.parametrize("equal", [True, False], ids=["equal-suffix-weights", "seeded-weights"])
def test_weighted_quotient_keeps_every_path_bit_for_bit(engine, equal):
    from genlm_backend_amd.constraints import ByteWFSA, minimize

    lex = _lexicon(equal)
    wf = ByteWFSA.from_weighted_strings(lex)
    small, state_map = minimize(engine, wf)
    keep = M.keep_of(wf.delta, wf.accepting, wf.start)
    cls, _ = M.refine(wf.delta, keep, wf.final_logw.view(np.uint32), wf.arc_logw.view(np.uint32))
    new_id, rep = M.new_ids(cls)
    assert type(small) is ByteWFSA and np.array_equal(state_map, new_id) and small.n_states == len(rep) < wf.n_states
    wd, warc, wfin, _ = M.quotient(wf.delta, keep, new_id, rep, wf.arc_logw, wf.final_logw)
    assert np.array_equal(small.delta, wd) and _same(small.arc_logw, warc) and _same(small.final_logw, wfin)
    unweighted = len(M.new_ids(M.refine(wf.delta, keep, wf.accepting.astype(np.int64))[0])[1])
    assert small.n_states >= unweighted and (equal or small.n_states > unweighted)
    for s in lex:
        assert small.path_logw(s).tobytes() == wf.path_logw(s).tobytes() and np.isfinite(small.path_logw(s))
    rng = np.random.default_rng(8)
    rejected = 0
    while rejected < 500:
        s = bytes(rng.choice(np.frombuffer(b"abcd", np.uint8), int(rng.integers(0, 9))))
        if s not in lex:
            rejected += 1
            assert np.isneginf(small.path_logw(s)) and np.isneginf(wf.path_logw(s))


@pytest.mark.parametrize("semiring", ["log", "max"])
def test_minimised_after_the_push_equals_the_pushed_twin_through_state_map(engine, semiring):
    from genlm_backend_amd.constraints import ByteWFSA, DeviceConstraint

    vocab, eos, skip = _vocab(300)
    wf = ByteWFSA.from_weighted_strings(_lexicon(True))
    twin = DeviceConstraint(engine, wf, vocab, eos, skip_ids=skip, push=semiring, mask_bank_bytes=4 << 20)
    c = DeviceConstraint(engine, wf, vocab, eos, skip_ids=skip, push=semiring, mask_bank_bytes=4 << 20, minimize=True)
    pw, mw = twin.pushed_wfsa(), c.pushed_wfsa()
    sm = c.state_map.cpu().numpy()
    stats = c.minimize_stats()
    assert c.source_dfa is wf and c.dfa is not wf and c.state_map.dtype == torch.int32 and c.state_map.shape == (wf.n_states,)
    assert stats["states_in"] == wf.n_states and stats["states_out"] == c.dfa.n_states == mw.n_states < wf.n_states and stats["rounds"] >= 1
    assert c.start_logw == twin.start_logw and torch.equal(c.backward, twin.backward) and c.backward.shape == (wf.n_states,)
    assert c.dfa.start == sm[wf.start] == 0 and (sm >= 0).all()  # a trie: every state is live and reachable
    for s in range(wf.n_states):  # every source state's pushed row is the row of its quotient state, relabelled
        to = pw.delta[s]
        assert _same(pw.arc_logw[s], mw.arc_logw[sm[s]]) and pw.final_logw[s].tobytes() == mw.final_logw[sm[s]].tobytes()
        assert np.array_equal(np.where(to >= 0, sm[np.maximum(to, 0)], -1), mw.delta[sm[s]])
    for s in list(_lexicon(True))[:100]:
        assert mw.path_logw(s).tobytes() == pw.path_logw(s).tobytes()
    plain = DeviceConstraint(engine, wf, vocab, eos, skip_ids=skip, mask_bank_bytes=4 << 20)
    assert plain.state_map is None and plain.source_dfa is wf and plain.dfa is wf
    assert plain.minimize_stats() == {"states_in": wf.n_states, "states_out": wf.n_states, "rounds": 0}


def test_standalone_and_constructor_minimisation_are_one_pipeline(engine):
    """Eight weighted strings that share suffixes (35 states) under a 70-token vocabulary (three bit words, two waves): what
    `minimize` returns and what `DeviceConstraint(minimize=True)` serves are the same bits, with weights and without."""
    from genlm_backend_amd.constraints import ByteDFA, ByteWFSA, DeviceConstraint, minimize

    pieces = [b"ed", b"ing", b"walk", b"talk", b"bak", b"cak", b"ke", b"king", b"al", b"lk"]  # ids 59 .. 68: both sides of 64
    vocab = [bytes([48 + i]) * 2 for i in range(33)] + [bytes([97 + i]) for i in range(26)] + pieces + [b"<eos>"]
    eos, skip = 69, (69,)
    assert len(vocab) == 70
    words ={stem + end: w for stem in (b"walk", b"talk", b"bak", b"cak") for end, w in ((b"ed", -1.0), (b"ing", -2.5))}
    wf = ByteWFSA.from_weighted_strings(words)
    assert len(words) == 8 and wf.n_states == 35
    for a in (wf, ByteDFA(wf.delta, wf.accepting, wf.start)):
        small, state_map = minimize(engine, a)
        c = DeviceConstraint(engine, a, vocab, eos, skip_ids=skip, minimize=True)
        assert type(small) is type(c.dfa) is type(a) and small.n_states == c.dfa.n_states < a.n_states
        assert state_map.dtype == np.int32 and np.array_equal(state_map, c.state_map.cpu().numpy())
        assert small.start == c.dfa.start == c.tables.start
        for host in (c.dfa.delta, c._delta.cpu().numpy()):
            assert host.dtype == np.int32 and np.array_equal(small.delta, host)
        for host in (c.dfa.accepting, c._acc.cpu().numpy().astype(np.bool_)):
            assert np.array_equal(small.accepting, host)
        if a is wf:
            for arc, fin in ((c.dfa.arc_logw, c.dfa.final_logw), (c._arc_logw.cpu().numpy(), c._final_logw.cpu().numpy())):
                assert _same(small.arc_logw, arc) and _same(small.final_logw, fin)
            for s, w in words.items():
                assert small.path_logw(s).tobytes() == np.float32(w).tobytes()
        else:
            assert c._arc_logw is None and c._final_logw is None
        # and the rows served are those of a constraint over the standalone quotient
        twin = DeviceConstraint(engine, small, vocab, eos, skip_ids=skip)
        states = torch.arange(small.n_states, dtype=torch.int32, device=engine.device)
        assert c.words == 3 and c.warm() and twin.warm()
        rows_c, rows_t = c.mask_rows(states).cpu().numpy(), twin.mask_rows(states).cpu().numpy()
        c.check(), twin.check()
        assert (rows_c >= 2).all() and c.bank.cpu().numpy()[rows_c].tobytes() == twin.bank.cpu().numpy()[rows_t].tobytes()


# ---- serving --------------------------------------------------------------------------------------------------------------------
def _pair(engine, name, V, weighted, **kw):
    from genlm_backend_amd.constraints import ByteDFA, ByteWFSA, DeviceConstraint

    vocab, eos, skip = _vocab(V)
    d, acc, start = _automaton(name)
    if weighted:  # weights that depend on the byte and on whether the state accepts: equivalent states keep equal bits
        arc = np.where(np.asarray(d) >= 0, -(np.arange(256) % 7).astype(np.float32) / 4, -np.inf).astype(np.float32)
        dfa = ByteWFSA(d, arc, np.where(acc, -0.5, -np.inf).astype(np.float32), start)
    else:
        dfa = ByteDFA(d, acc, start)
    return (DeviceConstraint(engine, dfa, vocab, eos, skip_ids=skip, **kw),
            DeviceConstraint(engine, dfa, vocab, eos, skip_ids=skip, minimize=True, **kw))


@pytest.mark.parametrize("weighted", [False, True], ids=["bits", "weights"])
@pytest.mark.parametrize("name,V,sizes", [("doubled", 300, (84, 37)), ("trie", 2049, (1440, 406))])
def test_served_rows_and_advance_commute_with_state_map(engine, name, V, sizes, weighted):
    plain, small = _pair(engine, name, V, weighted, mask_bank_bytes=64 << 20)
    assert (plain.dfa.n_states, small.dfa.n_states) == sizes and small.minimize_stats()["states_in"] == sizes[0]
    assert plain.warm() and small.warm() and small.capacity == sizes[1] + 2
    sm = small.state_map.cpu().numpy()
    kept = M.keep_of(*_automaton(name))
    assert np.array_equal(sm >= 0, kept)
    dev = engine.device
    src_states = torch.arange(sizes[0], dtype=torch.int32, device=dev)
    rows_plain = plain.mask_rows(src_states).cpu().numpy()
    rows_small = small.mask_rows(small.state_map).cpu().numpy()
    plain.check(), small.check()
    cols = V if weighted else plain.words
    bank_p, bank_s = plain.bank[:, :cols].cpu().numpy(), small.bank[:, :cols].cpu().numpy()
    assert (rows_small[~kept] == 0).all() and (rows_small[kept] >= 2).all()  # dropped states are served row 0
    assert bank_p[rows_plain[kept]].tobytes() == bank_s[rows_small[kept]].tobytes()
    # advance over seeded token strings commutes with the map
    rng = np.random.default_rng(V)
    vocab = _vocab(V)[0]
    n, L = 256, 6
    singles = np.array([t for t in range(V) if len(vocab[t]) == 1 and (name != "trie" or vocab[t] in b"abcd")])
    tok = np.where(rng.random((n, L)) < 0.8, rng.choice(singles, (n, L)), rng.integers(0, V, (n, L))).astype(np.int32)
    start_states = rng.choice(np.nonzero(kept)[0], n).astype(np.int32)
    start_states[::2] = plain.dfa.start  # (a trie's states are mostly deep: half the walks begin where there is room to walk)
    frm = torch.zeros(n, dtype=torch.int32, device=dev)
    to = torch.from_numpy(rng.integers(0, L + 1, n).astype(np.int32)).to(dev)
    tok_d = torch.from_numpy(tok).to(dev)
    a = plain.advance(torch.from_numpy(start_states).to(dev), tok_d, frm, to).cpu().numpy()
    b = small.advance(torch.from_numpy(sm[start_states]).to(dev), tok_d, frm, to).cpu().numpy()
    assert np.array_equal(np.where(a >= 0, sm[np.maximum(a, 0)], -1), b) and min((a >= 0).sum(), (a < 0).sum()) > n // 8
    # the same rows through an evicting bank of 8 + 2 rows
    row_bytes = (small.row_elems if weighted else small.words) * 4
    _, evict = _pair(engine, name, V, weighted, mask_bank_bytes=10 * row_bytes, on_full="evict")
    assert evict._evicting and evict.capacity == 10
    some = rng.permutation(np.nonzero(kept)[0])[:32].astype(np.int32)
    for k in range(0, 32, 8):
        part = some[k:k + 8]
        ids = evict.mask_rows(torch.from_numpy(sm[part]).to(dev)).cpu().numpy()
        ebank = evict.bank[:, :cols].cpu().numpy()
        assert (ids >= 2).all() and ebank[ids].tobytes() == bank_p[rows_plain[part]].tobytes()
    evict.check()
    assert evict.stats()["evictions"] > 0


# ---- end to end -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["regex", "trie"])
@pytest.mark.parametrize("kw", [dict(), dict(use_particle_kv=True, share_kv=False)], ids=["plain", "private-kv"])
def test_device_sis_is_the_same_run_minimised_or_not(engine, kw, source):
    """The finite language of `( yes| no| maybe)`, from the regex (10 states: the subset construction already shares the one
    accepting state, and nothing else is equivalent) and from its trie (12 states, 10 after minimisation)."""
    from genlm_backend_amd.constraints import ByteDFA, DeviceConstraint
    from genlm_backend_amd.sis import DeviceSIS

    V = 300
    m, vocab = _model(engine, V), _spread_vocab(V)
    dfa = ByteDFA.from_regex(rb"( yes| no| maybe)") if source == "regex" else ByteDFA.from_strings([b" yes", b" no", b" maybe"])
    plain = DeviceConstraint(m, dfa, vocab, 0, skip_ids=(0,))
    small = DeviceConstraint(m, dfa, vocab, 0, skip_ids=(0,), minimize=True)
    assert (dfa.n_states, small.dfa.n_states) == ((10, 10) if source == "regex" else (12, 10))
    assert small.minimize_stats()["states_out"] == M.minimize(dfa.delta, dfa.accepting, 0)[0].shape[0]
    runs = []
    for c in (plain, small):
        sis = DeviceSIS(m, 48, [5, 17, 99], 6, 0, seed=11, constraint=c, **kw)
        sis.run()
        c.check()
        runs.append(sis)
    a, b = runs
    for name in ("contexts", "lengths", "log_weights"):
        x, y = getattr(a, name).cpu().numpy(), getattr(b, name).cpu().numpy()
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), name
    sm = small.state_map
    assert torch.equal(torch.where(a.states >= 0, sm[a.states.clamp(min=0).long()], a.states), b.states)
    ctx, lw = b.results()
    assert np.isfinite(lw).any() and int(b.active.sum().item()) == 0
    for cx, w in zip(ctx, lw):
        if np.isfinite(w):
            assert b"".join(vocab[t] for t in cx) in (b" yes", b" no", b" maybe")


# ---- argument errors ------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(engine):
    from genlm_backend_amd import _lib

    d, acc, start = _automaton("doubled")
    keep = M.keep_of(d, acc, start)
    arc = np.where(np.asarray(d) >= 0, 0.0, -np.inf).astype(np.float32)
    fin = np.where(acc, 0.0, -np.inf).astype(np.float32)
    dv = Dev(engine, d, keep, fin.view(np.uint32), arc.view(np.uint32), arc, fin, acc)
    assert dv.refine(1, 1)[:3] == (1, 0, 0)
    new_id, rep = M.new_ids(M.refine(d, keep, fin.view(np.uint32), arc.view(np.uint32))[0])
    dv.quotient(new_id, rep)
    torch.cuda.synchronize()
    tensors = [dv.cls, dv.scratch, dv.status, dv.table] + dv.outs
    before = [t.clone() for t in tensors]
    lib, st = engine.lib, engine._stream()

    def broken(field, value):
        p = dv.qargs
        q = _lib.DfaMinArgs.from_buffer_copy(p)
        q.rounds, q.restart = 4, 0
        setattr(q, field, value)
        return q

    both = [("struct_size", 0), ("struct_size", C.sizeof(_lib.DfaMinArgs) - 8), ("n_states", 0), ("n_states", -1), ("delta", None),
            ("keep", None)]
    refine = [("rounds", 0), ("rounds", 65537), ("table_slots", dv.slots // 2), ("table_slots", dv.slots + 1), ("final_bits", None),
              ("cls", None), ("scratch", None), ("table", None), ("status", None)]
    quotient = [("n_new", 0), ("n_new", dv.S + 1), ("new_id", None), ("rep", None), ("delta_out", None), ("arc_logw", None),
                ("final_logw", None), ("accepting", None)]
    for fn, own in ((lib.glb_dfa_refine, refine), (lib.glb_dfa_quotient, quotient)):
        assert fn(None, st) == _lib.GLB_EINVAL
        for field, value in both + own:
            assert fn(C.byref(broken(field, value)), st) == _lib.GLB_EINVAL and field in _lib.last_error(), (field, value)
    torch.cuda.synchronize()
    assert all(torch.equal(t, b) for t, b in zip(tensors, before))  # nothing ran
    got = dv.converge()  # the unbroken block does run
    assert got[1:3] == (1, 0) and got[3] == len(rep) and dv.canaries_intact()
