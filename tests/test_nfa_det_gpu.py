"""Determinisation on the GPU (glb_nfa_closure / glb_nfa_subset_round, constraints.determinize): delta, accepting, sets and live,
array for array, against the restatement tests/nfa_det_ref.py - equal arrays test the numbering contract - at the word
boundaries of a set, with nearly every hash colliding, canaries behind every output at exactly the rows needed, the overflow,
and an automaton served by DeviceConstraint(minimize=True) under DeviceSIS.  Everything is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dfa_min_ref as M
from tests import dfa_ref as R
from tests import nfa_det_ref as N
from tests.test_wfsa_gpu import _model

pytestmark = pytest.mark.gpu
ICANARY = 0x5a5a5a5a
_CACHE = {}


def mix(n):
    """n important states, all in the start's closure that are even or the last: x keeps every state, a moves a state 61 up -
    across the words of a set -, b keeps the states at a word's two ends and drops the rest, an empty arc crosses every
    word boundary; the last state - the top bit of the last word - accepts.  The start has no arc: it is not important."""
    from genlm_backend_amd.constraints import ByteNFA

    i = np.arange(n)
    hop, edge = i[i + 61 < n], i[(i % 64 == 0) | (i % 64 == 63)]
    src, dst = np.concatenate([i, hop, edge]), np.concatenate([i, hop + 61, edge])
    arc_set = np.zeros((len(src), 256), np.bool_)
    arc_set[:n, 120] = True
    arc_set[n:n + len(hop), 97] = True
    arc_set[n + len(hop):, 98] = True
    arc_set[n + len(hop):, 200:] = True
    cross, first = i[(i % 64 == 63) & (i + 1 < n)], i[(i % 2 == 0) | (i == n - 1)]
    acc = np.zeros(n + 1, np.bool_)
    acc[n - 1] = True
    return ByteNFA(n + 1, n, acc, src, dst, arc_set, np.concatenate([np.full(len(first), n), cross]), np.concatenate([first, cross + 1]))


def _hand(n, start, accepting, arcs=(), eps=()):
    """A hand-made NFA: arcs (src, dst, bytes), eps (src, dst)."""
    from genlm_backend_amd.constraints import ByteNFA

    arc_set = np.zeros((len(arcs), 256), np.bool_)
    for k, (_, _, read) in enumerate(arcs):
        arc_set[k, list(read)] = True
    acc = np.zeros(n, np.bool_)
    acc[list(accepting)] = True
    return ByteNFA(n, start, acc, [a[0] for a in arcs], [a[1] for a in arcs], arc_set, [e[0] for e in eps], [e[1] for e in eps])


def _nfa(name):
    from genlm_backend_amd.constraints import ByteDFA, ByteNFA

    if name not in _CACHE:
        if isinstance(name, bytes):
            x = ByteNFA.from_regex(name)
        elif name.startswith("mix"):
            x = mix(int(name[3:]))
        elif name == "trie":
            x = ByteNFA.from_dfa(ByteDFA.from_strings(M.lexicon_trie()))
        elif name == "trie-sep-trie":
            trie = ByteDFA.from_strings(M.lexicon_trie())
            x = ByteNFA.concat([trie, ByteDFA.from_regex(rb" "), trie])
        else:
            x = {
                "no-arcs": lambda: _hand(1, 0, []),                                           # one state, the empty set, nothing accepted
                "accepting-start": lambda: _hand(1, 0, [0]),
                "eps-self-loop": lambda: _hand(2, 0, [1], [(0, 1, b"a")], [(0, 0), (1, 1), (1, 0)]),
                "unreachable-accepting": lambda: _hand(4, 0, [2, 3], [(0, 2, b"ab"), (1, 3, b"a")]),  # state 3 is important and never met
                "all-bytes": lambda: _hand(2, 0, [1], [(0, 1, range(256)), (1, 1, range(256))]),
                "256-groups": lambda: _hand(257, 0, range(1, 257, 3), [(0, 1 + b, [b]) for b in range(256)] + [(7, 9, b"z"), (9, 7, b"z")]),
            }[name]()
        _CACHE[name] = x
    return _CACHE[name]


def _want(name):
    if ("want", name) not in _CACHE:
        _CACHE[("want", name)] = N.determinize(_nfa(name))
    return _CACHE[("want", name)]


BOUNDARIES = ["mix1", "mix63", "mix64", "mix65", "mix4096"]
DEGENERATE = ["no-arcs", "accepting-start", "eps-self-loop", rb"(a*)*", "unreachable-accepting", "all-bytes", "256-groups"]
CASES = BOUNDARIES + [rb"(a|b)*a(a|b){9}", "trie", "trie-sep-trie"] + DEGENERATE


class Dev:
    """One glb_nfa_args on the device with `cap` rows, a canary behind every output and every scratch buffer."""

    def __init__(self, engine, nfa, cap, hash_mask=0, chunk=None):
        from genlm_backend_amd import _lib
        from genlm_backend_amd.constraints.tables import _nfa_arrays

        self.eng, dev = engine, engine.device
        a = self.arrays = _nfa_arrays(nfa)
        G, W, n = a["n_groups"], a["n_words"], a["n_states"]
        self.cap, self.W, self.chunk = cap, W, min(cap, chunk or cap)
        self.ins = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).to(dev) for k, v in a.items() if isinstance(v, np.ndarray)}
        i = lambda k: torch.full((k,), ICANARY, dtype=torch.int32, device=dev)
        q = lambda k: torch.full((k,), ICANARY, dtype=torch.int64, device=dev)
        self.slots = 1 << max(1, (2 * cap - 1).bit_length())
        self.sizes = dict(eclose=n * W, table=self.slots * 12 // 8, cand=self.chunk * G * W, sets=cap * W, delta=256 * cap, accepting=cap,
                          counts=self.chunk, status=16, live=cap)
        self.out = dict(eclose=q(n * W + 8), table=q(self.sizes["table"] + 2), cand=q(self.sizes["cand"] + 8), sets=q(cap * W + 8),
                        delta=i(256 * cap + 8), accepting=torch.full((cap + 8,), 0x5a, dtype=torch.uint8, device=dev), counts=i(self.chunk + 8),
                        status=i(24), live=torch.full((cap + 8,), 0x5a, dtype=torch.uint8, device=dev))
        self.out["status"][:16] = 0
        p = _lib.NfaArgs()
        p.struct_size = C.sizeof(_lib.NfaArgs)
        for k in ("n_states", "start", "n_important", "n_words", "n_arcs", "n_eps", "n_groups"):
            setattr(p, k, a[k])
        for k in ("eps_off", "eps_to", "bit_of", "arc_off", "arc_dst", "arc_bytes", "accepting_mask", "group_of", "group_lo"):
            setattr(p, k, self.ins[k].data_ptr())
        for k in ("eclose", "table", "cand", "sets", "counts", "status"):
            setattr(p, k, self.out[k].data_ptr())
        p.delta_out, p.accepting_out = self.out["delta"].data_ptr(), self.out["accepting"].data_ptr()
        p.hash_mask, p.max_states, p.chunk, p.table_slots = hash_mask, cap, self.chunk, self.slots
        self.p = p

    def run(self, name, words, budget, batch=64):
        """`name` in calls of `batch` until the words at `words` say stop; the status words."""
        self.p.restart, self.p.rounds = 1, batch
        while True:
            self.eng.nfa_call(name, self.p)
            self.p.restart = 0
            st = self.out["status"].cpu().tolist()
            if st[words + 1] or st[words + 2] or st[words] > budget:
                return st

    def search(self, batch=64):
        """(rounds, converged, flags, states) of the closure and then the search."""
        st = self.run("glb_nfa_closure", 8, self.arrays["n_states"] + 1, batch)
        assert st[9] == 1 and st[10] == 0 and 1 <= st[8] <= self.arrays["n_states"] + 1
        return tuple(self.run("glb_nfa_subset_round", 0, self.cap + 1, batch)[:4])

    def live(self, n):
        from genlm_backend_amd import _lib

        status = torch.zeros(_lib.FSA_STATUS, dtype=torch.int32, device=self.eng.device)
        q = _lib.FsaProductArgs()
        q.struct_size, q.n_states, q.max_states, q.rounds, q.restart = C.sizeof(_lib.FsaProductArgs), n, n, 64, 1
        q.delta_out, q.accepting_out, q.live = (self.out[k].data_ptr() for k in ("delta", "accepting", "live"))
        q.status = status.data_ptr()
        while True:
            self.eng.fsa_call("glb_fsa_live", q)
            q.restart = 0
            st = status.cpu().tolist()
            if st[9] or st[8] > n + 1:
                return st[9]

    def tables(self, n):
        host = lambda k, m: self.out[k][:m].cpu().numpy()
        return dict(delta=host("delta", 256 * n).reshape(n, 256), accepting=host("accepting", n).astype(np.bool_),
                    sets=host("sets", n * self.W).view(np.uint64).reshape(n, self.W), live=host("live", n).astype(np.bool_))

    def canaries_intact(self, live_rows=0):
        sizes = dict(self.sizes, live=live_rows)
        return all(bool((self.out[k][m:] == (0x5a if self.out[k].dtype == torch.uint8 else ICANARY)).all()) for k, m in sizes.items())


def _equal(got, want, keys=("delta", "accepting", "sets", "live")):
    for k in keys:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def _equal_public(out, want):
    dfa, sets, states = out
    assert dfa.start == 0 and dfa.n_states == len(want["accepting"]) and dfa.delta.dtype == np.int32 and dfa.live.dtype == np.bool_
    _equal(dict(delta=dfa.delta, accepting=dfa.accepting, sets=sets, live=dfa.live), want)
    assert states.dtype == np.int32 and np.array_equal(states, want["states"])


# ---- every array, state for state: the word boundaries, growth, wide frontiers, the degenerate automata ---------------------------
@pytest.mark.parametrize("hash_mask", [0, 0xF], ids=["hash", "hash&0xF"])
@pytest.mark.parametrize("case", CASES, ids=[repr(c) for c in CASES])
def test_arrays_state_for_state(engine, case, hash_mask):
    from genlm_backend_amd.constraints import ByteDFA, determinize

    nfa, want = _nfa(case), _want(case)
    n = len(want["accepting"])
    dv = Dev(engine, nfa, n, hash_mask)  # exactly the rows the search needs: one more would be written into a canary
    rounds, converged, flags, states = dv.search()
    assert (converged, flags, states) == (1, 0, n) and dv.canaries_intact()
    _equal(dv.tables(n), want, ("delta", "accepting", "sets"))
    assert dv.live(n) == 1 and dv.canaries_intact(live_rows=n)
    _equal(dv.tables(n), want)
    # the public call
    out = determinize(engine, nfa, _hash_mask=hash_mask)
    assert type(out[0]) is ByteDFA
    _equal_public(out, want)
    engine.check()


def test_what_the_cases_exercise():
    """From the restatement alone: the important states and words of the boundary cases, the sizes of the others."""
    for name, n_imp, words in (("mix1", 1, 1), ("mix63", 63, 1), ("mix64", 64, 1), ("mix65", 65, 2), ("mix4096", 4096, 64)):
        w = _want(name)
        assert len(w["states"]) == n_imp and w["sets"].shape[1] == words and w["accepting"].any()
        if n_imp >= 63:  # the top bit of the last word is in some set, and not in every one
            top = (w["sets"][:, -1] >> np.uint64((n_imp - 1) % 64)) & np.uint64(1)
            assert top.any() and not top.all()
    big = _want("mix4096")
    assert len(big["accepting"]) > 2000 and (np.unpackbits(big["sets"].view(np.uint8), axis=1).sum(axis=1) > 1000).any()
    assert (big["sets"] != 0).all(axis=1).any()  # a set with members in every one of the 64 words
    assert len(_want(rb"(a|b)*a(a|b){9}")["accepting"]) == 1024
    assert len(_want("trie")["accepting"]) == 1440 and len(_want("trie-sep-trie")["accepting"]) > 1440
    assert len(_want("no-arcs")["accepting"]) == 1 and not _want("no-arcs")["sets"].any() and not _want("no-arcs")["live"].any()
    from genlm_backend_amd.constraints.tables import _nfa_arrays

    assert _want("accepting-start")["accepting"].tolist() == [True]
    # 256 groups; a target that is not important is the empty set: of the 256 arcs of the start, the 86 into accepting states and the one into state 9 remain
    assert _nfa_arrays(_nfa("256-groups"))["n_groups"] == 256 and len(_want("256-groups")["accepting"]) == 88 and (_want("256-groups")["delta"][0] < 0).sum() == 169
    assert len(_want("unreachable-accepting")["states"]) == 4 and len(_want("unreachable-accepting")["accepting"]) == 2


def test_a_round_takes_a_chunk_of_the_queue(engine):
    """The candidate sets of a round are a buffer of `chunk` states: with 5 states a round the arrays are the same, after more rounds."""
    for case in (rb"(a|b)*a(a|b){9}", "mix65"):
        want = _want(case)
        n = len(want["accepting"])
        whole, small = Dev(engine, _nfa(case), n), Dev(engine, _nfa(case), n, chunk=5)
        a, b = whole.search(), small.search()
        assert a[1:] == b[1:] == (1, 0, n) and b[0] >= -(-n // 5) and (b[0] > a[0] or n <= 5) and small.canaries_intact()
        _equal(small.tables(n), want, ("delta", "accepting", "sets"))


def test_growth_overflow_raises_and_the_exact_count_passes(engine):
    from genlm_backend_amd.constraints import determinize

    nfa, want = _nfa(rb"(a|b)*a(a|b){9}"), _want(rb"(a|b)*a(a|b){9}")
    n = len(want["accepting"])
    for hash_mask in (0, 0xF):
        with pytest.raises(ValueError, match=f"max_states={n - 1}") as e:
            determinize(engine, nfa, max_states=n - 1, _hash_mask=hash_mask)
        assert int(str(e.value).split("reached at least ")[1].split()[0]) >= n
        _equal_public(determinize(engine, nfa, max_states=n, _hash_mask=hash_mask), want)
    # at the block: the flag, the count, and nothing written past the rows
    dv = Dev(engine, nfa, n - 1)
    rounds, converged, flags, states = dv.search()
    assert (converged, flags) == (0, 1) and states <= n - 1 and dv.out["status"].cpu().tolist()[7] >= n and dv.canaries_intact()
    # a search far past max_states says so at once: 2^15 sets behind a table of 128 slots
    with pytest.raises(ValueError, match="max_states=64"):
        determinize(engine, _nfa(rb"(a|b)*a(a|b){14}"), max_states=64)
    engine.check()


@pytest.mark.parametrize("batch", [64, 7])
def test_many_rounds_in_batches(engine, batch):
    """A literal of 200 bytes: 201 states, each a round of its own, the last finding nothing - several batches of launches."""
    from genlm_backend_amd.constraints import determinize

    text = bytes(97 + (i * i) % 5 for i in range(200))
    nfa, want = _nfa(text), _want(text)
    assert len(want["accepting"]) == 201
    for hash_mask in (0, 0xF):
        dv = Dev(engine, nfa, 201, hash_mask)
        assert dv.search(batch) == (201, 1, 0, 201) and dv.canaries_intact()
        _equal(dv.tables(201), want, ("delta", "accepting", "sets"))
        _equal_public(determinize(engine, nfa, _hash_mask=hash_mask, _batch=batch), want)


def test_the_wide_automata_accept_their_languages(engine):
    from genlm_backend_amd.constraints import determinize

    words = list(dict.fromkeys(M.lexicon_trie()))
    one, _, _ = determinize(engine, _nfa("trie"))
    two, sets, states = determinize(engine, _nfa("trie-sep-trie"))
    rng = np.random.default_rng(3)
    for k in range(300):
        a, b = words[int(rng.integers(len(words)))], words[int(rng.integers(len(words)))]
        assert one.accepts(a) and not one.accepts(a + b" ") and two.accepts(a + b" " + b) and not two.accepts(a) and not two.accepts(a + b" ")
        assert not two.accepts(a + b"  " + b) and one.accepts(a[:-1]) == (a[:-1] in words) and two.accepts(a + b" " + b[:-1]) == (b[:-1] in words)
    # (the first trie's leaves no longer accept and have no arcs: they are not important, the 2882 states leave 2431)
    assert two.live.all() and len(states) == int(N.important(_nfa("trie-sep-trie")).sum()) == 2431 and sets.shape == (two.n_states, 38)


def test_more_than_4096_important_states_is_refused(engine):
    from genlm_backend_amd.constraints import ByteNFA, determinize

    n = 4097
    wide = ByteNFA(n + 1, 0, np.zeros(n + 1, np.bool_), np.arange(n), np.arange(1, n + 1), np.ones((n, 256), np.bool_))
    with pytest.raises(ValueError, match="4096"):
        determinize(engine, wide)


def test_from_regex_on_the_device(engine):
    from genlm_backend_amd.constraints import ByteDFA

    for p in (rb"-?(0|[1-9][0-9]*)(\.[0-9]+)?", rb"( yes| no| maybe)", rb""):
        host = ByteDFA.from_regex(p)
        got = ByteDFA.from_regex(p, device=engine)
        d, acc, old = N.renumber(host.delta, host.accepting, 0)
        assert type(got) is ByteDFA and np.array_equal(got.delta, d) and np.array_equal(got.accepting, acc) and np.array_equal(got.live, host.live[old])
    with pytest.raises(ValueError, match="max_states=3"):
        ByteDFA.from_regex(rb"abcdef", max_states=3, device=engine)


# ---- served ------------------------------------------------------------------------------------------------------------------------
def test_determinised_minimised_and_served_end_to_end(engine):
    from genlm_backend_amd.constraints import ByteDFA, ByteNFA, DeviceConstraint, determinize
    from genlm_backend_amd.sis import DeviceSIS

    vocab, eos, skip = R.synth_vocab(300, 300)
    m = _model(engine, 300)
    word = ByteDFA.from_strings([b"yes", b"no", b"a", b"ab", b"b", b"0", b"10"])
    nfa = ByteNFA.concat([word, ByteNFA.concat([ByteDFA.from_regex(rb"[ ,]"), word]).star()])  # word([ ,]word)*
    want = N.determinize(nfa)
    out = determinize(m, nfa)
    _equal_public(out, want)
    both = out[0]
    c = DeviceConstraint(m, both, vocab, eos, skip_ids=skip, minimize=True)
    assert c.source_dfa is both and c.dfa.n_states <= both.n_states and c.warm()
    ref = R.Ref(want["delta"], want["accepting"], 0, vocab, eos, skip)
    rows = c.mask_rows(c.state_map).cpu().numpy()
    c.check()
    bank = c.bank[:, :c.words].cpu().numpy().view(np.uint32)
    assert (rows >= 2).all()
    for s in range(both.n_states):
        assert np.array_equal(bank[rows[s]], ref.mask(s)), s
    sis = DeviceSIS(m, 64, [5, 17, 99], 6, eos, seed=11, constraint=c)
    sis.run()
    ctx, lw = sis.results()
    assert np.isfinite(lw).any() and int(sis.active.sum().item()) == 0
    for cx, w in zip(ctx, lw):
        text = b"".join(vocab[t] for t in cx if t != eos)
        if np.isfinite(w):
            assert nfa.accepts(text) and both.accepts(text), text
