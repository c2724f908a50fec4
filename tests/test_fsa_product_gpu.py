"""Products of automata on the GPU (glb_fsa_product_round / glb_fsa_live, constraints.product): the search's tables, state for
state, against the NumPy restatement tests/fsa_product_ref.py - equal arrays test the numbering contract - weights as bits,
canaries behind every output, the overflow, and a product served by DeviceConstraint(minimize=True) under DeviceSIS.
Everything is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dfa_min_ref as M
from tests import dfa_ref as R
from tests import fsa_product_ref as F
from tests.test_wfsa_gpu import _model

pytestmark = pytest.mark.gpu
CANARY = 12345.0
ICANARY = 0x5a5a5a5a
OPS = ("and", "or", "sub")
_CACHE = {}


def _operand(name):
    from genlm_backend_amd.constraints import ByteDFA

    if name not in _CACHE:
        if name == "trie":
            _CACHE[name] = ByteDFA.from_strings(M.lexicon_trie())
        elif name == "moved":  # [ab]+c with its states renamed: the start is state 2, and two states that nothing accepts from
            d = np.full((5, 256), -1, np.int32)
            d[2, 97] = d[2, 98] = d[0, 97] = d[0, 98] = 0
            d[0, 99] = 4
            d[2, 100] = d[0, 100] = 1  # d: into a trap
            d[1, :] = 3
            d[3, :] = 1
            _CACHE[name] = ByteDFA(d, np.array([0, 0, 0, 0, 1], np.bool_), 2)
        elif name == "nothing":  # two states, neither accepts: the start itself is not live
            _CACHE[name] = ByteDFA(np.ones((2, 256), np.int32), np.zeros(2, np.bool_), 0)
        elif isinstance(name, bytes):
            _CACHE[name] = ByteDFA.from_regex(name)
        else:
            _CACHE[name] = ByteDFA(*R.automata()[name])
    return _CACHE[name]


# (a, b): the pairs the products are checked on
CASES = {
    "digits-random37": ("digits", "random37"),                # b starts in state 3
    "chain": (rb"a{200}", rb"(aa)*"),                         # 201 rounds with a frontier of one state: past a batch of 64 launches
    "trie-regex": ("trie", rb"[ab]*c?[a-d]{0,3}"),            # wide frontiers, many pairs that one side ends
    "dead-start": (rb"a+", rb"b+"),                           # "and": no string; the start pair goes nowhere
    "no-start": ("nothing", "digits"),                        # a's start is not live: under "and" and "sub" no start pair exists
    "moved-start": ("moved", rb"[a-c]*"),                     # a start that is not state 0, states that are not live
    "trap": ("trap", "everything"),                           # states of a that are not live
}


def _untrimmed(case, op):
    key = ("search", case, op)
    if key not in _CACHE:
        a, b = (_operand(x) for x in CASES[case])
        _CACHE[key] = F.search(F.side(a), F.side(b), op)
    return _CACHE[key]


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


class Dev:
    """One glb_fsa_product_args on the device with `cap` rows a table, a canary behind every output."""

    def __init__(self, engine, a, b, op, cap):
        from genlm_backend_amd import _lib

        self.eng, dev = engine, engine.device
        self.cap, self.weighted = cap, hasattr(a, "arc_logw") or hasattr(b, "arc_logw")
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        self.ins = []
        p = _lib.FsaProductArgs()
        p.struct_size, p.op = C.sizeof(_lib.FsaProductArgs), OPS.index(op)
        for side, x in (("a", a), ("b", b)):
            t = [up(x.delta), up(x.accepting.astype(np.uint8)), up(x.live.astype(np.uint8))]
            setattr(p, "n_" + side, x.n_states), setattr(p, "start_" + side, x.start)
            setattr(p, "delta_" + side, t[0].data_ptr()), setattr(p, "accepting_" + side, t[1].data_ptr()), setattr(p, "live_" + side, t[2].data_ptr())
            if hasattr(x, "arc_logw"):
                t += [up(x.arc_logw), up(x.final_logw)]
                setattr(p, "arc_" + side, t[3].data_ptr()), setattr(p, "final_" + side, t[4].data_ptr())
            self.ins += t
        i = lambda n: torch.full((n,), ICANARY, dtype=torch.int32, device=dev)
        f = lambda n: torch.full((n,), CANARY, dtype=torch.float32, device=dev)
        u = lambda n: torch.full((n,), 0x5a, dtype=torch.uint8, device=dev)
        self.slots = 1 << max(1, (2 * cap - 1).bit_length())
        self.table = torch.zeros(2 * self.slots + 2, dtype=torch.int64, device=dev)
        self.table[-2:] = ICANARY
        self.pairs, self.delta, self.counts, self.status = i(2 * cap + 8), i(256 * cap + 8), i(cap + 8), i(24)
        self.accepting, self.live, self.arc, self.final = u(cap + 8), u(cap + 8), f(256 * cap + 8), f(cap + 8)
        p.max_states, p.table, p.table_slots = cap, self.table.data_ptr(), self.slots
        p.pairs, p.delta_out, p.accepting_out = self.pairs.data_ptr(), self.delta.data_ptr(), self.accepting.data_ptr()
        p.live, p.counts, p.status = self.live.data_ptr(), self.counts.data_ptr(), self.status.data_ptr()
        if self.weighted:
            p.arc_out, p.final_out = self.arc.data_ptr(), self.final.data_ptr()
        self.p = p

    def search(self, batch=64):
        """Rounds in calls of `batch` until the words say stop; (rounds, converged, flags, states)."""
        self.p.restart, self.p.rounds = 1, batch
        while True:
            self.eng.fsa_call("glb_fsa_product_round", self.p)
            self.p.restart = 0
            st = self.status.cpu().tolist()
            if st[1] or st[2] or st[0] > self.cap + 1:
                return tuple(st[:4])

    def sweep(self, n, batch=64):
        self.p.n_states, self.p.restart, self.p.rounds = n, 1, batch
        while True:
            self.eng.fsa_call("glb_fsa_live", self.p)
            self.p.restart = 0
            st = self.status.cpu().tolist()
            if st[9] or st[8] > n + 1:
                return st[8], st[9], st[10]

    def tables(self, n):
        host = lambda t, k: t[:k].cpu().numpy()
        return dict(delta=host(self.delta, 256 * n).reshape(n, 256), pairs=host(self.pairs, 2 * n).reshape(n, 2),
                    accepting=host(self.accepting, n), live=host(self.live, n), arc_logw=host(self.arc, 256 * n).reshape(n, 256),
                    final_logw=host(self.final, n))

    def canaries_intact(self, n_live=None):
        cap = self.cap
        ok = bool((self.pairs[2 * cap:] == ICANARY).all()) and bool((self.delta[256 * cap:] == ICANARY).all())
        ok = ok and bool((self.counts[cap:] == ICANARY).all()) and bool((self.status[16:] == ICANARY).all()) and bool((self.table[-2:] == ICANARY).all())
        ok = ok and bool((self.accepting[cap:] == 0x5a).all()) and bool((self.live[cap if n_live is None else n_live:] == 0x5a).all())
        ok = ok and bool((self.arc[256 * cap if self.weighted else 0:] == CANARY).all())
        return ok and bool((self.final[cap if self.weighted else 0:] == CANARY).all())


def _equal_trimmed(got, pairs, want):
    """The host automaton `product` returned against the restatement's dict."""
    assert got.delta.dtype == np.int32 and np.array_equal(got.delta, want["delta"]) and got.start == 0
    assert np.array_equal(got.accepting, want["accepting"]) and np.array_equal(got.live, want["live"]) and got.live.dtype == np.bool_
    assert pairs.dtype == np.int32 and np.array_equal(pairs, want["pairs"]) and got.n_states == len(want["live"])
    if want["arc_logw"] is not None:
        assert np.array_equal(_bits(got.arc_logw), _bits(want["arc_logw"])) and np.array_equal(_bits(got.final_logw), _bits(want["final_logw"]))


# ---- the search, the liveness and the trim, array for array ------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("case", list(CASES))
def test_tables_state_for_state(engine, case, op):
    from genlm_backend_amd.constraints import ByteDFA, product

    a, b = (_operand(x) for x in CASES[case])
    want = _untrimmed(case, op)
    n = len(want["accepting"])
    dv = Dev(engine, a, b, op, n)  # exactly the rows the search needs: one more would be written into a canary
    rounds, converged, flags, states = dv.search()
    assert (converged, flags, states) == (1, 0, n) and dv.canaries_intact(n_live=0)
    got = dv.tables(n)
    assert np.array_equal(got["pairs"], want["pairs"]) and np.array_equal(got["delta"], want["delta"])
    assert np.array_equal(got["accepting"].astype(np.bool_), want["accepting"])
    live = F.liveness(want["delta"], want["accepting"])
    sweeps, settled, lflags = dv.sweep(n)
    assert (settled, lflags) == (1, 0) and 1 <= sweeps <= n + 1 and np.array_equal(dv.tables(n)["live"].astype(np.bool_), live)
    assert dv.canaries_intact(n_live=n) and dv.status.cpu().tolist()[:4] == [rounds, 1, 0, n]
    if case == "chain":  # every state is a frontier of its own, the last finds nothing: batches of 64 launches, several of them
        assert rounds == n and (op != "and" or n == 201)
        one = Dev(engine, a, b, op, n)
        assert one.search(batch=7) == (rounds, 1, 0, n) and np.array_equal(one.tables(n)["delta"], want["delta"])
    if case == "dead-start" and op == "and":
        assert n == 1 and want["pairs"].tolist() == [[0, 0]] and not live.any()
    if case == "no-start":
        assert (n == 1 and want["pairs"].tolist() == [[-1, -1]] and not live.any()) if op != "or" else want["pairs"][0].tolist() == [-1, 0]
    # the public call: trimmed, `live` from the device
    both, pairs = product(engine, a, b, op)
    trimmed = F.trim(want)
    assert type(both) is ByteDFA
    _equal_trimmed(both, pairs, trimmed)
    assert both.live.all() or both.n_states == 1
    engine.check()


def test_what_the_cases_exercise():
    """From the restatement alone: the states before and after the trim.  "or" never trims - a pair exists there because a side
    of it is live; the differences a{200} - (aa)* and [ab]+c - [a-c]* are empty: every state but the start goes."""
    sizes = {(case, op): (len(_untrimmed(case, op)["accepting"]), len(F.trim(_untrimmed(case, op))["live"])) for case in CASES for op in OPS}
    assert all(before == after for (_, op), (before, after) in sizes.items() if op == "or")
    assert sizes[("dead-start", "and")] == (1, 1) and sizes[("chain", "and")] == (201, 201) and sizes[("chain", "sub")] == (201, 1)
    assert sizes[("moved-start", "sub")][1] == 1 < sizes[("moved-start", "sub")][0] and sizes[("trap", "sub")][1] == 1
    for op in ("and", "sub"):  # wide frontiers (more than one block's worth of states) and a trim that drops some states, not all
        before, after = sizes[("trie-regex", op)]
        assert before > 256 and 1 < after < before


def test_overflow_raises_and_the_exact_count_passes(engine):
    from genlm_backend_amd.constraints import product

    a, b = (_operand(x) for x in CASES["trie-regex"])
    n = len(_untrimmed("trie-regex", "sub")["accepting"])
    with pytest.raises(ValueError, match=f"max_states={n - 1}") as e:
        product(engine, a, b, "sub", max_states=n - 1)
    reached = int(str(e.value).split("reached at least ")[1].split()[0])
    assert reached == n  # the count of the first round that passed n - 1: no later round ran
    both, pairs = product(engine, a, b, "sub", max_states=n)
    _equal_trimmed(both, pairs, F.trim(_untrimmed("trie-regex", "sub")))
    # at the block: the flag, the count, and nothing written past the rows
    dv = Dev(engine, a, b, "sub", n - 1)
    rounds, converged, flags, states = dv.search()
    assert (converged, flags) == (0, 1) and states <= n - 1 and dv.status.cpu().tolist()[7] == reached and dv.canaries_intact(n_live=0)


def _dense(seed, S=1000):
    """A seeded automaton of S states, seven arcs in ten present: a pair of them reaches about S * S pairs within three rounds."""
    from genlm_backend_amd.constraints import ByteDFA

    if ("dense", seed) not in _CACHE:
        rng = np.random.default_rng(seed)
        d = rng.integers(0, S, (S, 256)).astype(np.int32)
        d[rng.random((S, 256)) < 0.3] = -1
        acc = rng.random(S) < 0.2
        acc[0] = True
        _CACHE[("dense", seed)] = ByteDFA(d, acc, 0)
    return _CACHE[("dense", seed)]


@pytest.mark.parametrize("max_states", [1024, 1 << 18])
def test_a_wide_search_far_past_max_states_is_the_overflow_and_ends_at_once(engine, max_states):
    """Two dense automata of 1000 states: the second round's 120 or so states reach some 15000 distinct pairs and the third's
    far more than any table here holds - 2048 slots under max_states = 1024, 2^19 under the default.  The search must say
    `max_states`, never that its table is full, and must not probe a full table arc by arc: the flag goes up in the middle of
    the expansion and the launch drains."""
    from genlm_backend_amd.constraints import product

    a, b = _dense(1), _dense(2)
    with pytest.raises(ValueError, match=f"max_states={max_states}") as e:
        product(engine, a, b, "and", max_states=max_states)
    assert int(str(e.value).split("reached at least ")[1].split()[0]) > max_states
    if max_states == 1024:  # at the block: bit 0 alone, nothing numbered past the rows, nothing written behind them
        dv = Dev(engine, a, b, "and", max_states)
        rounds, converged, flags, states = dv.search()
        st = dv.status.cpu().tolist()
        assert (converged, flags) == (0, 1) and states <= max_states and st[7] > max_states and dv.canaries_intact(n_live=0)
    engine.check()


# ---- weights ----------------------------------------------------------------------------------------------------------------------
def _weighted(dfa, k, m):
    from genlm_backend_amd.constraints import ByteWFSA

    arc = np.where(dfa.delta >= 0, -np.float32(k) * (1 + np.arange(256) % 7).astype(np.float32), -np.inf).astype(np.float32)
    fin = np.where(dfa.accepting, -np.float32(m) * (1 + np.arange(dfa.n_states) % 3).astype(np.float32), -np.inf).astype(np.float32)
    return ByteWFSA(dfa.delta, arc, fin, dfa.start)


def test_a_weighted_lexicon_and_a_regex_keep_the_lexicons_bits(engine):
    from genlm_backend_amd.constraints import ByteWFSA, product

    rng = np.random.default_rng(2)
    lex = ByteWFSA.from_weighted_strings({w: float(np.float32(-0.1 * rng.integers(1, 50))) for w in dict.fromkeys(M.lexicon_trie())})
    rx = _operand(rb"[ab]*c?[a-d]{0,3}")
    for a, b, side in ((lex, rx, 0), (rx, lex, 1)):
        both, pairs = product(engine, a, b, "and")
        want = F.product(a, b, "and")
        assert type(both) is ByteWFSA and 1 < both.n_states < lex.n_states
        _equal_trimmed(both, pairs, want)
        src = pairs[:, side]
        there = both.delta >= 0
        assert (src >= 0).all() and np.array_equal(_bits(both.arc_logw)[there], _bits(lex.arc_logw[src])[there]) and np.isneginf(both.arc_logw[~there]).all()
        assert np.array_equal(_bits(both.final_logw)[both.accepting], _bits(lex.final_logw[src])[both.accepting]) and both.accepting.any()
        assert np.isneginf(both.final_logw[~both.accepting]).all()
        for w in list(dict.fromkeys(M.lexicon_trie()))[:200]:
            assert both.path_logw(w).tobytes() == (lex.path_logw(w) if rx.accepts(w) else np.float32(-np.inf)).tobytes()
    # the difference keeps a's weights too
    rest, pairs = product(engine, lex, rx, "sub")
    _equal_trimmed(rest, pairs, F.product(lex, rx, "sub"))
    assert type(rest) is ByteWFSA and rest.n_states + both.n_states >= lex.n_states  # (a prefix has a word the regex takes below it, or one it does not)


def test_two_weighted_operands_add_as_float32(engine):
    from genlm_backend_amd.constraints import ByteWFSA, product

    a, b = _weighted(_operand("random37"), 0.1, 0.3), _weighted(_operand(rb".*a.{2}"), 0.2, 0.7)
    want = F.search(F.side(a), F.side(b), "and")
    n = len(want["accepting"])
    dv = Dev(engine, a, b, "and", n)
    assert dv.search()[1:] == (1, 0, n) and dv.canaries_intact(n_live=0)
    got = dv.tables(n)
    assert np.array_equal(got["delta"], want["delta"]) and np.array_equal(_bits(got["arc_logw"]), _bits(want["arc_logw"]))
    assert np.array_equal(_bits(got["final_logw"]), _bits(want["final_logw"]))
    both, pairs = product(engine, a, b, "and")
    _equal_trimmed(both, pairs, F.product(a, b, "and"))
    assert type(both) is ByteWFSA
    there = both.delta >= 0
    sums = (a.arc_logw[pairs[:, 0]] + b.arc_logw[pairs[:, 1]]).astype(np.float32)  # float32 + float32: one rounding
    exact = a.arc_logw[pairs[:, 0]].astype(np.float64) + b.arc_logw[pairs[:, 1]].astype(np.float64)
    assert np.array_equal(_bits(both.arc_logw)[there], _bits(sums)[there]) and (sums[there].astype(np.float64) != exact[there]).any()  # sums that round
    fin = (a.final_logw[pairs[:, 0]] + b.final_logw[pairs[:, 1]]).astype(np.float32)
    assert np.array_equal(_bits(both.final_logw), _bits(fin)) and np.isfinite(fin).any()


# ---- served ------------------------------------------------------------------------------------------------------------------------
def test_a_product_minimised_and_served_end_to_end(engine):
    from genlm_backend_amd.constraints import DeviceConstraint, product
    from genlm_backend_amd.sis import DeviceSIS

    vocab, eos, skip = R.synth_vocab(300, 300)
    m = _model(engine, 300)
    a, b = _operand(rb"[0-9]+[a-z]*"), _operand(rb"([0-9][0-9])+(yes|no|[ab])*")
    both, pairs = product(m, a, b, "and")
    want = F.product(a, b, "and")
    _equal_trimmed(both, pairs, want)
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
        in_a, in_b = a.accepts(text), b.accepts(text)
        if np.isfinite(w):
            assert in_a and in_b, text
        if in_a != in_b:
            assert np.isneginf(w), text


# ---- argument errors ---------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(engine):
    from genlm_backend_amd import _lib

    a, b = _weighted(_operand("digits"), 0.5, 0.25), _operand("random37")
    dv = Dev(engine, a, b, "and", 64)
    n = dv.search()[3]
    dv.sweep(n)
    torch.cuda.synchronize()
    tensors = [dv.pairs, dv.delta, dv.counts, dv.status, dv.table, dv.accepting, dv.live, dv.arc, dv.final]
    before = [t.clone() for t in tensors]
    lib, st = engine.lib, engine._stream()

    def broken(field, value):
        q = _lib.FsaProductArgs.from_buffer_copy(dv.p)
        q.rounds, q.restart = 4, 1
        setattr(q, field, value)
        return q

    # (field, value, what the message names: the field unless said otherwise)
    shared = [("struct_size", 0), ("struct_size", C.sizeof(_lib.FsaProductArgs) - 8), ("max_states", 0), ("max_states", (1 << 22) + 1),
              ("rounds", 0), ("rounds", 65537), ("delta_out", None), ("accepting_out", None), ("status", None)]
    search = [("op", 3), ("op", -1), ("n_a", 0), ("n_b", -1), ("start_a", 2), ("start_b", -1), ("delta_a", None), ("delta_b", None),
              ("accepting_a", None), ("live_b", None), ("final_a", None), ("arc_out", None), ("final_out", None), ("table_slots", dv.slots // 2),
              ("table_slots", dv.slots + 1), ("table", None), ("pairs", None), ("counts", None),
              ("op", _lib.FSA_OR, "arc_a"), ("arc_b", dv.ins[3].data_ptr())]  # weights under "or"; an arc_b without its final_b
    live = [("n_states", 0), ("n_states", 65), ("live", None)]
    for fn, own in ((lib.glb_fsa_product_round, search), (lib.glb_fsa_live, live)):
        assert fn(None, st) == _lib.GLB_EINVAL
        for field, value, *named in shared + own:
            assert fn(C.byref(broken(field, value)), st) == _lib.GLB_EINVAL and (named or [field])[0] in _lib.last_error(), (field, value)
    torch.cuda.synchronize()
    assert all(torch.equal(t, x) for t, x in zip(tensors, before))  # nothing ran
    assert dv.search()[1:] == (1, 0, n) and dv.canaries_intact(n_live=n)  # the unbroken block does run
