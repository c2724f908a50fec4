"""A byte beam under a byte automaton on the GPU (glb_bytelm_step, `ByteBeam(constraint=...)`, `ByteSIS`)
against the float64 restatement tests/bytelm_constraint_ref.py.

The kernel tests use the harness of tests/test_bytelm_gpu.py: the restatement gets the DEVICE's masses, so nodes, states,
flags and bytes are compared exactly and only the kernel's float32 arithmetic is under a tolerance - TOL = 1e-5 absolute on a
log-probability of P_MIN = 1e-6 and more and on log Zc: the handful of float32 operations of the unconstrained row plus one
more logsumexp over at most 257 terms.  Forbidden columns are compared exactly (-inf).  A uniform handed to the kernel is the
midpoint of the float64 CDF interval of a column of probability 1e-3 and more: 5e-4 from either end against about 1e-6 of
float32 error, so the byte drawn must be that column and no case is skipped.  The end-to-end tests feed the restatement the
model's own rows and allow GAP = 1e-3 (tests/test_beam_gpu.py)."""
import math
import types

import numpy as np
import pytest
import torch

from tests import bytelm_constraint_ref as CR
from tests import bytelm_ref as R
from tests.test_bytelm_gpu import DT, GAP, P_MIN, TOL, _cands, _check_row, _state, _tables, _trie

pytestmark = pytest.mark.gpu

STRINGS = [b"ab", b"abc", b"b", b"ca", b"zz"]  # "z" is no letter of the vocabulary: the state behind it has no mass to offer
NINF = -np.inf


def _walk(a, text):
    s = a.start
    for b in text:
        s = int(a.delta[s, b])
    return s


def _automata(engine):
    """{name: (host automaton or namespace, DeviceTables, {scenario: state})}: the trie of STRINGS with two more states - X,
    whose only arc leads to D, from which nothing is accepted; the same tables with unequal weights, one arc of -inf that
    delta still has; the one state that allows everything."""
    from genlm_backend_amd.constraints import ByteDFA
    from genlm_backend_amd.constraints.tables import DeviceTables

    base = ByteDFA.from_strings(STRINGS)
    S0 = base.n_states
    delta = np.concatenate([base.delta, np.full((2, 256), -1, np.int32)])
    delta[S0, ord("a")] = S0 + 1      # X
    delta[S0 + 1, ord("a")] = S0 + 1  # D
    dfa = ByteDFA(delta, np.concatenate([base.accepting, [False, False]]), 0)
    assert not dfa.live[S0] and not dfa.live[S0 + 1]
    states = {"ordinary": 0, "accepting with an arc": _walk(dfa, b"ab"), "accepting, no arc": _walk(dfa, b"b"),
              "no mass": _walk(dfa, b"z"), "only arc to a dead end": S0, "minus one": -1, "out of range": dfa.n_states}
    rng = np.random.default_rng(33)
    arc = np.where(dfa.delta >= 0, rng.uniform(-2.0, 1.0, dfa.delta.shape), -np.inf).astype(np.float32)
    arc[0, ord("c")] = -np.inf  # (delta keeps the arc: the weight alone forbids it)
    fin = np.where(dfa.accepting, rng.uniform(-2.0, 1.0, dfa.n_states), -np.inf).astype(np.float32)
    weighted = types.SimpleNamespace(delta=dfa.delta, accepting=dfa.accepting, live=dfa.live, arc_logw=arc, final_logw=fin, start=0)
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(engine.device)
    wt = DeviceTables(eng=engine, delta=put(dfa.delta), accepting=put(dfa.accepting.astype(np.uint8)), live=put(dfa.live.astype(np.uint8)),
                      arc_logw=put(arc), final_logw=put(fin), start=0)
    free = ByteDFA(np.zeros((1, 256), np.int32), np.array([True]), 0)
    return {"dfa": (dfa, DeviceTables.upload(engine, dfa), states), "wfsa": (weighted, wt, states),
            "free": (free, DeviceTables.upload(engine, free), {"ordinary": 0, "minus one": -1, "out of range": 1})}


class Case:
    """A kernel case of tests/bytelm_ref.py on the device: group 0 has a candidate at the root, group 1 (G = 3) has none,
    group 2 (G = 3) has no live candidate at all.  `rows`: the restatement's unconstrained rows on the device's masses."""

    def __init__(self, engine, G, width, dtype, groups=None):
        self.engine, self.G, self.width = engine, G, width
        self.trie, self.host, self.tdev, node_of = _trie(engine)
        dev = engine.device
        case = R.kernel_case(R.kernel_seed(G, width, dtype), G, width, dtype)
        case["node"][0] = b""
        if G == 3:
            case["node"][width:2 * width] = [n or b"a" for n in case["node"][width:2 * width]]
        self.node_h, self.node, self.alive, self.u, self.w = _state(case, node_of, dev)
        self.alive_h, self.u_h, self.w_h = case["alive"], case["u"], case["w"]
        store = torch.from_numpy(case["logits"]).to(dev).to(DT[dtype])
        self.sel = engine.bytelm_children(self.tdev, self.node, self.alive, width)
        self.mass = self.trie.masses_from_logits(store, nodes=self.sel, wide_selections=True)
        self.tables = _tables(self.sel.cpu().numpy(), self.mass.cpu().numpy(), self.host["leaf_token"])
        self.rows = [R.next_row(self.cands(g), self.tables[g * width:(g + 1) * width], self.host["root"])[0] for g in range(G)]

    def cands(self, g):
        return _cands(self.node_h, self.alive_h, self.u_h, self.w_h, g * self.width, (g + 1) * self.width)

    def step(self, tables, state, ended=None, lw=None, cut=None, **kw):
        """glb_bytelm_step on copies of the state (`cut`: of one group's part); everything it wrote, on the host."""
        dev, G = self.engine.device, self.G if cut is None else 1
        f = (lambda t: t.clone()) if cut is None else (lambda t: t[cut * self.width:(cut + 1) * self.width].clone())
        t = dict(node=f(self.node), w=f(self.w), alive=f(self.alive), state=torch.tensor(state, dtype=torch.int32, device=dev),
                 ended=torch.tensor(ended if ended is not None else [0] * G, dtype=torch.int32, device=dev),
                 log_weight=torch.tensor(lw if lw is not None else [0.25] * G, dtype=torch.float32, device=dev),
                 logp=torch.full((G,), 0.5, dtype=torch.float32, device=dev), fresh=torch.zeros(G, dtype=torch.int32, device=dev))
        for k in ("byte", "uniform"):
            if kw.get(k) is not None:
                kw[k] = torch.tensor(kw[k], dtype=torch.int32 if k == "byte" else torch.float32, device=dev)
        out = self.engine.bytelm_step(self.tdev, t["node"], f(self.u), t["w"], t["alive"], f(self.sel), f(self.mass), self.width, tables,
                                      t["state"], t["ended"], t["log_weight"], t["logp"], fresh=t["fresh"], want_row=True, **kw)
        got = {k: v.cpu().numpy() for k, v in t.items()}
        got.update({k: v.cpu().numpy() for k, v in out.items() if v is not None})
        return got

    def check_group(self, got, g, automaton, state, byte, drawn, what, lw0=0.25, at=None):
        """Group g of `got` (at index `at` of its tensors) against the restatement: the row, log Zc, the byte, the advance."""
        at, width, root = g if at is None else at, self.width, self.host["root"]
        lo, hi = g * width, (g + 1) * width
        crow, logZc = CR.constrained_row(self.rows[g], automaton, state)
        lc = CR.lc_row(self.rows[g], automaton, state)
        _check_row(got["row"][at], crow, what)
        assert (got["logZc"][at] == NINF) if logZc == NINF else abs(got["logZc"][at] - logZc) <= TOL, what
        dead = logZc == NINF or (not drawn and lc[byte] == NINF)
        assert got["fresh"][at] == 1, what
        sl = slice(at * width, (at + 1) * width)
        if dead:
            assert got["state"][at] == -1 and got["ended"][at] == 0 and got["log_weight"][at] == NINF, what
            assert not got["alive"][sl].any() and (got["w"][sl][self.alive_h[lo:hi] != 0] == NINF).all(), what
            if drawn:
                assert got["byte"][at] == -1 and got["logp"][at] == 0.5, what
            return
        assert got["byte"][at] == byte, (what, got["byte"][at], byte)
        moved = R.advance_group(self.cands(g), self.tables[lo:hi], byte, root)
        assert got["alive"][sl].tolist() == [int(c is not None) for c in moved], what
        for s, c in enumerate(moved):
            if c is not None:
                assert got["node"][sl][s] == c["n"] and abs(got["w"][sl][s] - c["w"]) <= TOL, what
        assert got["state"][at] == (-1 if byte == 256 else int(automaton.delta[state, byte])), what
        assert got["ended"][at] == int(byte == 256), what
        assert abs(got["logp"][at] - (0.5 + self.rows[g][byte])) <= TOL, what
        own = lc[byte] - self.rows[g][byte]
        assert abs(got["log_weight"][at] - (lw0 + (logZc if drawn else own))) <= TOL, what

    def midpoint(self, automaton, state, g, rng):
        """(uniform, column): the midpoint of the CDF interval of a column of probability 1e-3 and more, chosen by `rng`."""
        crow, logZc = CR.constrained_row(self.rows[g], automaton, state)
        if logZc == NINF:
            return 0.5, -1
        cols = np.nonzero(crow >= math.log(1e-3))[0]
        c = int(cols[rng.integers(len(cols))])
        u = CR.cdf(crow)[c] - math.exp(crow[c]) / 2
        assert CR.pick(crow, u) == c
        return float(u), c


CASES = [(G, width, dtype) for G in (1, 3) for width in (1, 5, 64) for dtype in ("float32", "bfloat16")]


@pytest.mark.parametrize("G,width,dtype", CASES)
def test_the_kernel_against_the_restatement_on_the_device_masses(engine, G, width, dtype):
    case, rng = Case(engine, G, width, dtype), np.random.default_rng(G * 100 + width)
    seen = set()
    for name, (automaton, tables, states) in _automata(engine).items():
        for scenario, state in states.items():
            picks = [case.midpoint(automaton, state, g, rng) for g in range(G)]
            got = case.step(tables, [state] * G, uniform=[u for u, _ in picks])
            assert not any(np.isnan(got[k]).any() for k in ("row", "logZc", "log_weight", "logp", "w")), (name, scenario)
            for g in range(G):
                case.check_group(got, g, automaton, state, picks[g][1], True, (name, scenario, G, width, dtype, g))
            row0, dead0 = got["row"][0], got["state"][0] == -1 and got["ended"][0] == 0
            # what each scenario is there for, on group 0 (a candidate at the root) and group 1 (none there)
            if scenario == "ordinary":
                assert np.isfinite(got["logZc"][0]) and got["byte"][0] >= 0
                if name != "free":
                    assert row0[ord("z")] == NINF  # (allowed, without mass)
                if name == "wfsa":
                    assert row0[ord("c")] == NINF and np.isfinite(case.rows[0][ord("c")])  # the arc of weight -inf
            if scenario.startswith("accepting"):
                assert np.isfinite(row0[256]), "EOS allowed and finite for a group with a candidate at the root"
                if G == 3:
                    assert got["row"][1][256] == NINF, "EOS without mass: no candidate at the root"
                    if scenario == "accepting, no arc":
                        assert got["state"][1] == -1 and got["log_weight"][1] == NINF and got["byte"][1] == -1
            if scenario == "accepting, no arc":
                assert got["byte"][0] == 256 and got["ended"][0] == 1 and got["state"][0] == -1 and np.isfinite(got["log_weight"][0])
            if scenario in ("no mass", "only arc to a dead end", "minus one", "out of range"):
                assert dead0 and got["logZc"][0] == NINF and (row0 == NINF).all() and got["byte"][0] == -1
                assert got["log_weight"][0] == NINF and not got["alive"].any()
            if G == 3:  # the group without a live candidate dies under every automaton
                assert got["state"][2] == -1 and got["log_weight"][2] == NINF and (got["row"][2] == NINF).all()
            seen.add(scenario)
        # an ended group is skipped: nothing of it is written, its weight is kept bit for bit
        lw = [float(np.float32(-3.7 - g)) for g in range(G)]
        got = case.step(tables, [-1] * G, ended=[1] * G, lw=lw, uniform=[0.5] * G)
        assert got["log_weight"].tobytes() == np.array(lw, np.float32).tobytes() and (got["ended"] == 1).all() and (got["state"] == -1).all()
        assert np.array_equal(got["node"], case.node_h) and np.array_equal(got["alive"], case.alive_h) and (got["logp"] == 0.5).all()
        assert got["w"].tobytes() == case.w_h.tobytes() and (got["fresh"] == 0).all()
        assert (got["byte"] == -1).all() and (got["row"] == NINF).all() and (got["logZc"] == NINF).all()
    assert seen == {"ordinary", "accepting with an arc", "accepting, no arc", "no mass", "only arc to a dead end", "minus one", "out of range"}


@pytest.mark.parametrize("name", ["dfa", "wfsa"])
def test_a_given_byte_allowed_forbidden_and_minus_one(engine, name):
    case = Case(engine, 3, 5, "float32")
    automaton, tables, _ = _automata(engine)[name]
    # group 0 reads an allowed byte, group 1 a forbidden one, group 2 is left alone
    got = case.step(tables, [0, 0, 0], byte=[ord("a"), ord("c") if name == "wfsa" else ord("q"), -1])
    case.check_group(got, 0, automaton, 0, ord("a"), False, (name, "allowed"))
    case.check_group(got, 1, automaton, 0, ord("c") if name == "wfsa" else ord("q"), False, (name, "forbidden"))
    assert got["state"][0] == int(automaton.delta[0, ord("a")]) and np.isfinite(got["log_weight"][0])
    if name == "dfa":
        assert got["log_weight"][0] == 0.25  # an allowed byte of a ByteDFA weighs nothing
    assert got["state"][1] == -1 and got["log_weight"][1] == NINF and not got["alive"][5:10].any() and not np.isnan(got["logp"]).any()
    lo = 2 * case.width
    assert got["state"][2] == 0 and got["log_weight"][2] == 0.25 and got["logp"][2] == 0.5 and got["fresh"][2] == 0
    assert np.array_equal(got["node"][lo:], case.node_h[lo:]) and np.array_equal(got["alive"][lo:], case.alive_h[lo:])
    # EOS given at an accepting state ends the group; at the start state it is forbidden
    acc = _walk(automaton, b"ab")
    got = case.step(tables, [acc, 0, 0], byte=[256, 256, -1])
    case.check_group(got, 0, automaton, acc, 256, False, (name, "EOS"))
    case.check_group(got, 1, automaton, 0, 256, False, (name, "EOS forbidden"))
    assert got["ended"].tolist() == [1, 0, 0] and got["state"].tolist() == [-1, -1, 0]


@pytest.mark.parametrize("width,dtype", [(1, "float32"), (5, "bfloat16"), (64, "float32")])
def test_the_automaton_that_allows_everything_is_the_plain_advance(engine, width, dtype):
    case = Case(engine, 3, width, dtype)
    _, tables, _ = _automata(engine)["free"]
    eng, dev = engine, engine.device
    rows, _ = eng.bytelm_next(case.tdev, case.node, case.u, case.w, case.alive, case.sel, case.mass, width)
    byte = [int(np.argmax(case.rows[0][:256])), 256, ord("b")]
    got = case.step(tables, [0, 0, 0], byte=byte)
    node, w, alive = case.node.clone(), case.w.clone(), case.alive.clone()
    logp, fresh = torch.full((3,), 0.5, device=dev), torch.zeros(3, dtype=torch.int32, device=dev)
    eng.bytelm_next(case.tdev, node, case.u, w, alive, case.sel, case.mass, width, byte=torch.tensor(byte, dtype=torch.int32, device=dev),
                    logp=logp, fresh=fresh)
    for k, t in (("node", node), ("w", w), ("alive", alive), ("fresh", fresh), ("logp", logp)):
        assert got[k].tobytes() == t.cpu().numpy().tobytes(), k
    plain = rows.cpu().numpy()
    live = np.isfinite(got["logZc"])
    assert live[:2].all() and np.abs(got["logZc"][live]).max() <= 1e-5
    assert ((got["row"] == NINF) == (plain == NINF)).all()
    fin = np.isfinite(plain)
    assert np.abs(got["row"][fin] - plain[fin]).max() <= 1e-5


def test_a_group_is_the_same_bytes_alone_and_in_a_batch(engine):
    case = Case(engine, 3, 5, "float32")
    for name, (automaton, tables, states) in _automata(engine).items():
        state = [states["ordinary"], states.get("accepting with an arc", 0), 0]
        for kw in (dict(uniform=[0.3, 0.6, 0.9]), dict(byte=[ord("a"), ord("c"), ord("b")]), dict(seed=7, offset=3)):
            whole = case.step(tables, state, **kw)
            for g in (0, 1):
                one = {k: ([v[g]] if isinstance(v, list) else v) for k, v in kw.items()}
                if "seed" in kw and g != 0:
                    continue  # (the Philox counter holds the group's index: only group 0 keeps its draw alone)
                alone = case.step(tables, [state[g]], cut=g, **one)
                for k in ("row", "logZc", "byte", "state", "ended", "log_weight", "logp", "fresh"):
                    assert whole[k][g:g + 1].tobytes() == alone[k].tobytes(), (name, kw, g, k)
                for k in ("node", "w", "alive"):
                    assert whole[k][g * 5:(g + 1) * 5].tobytes() == alone[k].tobytes(), (name, kw, g, k)


def test_philox_draws_follow_the_row_and_are_reproducible_on_the_host(engine):
    from tests.importance_ref import philox_pair

    trie, host, tdev, node_of = _trie(engine)
    dev, n = engine.device, 4096
    automaton, tables, _ = _automata(engine)["dfa"]
    logits = (0.5 * np.random.default_rng(2033).standard_normal((1, len(R.kernel_vocab()[0])))).astype(np.float32)  # (a flat row:
    store = torch.from_numpy(logits).to(dev)                                   # each of a, b, c keeps a good share of the draws)
    node = torch.full((n,), host["root"], dtype=torch.int32, device=dev)
    alive, u = torch.ones(n, dtype=torch.int32, device=dev), torch.zeros(n, device=dev)
    sel = engine.bytelm_children(tdev, node, alive, 1)
    mass = trie.masses_from_logits(store, nodes=sel[:1].contiguous(), wide_selections=True).expand(n, -1).contiguous()  # (one state, 4096 times)
    tab = _tables(sel[:1].cpu().numpy(), mass[:1].cpu().numpy(), host["leaf_token"])
    row = R.next_row([dict(x=(), n=host["root"], u=0.0, w=0.0)], tab, host["root"])[0]
    crow, _ = CR.constrained_row(row, automaton, 0)

    def draw(seed, offset):
        i32 = lambda v: torch.full((n,), v, dtype=torch.int32, device=dev)
        out = engine.bytelm_step(tdev, node.clone(), u, u.clone(), alive.clone(), sel, mass, 1, tables, i32(0), i32(0), u.clone(), u.clone(),
                                 seed=seed, offset=offset)
        return out["byte"].cpu().numpy()

    got = draw(2033, 5)
    p = np.where(crow > NINF, np.exp(crow), 0.0)
    assert (p > 0.1).sum() >= 3, "the state must leave several bytes likely, or equal draws show nothing"
    freq = np.bincount(got, minlength=257)[:257] / n
    assert (got >= 0).all() and (got <= 256).all()
    bound = 6 * np.sqrt(p * (1 - p) / n) + 1 / n
    print("largest frequency error over its bound", (np.abs(freq - p) / bound).max())
    assert (np.abs(freq - p) <= bound).all()
    assert np.array_equal(draw(2033, 5), got) and not np.array_equal(draw(2033, 6), got)
    # the documented counter and key: {g, 0, offset, 0} and {seed, 0}; the float is the 24 high bits of word 0
    cum, checked = CR.cdf(crow), 0
    for g in range(n):
        uni = ((philox_pair(2033, 5, g)[0] & 0xFFFFFFFF) >> 8) * 2.0 ** -24
        if np.abs(cum[crow > NINF] - uni).min() >= 1e-5:
            assert got[g] == CR.pick(crow, uni), g
            checked += 1
    assert checked > n * 0.99


# ---- end to end over a tiny GPT-2 -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(engine):
    from tests.test_wfsa_gpu import _model

    return _model(engine, 257)


@pytest.fixture(scope="module")
def host_lm(model):
    from tests.test_beam_gpu import _rows

    cache = {}

    def lm(x):
        if tuple(x) not in cache:
            cache[tuple(x)] = np.exp(_rows(model, [[0] + list(x)])[0])
        return cache[tuple(x)]

    return lm


def test_end_to_end_under_a_regex_against_the_restatement_on_the_model_rows(model, host_lm):
    from genlm_backend_amd import ByteBeam, ByteDFA

    vocab, texts = R.vocab257(), [b"abcabc", b"hggf"]
    dfa = ByteDFA.from_regex(rb"(abc)+|hg*f?")
    beam = ByteBeam(model, vocab, [0], width=64, n=2, prompt_ids=[0], max_bytes=16, constraint=dfa)
    refs = [CR.RefConstrainedBeam(host_lm, vocab, [0], 64, dfa) for _ in texts]
    for i in range(7):
        rows = beam.next_byte_logprobs()
        assert rows.shape == (2, 257) and rows.dtype == torch.float32 and rows is beam.next_byte_logprobs()
        got, logZ, lw = rows.cpu().numpy(), beam.next_byte_logZ().cpu().numpy(), beam.log_weights.cpu().numpy()
        for g, ref in enumerate(refs):
            want, wz = ref.next_byte_logprobs(), ref.next_byte_logZ()
            assert not ref.pruned
            assert ((got[g] == NINF) == (want == NINF)).all(), (i, g)  # forbidden columns, exactly
            fin = want > NINF
            err = np.abs(got[g][fin] - want[fin]).max()
            print("bytes", i, "group", g, "row error", err, "logZc error", abs(logZ[g] - wz), "weight error", abs(lw[g] - ref.log_weight))
            assert err <= GAP and abs(logZ[g] - wz) <= GAP and abs(lw[g] - ref.log_weight) <= GAP
            assert abs(float(torch.logsumexp(rows[g], 0))) <= 1e-5 and abs(float(beam.logp[g]) - ref.logp) <= GAP
        if i < 6:
            byte = [t[i] if i < len(t) else -1 for t in texts]
            beam.advance(byte)
            for ref, b in zip(refs, byte):
                ref.advance(b)
    assert beam.state.cpu().tolist() == [_walk(dfa, t) for t in texts] and beam.ended.cpu().tolist() == [0, 0]
    # drawn texts stay inside the language's prefixes; EOS only from an accepting state
    beam.reset()
    assert beam.log_weights.cpu().tolist() == [0.0, 0.0] and beam.state.cpu().tolist() == [dfa.start] * 2
    for text, ended in zip(beam.generate(max_bytes=12, seed=4), beam.ended.cpu().tolist()):
        s = dfa.start
        for b in text:
            s = int(dfa.delta[s, b])
            assert s >= 0 and dfa.live[s], text
        assert not ended or dfa.accepts(text)
    beam.reset()
    greedy = beam.generate(max_bytes=5, greedy=True)
    assert all(_walk(dfa, t) >= 0 for t in greedy)
    # a forbidden byte kills the group quietly
    beam.reset()
    beam.advance([ord("a"), ord("b")])
    assert beam.state.cpu().tolist()[1] == -1 and beam.log_weights.cpu().tolist()[1] == NINF and beam.log_weights.cpu().tolist()[0] == 0.0
    assert bool((beam.next_byte_logprobs()[1] == NINF).all()) and not bool(torch.isnan(beam.next_byte_logprobs()).any())
    with pytest.raises(ValueError, match="this beam has none"):
        ByteBeam(model, vocab, [0], width=4, prompt_ids=[0]).step()


# A text of k bytes has 1, 2, 4, 8 candidates after 0, 1, 2, 3 bytes over this vocabulary (every split into tokens of 1 to 3
# letters, each with or without an open token), so width = 4 holds every candidate of a text of two bytes: only then is the
# beam's logp the exact marginal that a beam of width 64 reports.  LONG has texts of three bytes: width 4 prunes there and logp
# is a sum of row entries normalised over the candidates kept - the restatement's at the same width; it misses the wide beam's
# on either side (measured on the MI355X: -11.0786 against -11.0775 for b"dea", -15.7922 against -15.7940 for b"hgf", up to
# 3.0e-3 over the lexicon), so there logp is compared with the restatement at width 4.
LEXICON = {b"ab": -0.5, b"a": 0.25, b"hg": -1.0, b"de": 0.5}
LONG = {b"abc": -0.5, b"ab": 0.25, b"hgf": -1.0, b"dea": 0.5}


@pytest.mark.parametrize("lexicon", [LEXICON, LONG], ids=["two bytes", "three bytes"])
def test_byte_sis_over_a_weighted_lexicon(model, host_lm, lexicon):
    from genlm_backend_amd import ByteBeam, ByteSIS, ByteWFSA

    LEXICON = lexicon
    vocab, wfsa = R.vocab257(), ByteWFSA.from_weighted_strings(LEXICON)
    sis = ByteSIS(model, 64, wfsa, vocab, [0], width=4, prompt_ids=[0], max_bytes=8, seed=11)
    texts, lw, finished = sis.run().results()
    lw_h, logp = lw.cpu().numpy(), sis.logp.cpu().numpy()
    assert bool(finished.all()) and all(t in LEXICON for t in texts) and len(set(texts)) > 1 and np.isfinite(lw_h).all()
    assert torch.equal(lw, sis.log_weights) and sis.bytes.shape == (64, 8) and sis.t <= 8
    want_lw, want_logp = {}, {}
    for text in set(texts):
        ref = CR.RefConstrainedBeam(host_lm, vocab, [0], 4, wfsa)
        total = 0.0
        for b in list(text) + [256]:
            total += ref.next_byte_logZ()
            ref.advance(b)
        want_lw[text], narrow = total, ref.logp
        plain = ByteBeam(model, vocab, [0], width=64, n=1, prompt_ids=[0], max_bytes=8)
        plain.prefill([text])
        plain.advance([256])
        want_logp[text] = float(plain.logp[0])
        if lexicon is LONG:  # (pruned: the restatement's logp at width 4)
            print(text, "logp at width 64", want_logp[text], "at width 4", narrow, "pruned", ref.pruned)
            want_logp[text] = narrow
        else:
            assert not ref.pruned
    worst_w = max(abs(lw_h[i] - want_lw[t]) for i, t in enumerate(texts))
    worst_p = max(abs(logp[i] - want_logp[t]) for i, t in enumerate(texts))
    print("largest weight error", worst_w, "largest logp error", worst_p)
    assert worst_w <= GAP and worst_p <= GAP
    ev = float(sis.log_evidence())
    assert abs(ev - (math.log(np.exp(lw_h.astype(np.float64)).sum()) - math.log(64))) <= 1e-4
    again = ByteSIS(model, 64, wfsa, vocab, [0], width=4, prompt_ids=[0], max_bytes=8, seed=11).run().results()[0]
    assert again == texts
    # max_bytes too short for any string of the language: nobody finishes, every returned weight is -inf, the raw ones are kept
    short = ByteSIS(model, 8, ByteWFSA.from_weighted_strings(LONG), vocab, [0], width=4, prompt_ids=[0], max_bytes=2, seed=11).run()
    _, lw2, fin2 = short.results()
    assert not bool(fin2.any()) and bool((lw2 == NINF).all()) and bool(torch.isfinite(short.log_weights).all())
    assert float(short.log_evidence()) == NINF


def test_byte_sis_resampling_gathers_every_particle_by_its_ancestor(model):
    from genlm_backend_amd import ByteDFA, ByteSIS

    vocab, dfa = R.vocab257(), ByteDFA.from_regex(rb"(abc)+|hg*f?|[a-h]{2,6}")
    sis = ByteSIS(model, 8, dfa, vocab, [0], width=4, prompt_ids=[0], max_bytes=8, seed=5)
    for _ in range(3):
        sis.step()
    anc = [1, 1, 0, 3, 7, 7, 2, 5]
    b = sis.beam
    before = {k: getattr(b, k).cpu().numpy().copy() for k in ("state", "ended", "logp", "log_weights")}
    rows, drawn = b.next_byte_logprobs().cpu().numpy().copy(), sis.bytes.cpu().numpy().copy()
    cands = [b.candidates(g) for g in range(8)]
    sis._resample(anc)
    assert b.next_byte_logprobs().cpu().numpy().tobytes() == rows[anc].tobytes()
    assert sis.bytes.cpu().numpy().tobytes() == drawn[anc].tobytes()
    for k in ("state", "ended", "logp"):
        assert getattr(b, k).cpu().numpy().tobytes() == before[k][anc].tobytes(), k
    assert [b.candidates(g) for g in range(8)] == [cands[a] for a in anc]
    mean = math.log(np.exp(before["log_weights"].astype(np.float64)).mean())
    assert np.abs(b.log_weights.cpu().numpy() - mean).max() <= 1e-5 and sis.n_resamples == 1
    full = ByteSIS(model, 16, dfa, vocab, [0], width=4, prompt_ids=[0], max_bytes=8, seed=6, resample_ess=1.0).run()
    texts, lw, finished = full.results()
    lw = lw.cpu().numpy()
    print("resamplings", full.n_resamples, "finished", int(finished.sum()))
    assert not np.isnan(lw).any() and (np.isfinite(lw) | (lw == NINF)).all() and not np.isnan(full.log_weights.cpu().numpy()).any()
    assert all(dfa.accepts(t) for t, f in zip(texts, finished.cpu().tolist()) if f)
