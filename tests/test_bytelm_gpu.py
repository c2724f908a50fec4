"""The byte-level beam on the GPU (glb_bytelm_children / _extend / _next, `ByteBeam`) against the float64
restatement tests/bytelm_ref.py.

The kernel tests hand the restatement the DEVICE's masses (`TokenByteTrie.masses_from_logits` of the same rows), so ids,
parents, tokens and slots are compared exactly and only the float32 arithmetic of the three kernels is under a tolerance:
1e-5 absolute on a log-probability of 1e-6 and more (a handful of float32 operations on numbers below 14 in magnitude).  A
pruning case may be skipped only where the deciding weights lie within 1e-5 of each other on the device's masses; the seeds
(tests/bytelm_ref.py `SEEDS`) keep them 1e-3 apart on float64 masses of the same rows (tests/test_bytelm_cpu.py), so none is
expected to.  The end-to-end test feeds the restatement the model's own log-probability rows and allows GAP = 1e-3, the bar
of tests/test_beam_gpu.py for sums of a handful of float32 log-probabilities."""
import math

import numpy as np
import pytest
import torch

from tests import bytelm_ref as R

pytestmark = pytest.mark.gpu

GAP = 1e-3    # tests/test_beam_gpu.py
TOL = 1e-5    # the kernels' float32 arithmetic on the same masses
P_MIN = 1e-6  # rows are compared where the probability is at least this
TIE = 1e-5    # a pruning case whose deciding weights are closer than this on the device's masses is skipped
DT = {"float32": torch.float32, "bfloat16": torch.bfloat16}


def _trie(engine):
    from genlm_backend_amd.bytelm import byte_trie, byte_trie_arrays

    vocab, eos = R.kernel_vocab()
    trie = byte_trie(vocab, eos, engine=engine)
    host = byte_trie_arrays(trie)
    dev = {k: (torch.from_numpy(v).to(engine.device) if isinstance(v, np.ndarray) else v) for k, v in host.items()}
    node_of = {bytes(trie.node2prefix[n]): n for n, kids in enumerate(trie.children) if kids}
    return trie, host, dev, node_of


def _tables(sel, mass, leaf_token):
    """tests/bytelm_ref.py's tables of every slot from the device's selection and mass rows."""
    out = []
    for srow, mrow in zip(sel, mass):
        out.append(({b: (int(srow[b]), float(mrow[b])) for b in range(256) if srow[b] >= 0},
                    [(int(leaf_token[srow[256 + j]]), float(mrow[256 + j])) for j in range(4) if srow[256 + j] >= 0]))
    return out


def _state(case, node_of, dev):
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    node = np.array([node_of[p] for p in case["node"]], np.int32)
    return node, t(node, np.int32), t(case["alive"], np.int32), t(case["u"], np.float32), t(case["w"], np.float32)


def _cands(node, alive, u, w, lo, hi):
    return [dict(x=(), n=int(node[s]), u=float(u[s]), w=float(w[s])) if alive[s] else None for s in range(lo, hi)]


def _check_row(got, want, what):
    assert not np.isnan(got).any(), what
    assert ((got == -np.inf) == (want == -np.inf)).all(), what
    sure = want >= math.log(P_MIN)
    err = np.abs(got[sure] - want[sure]).max() if sure.any() else 0.0
    print(what, "row error", err)
    assert err <= TOL, (what, err)


def _run_case(engine, G, width, dtype):
    """Returns False when the case had to be skipped (a near tie on the device's masses)."""
    from genlm_backend_amd.bytelm import children_table

    trie, host, tdev, node_of = _trie(engine)
    dev, root = engine.device, host["root"]
    case = R.kernel_case(R.kernel_seed(G, width, dtype), G, width, dtype)
    node_h, node, alive, u, w = _state(case, node_of, dev)
    store = torch.from_numpy(case["logits"]).to(dev).to(DT[dtype])
    N = G * width

    # ---- children: the host table, -1 rows for dead slots
    sel = engine.bytelm_children(tdev, node, alive, width)
    want_sel = children_table(trie, node_h)
    want_sel[case["alive"] == 0] = -1
    assert np.array_equal(sel.cpu().numpy(), want_sel)
    mass = trie.masses_from_logits(store, nodes=sel)
    assert mass.shape == (N, 260)

    # ---- extend: parents, tokens and slots exact on the device's own masses
    fresh = torch.ones(G, dtype=torch.int32, device=dev)
    out = engine.bytelm_extend(tdev, node, u, w, alive, sel, mass, width, fresh=fresh)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert fresh.cpu().tolist() == [0] * G
    tables = _tables(want_sel, mass.cpu().numpy(), host["leaf_token"])
    new_cands, spawned = [], []
    for g in range(G):
        lo, hi = g * width, (g + 1) * width
        new, parent, token, gap, _ = R.extend_group(_cands(node_h, case["alive"], case["u"], case["w"], lo, hi), tables[lo:hi], width, root)
        print((G, width, dtype), "group", g, "gap", gap)
        if gap < TIE:
            return False
        assert got["parent"][lo:hi].tolist() == [p + lo if p >= 0 else -1 for p in parent], g
        assert got["token"][lo:hi].tolist() == token, g
        assert got["alive"][lo:hi].tolist() == [int(c is not None) for c in new], g
        for s, c in enumerate(new, start=lo):
            if c is None:
                assert got["u"][s] == -np.inf and got["w"][s] == -np.inf and got["node"][s] == root
            else:
                assert got["node"][s] == c["n"] and abs(got["u"][s] - c["u"]) <= TOL and abs(got["w"][s] - c["w"]) <= TOL
                if token[s - lo] < 0:  # a kept candidate is the old one, bit for bit
                    assert got["u"][s] == case["u"][s] and got["w"][s] == case["w"][s]
        spawned += [s + lo for s in range(width) if token[s] >= 0]
        new_cands.append(new)
    assert int(got["n_spawned"][0]) == len(spawned) and got["spawned"].tolist() == spawned + [-1] * (N - len(spawned))
    # an unmoved group offers nothing and keeps every candidate
    again = engine.bytelm_extend(tdev, out["node"], out["u"], out["w"], out["alive"], sel, mass, width, fresh=fresh)
    assert int(again["n_spawned"].item()) == 0 and torch.equal(again["alive"], out["alive"]) and torch.equal(again["w"], out["w"])

    # ---- next: the rows on the masses of the new state
    sel2 = engine.bytelm_children(tdev, out["node"], out["alive"], width)
    mass2 = trie.masses_from_logits(store, nodes=sel2, wide_selections=True)
    rows, logZ = engine.bytelm_next(tdev, out["node"], out["u"], out["w"], out["alive"], sel2, mass2, width)
    rows, logZ = rows.cpu().numpy(), logZ.cpu().numpy()
    tables2 = _tables(sel2.cpu().numpy(), mass2.cpu().numpy(), host["leaf_token"])
    dev_cands = lambda g: _cands(got["node"], got["alive"], got["u"], got["w"], g * width, (g + 1) * width)
    want_rows = []
    for g in range(G):
        want, wz = R.next_row(dev_cands(g), tables2[g * width:(g + 1) * width], root)
        _check_row(rows[g], want, ("next", G, width, dtype, g))
        assert (logZ[g] == -np.inf) if wz == -np.inf else abs(logZ[g] - wz) <= TOL
        want_rows.append(want)
    if G == 3:  # the group without a live candidate
        assert (rows[2] == -np.inf).all() and logZ[2] == -np.inf

    # ---- advance: group 0 by its most probable byte, group 1 by a byte nothing spells, group 2 left alone
    best = int(np.argmax(want_rows[0][:256]))
    byte = [best, ord("z"), -1][:G]
    logp = torch.full((G,), 0.5, dtype=torch.float32, device=dev)
    node3, w3, alive3 = out["node"].clone(), out["w"].clone(), out["alive"].clone()
    engine.bytelm_next(tdev, node3, out["u"], w3, alive3, sel2, mass2, width, byte=torch.tensor(byte, dtype=torch.int32, device=dev),
                       logp=logp, fresh=fresh)
    assert fresh.cpu().tolist() == [1, 1, 0][:G]
    n3, a3, ww3, lp = node3.cpu().numpy(), alive3.cpu().numpy(), w3.cpu().numpy(), logp.cpu().numpy()
    for g in range(G):
        lo, hi = g * width, (g + 1) * width
        if byte[g] < 0:
            assert np.array_equal(n3[lo:hi], got["node"][lo:hi]) and np.array_equal(a3[lo:hi], got["alive"][lo:hi]) and lp[g] == 0.5
            continue
        moved = R.advance_group(dev_cands(g), tables2[lo:hi], byte[g], root)
        assert a3[lo:hi].tolist() == [int(c is not None) for c in moved], g
        for s, c in enumerate(moved, start=lo):
            if c is not None:
                assert n3[s] == c["n"] and abs(ww3[s] - c["w"]) <= TOL
            elif got["alive"][s]:
                assert ww3[s] == -np.inf
        want_lp = 0.5 + want_rows[g][byte[g]]
        assert (lp[g] == -np.inf) if want_lp == -np.inf else abs(lp[g] - want_lp) <= TOL, (g, lp[g], want_lp)
    assert not np.isnan(lp).any()
    if G == 3:  # the group that read a byte nothing spells: dead, a row of -inf, no NaN
        assert lp[1] == -np.inf and not a3[width:2 * width].any()
    sel3 = engine.bytelm_children(tdev, node3, alive3, width)
    mass3 = trie.masses_from_logits(store, nodes=sel3)
    rows3, logZ3 = engine.bytelm_next(tdev, node3, out["u"], w3, alive3, sel3, mass3, width)
    assert not torch.isnan(rows3).any() and not torch.isnan(logZ3).any()
    if G == 3:
        assert bool((rows3[1:] == -np.inf).all()) and bool((logZ3[1:] == -np.inf).all())
    # EOS ends a group
    engine.bytelm_next(tdev, node3, out["u"], w3, alive3, sel3, mass3, width, byte=torch.full((G,), 256, dtype=torch.int32, device=dev),
                       logp=logp, fresh=fresh)
    assert not alive3.any() and not torch.isnan(logp).any()
    return True


def test_kernels_against_the_restatement_on_the_device_masses(engine):
    done = [_run_case(engine, G, width, dtype) for G, width, dtype in R.KERNEL_CASES]
    skipped = done.count(False)
    print("skipped", skipped, "of", len(done))
    assert skipped <= len(done) // 10


def test_a_group_is_the_same_bytes_alone_and_in_a_batch(engine):
    trie, host, tdev, node_of = _trie(engine)
    dev, width = engine.device, 5
    case = R.kernel_case(R.kernel_seed(3, width, "float32"), 3, width, "float32")
    case["alive"][2 * width:] = 1  # (all three groups live here)
    case["u"][2 * width:] = case["w"][2 * width:] = -1.0
    _, node, alive, u, w = _state(case, node_of, dev)
    store = torch.from_numpy(case["logits"]).to(dev)
    sel = engine.bytelm_children(tdev, node, alive, width)
    mass = trie.masses_from_logits(store, nodes=sel)
    cut = lambda t: t[width:2 * width].contiguous()
    assert torch.equal(cut(sel), engine.bytelm_children(tdev, cut(node), cut(alive), width))
    whole = engine.bytelm_extend(tdev, node, u, w, alive, sel, mass, width)
    alone = engine.bytelm_extend(tdev, cut(node), cut(u), cut(w), cut(alive), cut(sel), cut(mass), width)
    same = lambda a, b: a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    for k in ("token", "node", "alive", "u", "w"):
        assert same(cut(whole[k]), alone[k]), k
    assert same(torch.where(cut(whole["parent"]) >= 0, cut(whole["parent"]) - width, cut(whole["parent"])), alone["parent"])
    sel2 = engine.bytelm_children(tdev, whole["node"], whole["alive"], width)
    mass2 = trie.masses_from_logits(store, nodes=sel2, wide_selections=True)
    args = lambda f: [f(whole[k]) for k in ("node", "u", "w", "alive")] + [f(sel2), f(mass2)]
    rows, logZ = engine.bytelm_next(tdev, *args(lambda t: t), width)
    rows1, logZ1 = engine.bytelm_next(tdev, *args(cut), width)
    assert same(rows[1:2], rows1) and same(logZ[1:2], logZ1) and bool(torch.isfinite(logZ1).all())
    best = int(rows1[0, :256].argmax())
    lp3, lp1 = torch.zeros(3, device=dev), torch.zeros(1, device=dev)
    a3, a1 = [t.clone() for t in args(lambda t: t)], [t.clone() for t in args(cut)]
    engine.bytelm_next(tdev, *a3, width, byte=torch.tensor([ord("a"), best, ord("b")], dtype=torch.int32, device=dev), logp=lp3)
    engine.bytelm_next(tdev, *a1, width, byte=torch.tensor([best], dtype=torch.int32, device=dev), logp=lp1)
    for x, y in zip(a3, a1):
        assert same(cut(x), y)
    assert same(lp3[1:2], lp1)


# ---- end to end over a tiny GPT-2 -------------------------------------------------------------------------------------------------
PREFIXES = [b"abcabc", b"hgfeda"]


@pytest.fixture(scope="module")
def model(engine):
    from tests.test_wfsa_gpu import _model

    return _model(engine, 257)


@pytest.fixture(scope="module")
def host_lm(model):
    from tests.test_beam_gpu import _rows

    def lm(x):
        return np.exp(_rows(model, [[0] + list(x)])[0])

    return lm


def test_end_to_end_against_the_restatement_on_the_model_rows(model, host_lm):
    from genlm_backend_amd import ByteBeam

    vocab = R.vocab257()
    beam = ByteBeam(model, vocab, [0], width=64, n=2, prompt_ids=[0], max_bytes=16)
    refs = [R.RefBeam(host_lm, vocab, [0], 64) for _ in PREFIXES]
    seen = []
    for i in range(7):  # the rows after 0 .. 6 bytes
        rows = beam.next_byte_logprobs()
        assert rows.shape == (2, 257) and rows.dtype == torch.float32 and rows is beam.next_byte_logprobs()
        got, lp = rows.cpu().numpy(), beam.logp.cpu().numpy()
        seen.append(got.copy())
        for g, ref in enumerate(refs):
            want = ref.next_byte_logprobs()
            sure = want >= math.log(P_MIN)
            err = np.abs(got[g][sure] - want[sure]).max()
            print("bytes", i, "group", g, "row error", err, "logp error", abs(lp[g] - ref.logp), "candidates", len(ref.live()))
            assert not ref.pruned and err <= GAP and abs(lp[g] - ref.logp) <= GAP
            assert not np.isnan(got[g]).any() and (got[g][~sure] < math.log(P_MIN) + GAP).all()
            assert abs(float(torch.logsumexp(rows[g], 0))) <= 1e-5
        if i < 6:
            beam.advance([p[i] for p in PREFIXES])
            for ref, p in zip(refs, PREFIXES):
                ref.advance(p[i])
    for g, ref in enumerate(refs):  # the candidates are the restatement's: the same tokenisations at the same nodes
        got = sorted((tuple(t), n) for t, n, _, _ in beam.candidates(g))
        assert got == sorted((c["x"], c["n"]) for c in ref.live())
    first = beam.generate(max_bytes=6, seed=0)
    # reset(), then the same bytes: the same rows (to 1e-5: the contexts are now served from warm KV rows, another path through
    # the same float32 model), and the same draws
    beam.reset()
    assert beam.logp.cpu().tolist() == [0.0, 0.0]
    for i in range(7):
        again = beam.next_byte_logprobs().cpu().numpy()
        finite = np.isfinite(seen[i])
        assert (np.isfinite(again) == finite).all() and np.abs(again[finite] - seen[i][finite]).max() <= 1e-5
        if i < 6:
            beam.advance(torch.tensor([p[i] for p in PREFIXES], dtype=torch.int32, device=model.device))
    assert beam.generate(max_bytes=6, seed=0) == first and all(len(t) <= 6 for t in first)
    beam.reset()
    beam.prefill(PREFIXES)
    greedy = beam.generate(max_bytes=4, greedy=True)
    assert all(isinstance(t, bytes) and len(t) <= 4 for t in greedy)


def test_candidates_inside_a_token_cost_no_forward(model):
    from genlm_backend_amd import ByteBeam

    width, text = 64, PREFIXES[0]
    beam = ByteBeam(model, R.vocab257(), [0], width=width, n=1, prompt_ids=[0], max_bytes=16)
    counted, inner = [], model._batch_step

    def counting(tok_d, st_d, ln_d, n, *args, **kw):
        counted.append(n)
        return inner(tok_d, st_d, ln_d, n, *args, **kw)

    model._batch_step = counting
    try:
        beam.prefill([text])
        beam.next_byte_logprobs()
    finally:
        del model._batch_step
    print("forwarded contexts", sum(counted), "in", len(counted), "calls")
    assert sum(counted) == beam.forwarded and 1 < sum(counted) < width * len(text)
    # a context is forwarded when a candidate commits a token, once: at least the live candidates' distinct contexts
    assert sum(counted) >= len({tuple(toks) for toks, _, _, _ in beam.candidates(0)})
