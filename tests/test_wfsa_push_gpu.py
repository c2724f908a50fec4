"""Weight pushing on the GPU (glb_dfa_backward / glb_dfa_push_weights, DeviceConstraint(push=...), DeviceSIS and
batch_next_token_step_device under a pushed constraint).  Under "max" everything is compared bit for bit against the NumPy
restatement tests/wfsa_push_ref.py; under "log" the backward weights against the float64 fixed point within 1e-5 (see
test_log_backward_weights) and everything made from them - pushed tables, bank rows, logZ, tokens - bit for bit again."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dfa_ref as R
from tests import wfsa_push_ref as P
from tests import wfsa_ref as W
from tests.test_wfsa_gpu import (FINAL_W, PROMPT, STRING, TOL, _byte_vocab, _mod3, _model, _one_string, _spread_vocab,  # noqa: F401
                                 byte_model, forced_total)

pytestmark = pytest.mark.gpu
CANARY = 12345.0
ICANARY = 0x5a5a5a5a
NAMES = ["digits", "everything", "trap", "random37", "trie"]
_CACHE = {}


def _automaton(name):
    """(delta, accepting, start, arc_logw, final_logw, depth or None), substochastic weights of seed 7; made once."""
    if name not in _CACHE:
        if name == "trie":
            d, acc, start, _, depth = P.trie()
            assert len(acc) % 4 and len(acc) > 3000 and depth == 8  # many workgroups, the last one not full
        else:
            (d, acc, start), depth = R.automata()[name], None
        _CACHE[name] = (d, acc, start) + P.substochastic_weights(d, acc, 7) + (depth,)
    return _CACHE[name]


def _vocab(V):
    if V not in _CACHE:
        _CACHE[V] = R.synth_vocab(V, V)
    return _CACHE[V]


class Dev:
    """The tables of one glb_dfa_push_args on the device, a canary behind every output."""

    def __init__(self, engine, d, arc, fin, start, semiring):
        self.eng, dev, S = engine, engine.device, len(fin)
        self.S = S
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.delta, self.arc, self.fin = up(np.asarray(d, np.int32)), up(arc), up(fin)
        f = lambda n: torch.full((n,), CANARY, dtype=torch.float32, device=dev)
        self.beta, self.scratch, self.final_out, self.arc_out = f(S + 8), f(S + 8), f(S + 8), f(S * 256 + 8)
        self.status = torch.full((16,), ICANARY, dtype=torch.int32, device=dev)
        self.start, self.semiring = start, semiring

    def args(self, sweeps=64, restart=0, tol=P.TOL):
        from genlm_backend_amd import _lib

        p = _lib.DfaPushArgs()
        p.struct_size = C.sizeof(_lib.DfaPushArgs)
        p.n_states, p.start = self.S, self.start
        p.semiring = _lib.DFA_PUSH_LOG if self.semiring == P.LOG else _lib.DFA_PUSH_MAX
        p.delta, p.arc_logw, p.final_logw = self.delta.data_ptr(), self.arc.data_ptr(), self.fin.data_ptr()
        p.beta, p.scratch, p.arc_out, p.final_out = (t.data_ptr() for t in (self.beta, self.scratch, self.arc_out, self.final_out))
        p.status, p.sweeps, p.restart, p.tol = self.status.data_ptr(), sweeps, restart, tol
        return p

    def backward(self, sweeps=64, restart=0, tol=P.TOL):
        """One call; (sweeps since the restart, converged, flags, sweeps of this call)."""
        self.eng.dfa_call("glb_dfa_backward", self.args(sweeps, restart, tol))
        st = self.status.cpu().tolist()
        assert st[4:8] == [0, 0, 0, 0]  # the marks are zero between calls
        return tuple(st[:4])

    def converge(self, batch=64, tol=P.TOL, limit=4096):
        total, conv, flags, _ = self.backward(batch, 1, tol)
        while not conv and total < limit:
            total, conv, flags, _ = self.backward(batch, 0, tol)
        return total, conv, flags

    def push(self):
        self.eng.dfa_call("glb_dfa_push_weights", self.args())
        return self.arc_out[:self.S * 256].cpu().numpy().reshape(self.S, 256), self.final_out[:self.S].cpu().numpy()

    def beta_host(self):
        return self.beta[:self.S].cpu().numpy()

    def canaries_intact(self):
        S = self.S
        return all(bool((t[n:] == CANARY).all()) for t, n in ((self.beta, S), (self.scratch, S), (self.final_out, S),
                                                              (self.arc_out, S * 256))) and bool((self.status[8:] == ICANARY).all())


def _same(a, b):
    return np.ascontiguousarray(a, np.float32).tobytes() == np.ascontiguousarray(b, np.float32).tobytes()


# ---- the backward weights and the pushed tables ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_max_backward_weights_and_pushed_tables_bit_for_bit(engine, name):
    d, acc, start, arc, fin, _ = _automaton(name)
    want, sweeps, ok = P.backward(d, arc, fin, P.MAX)
    assert ok and sweeps <= len(acc) + 1
    dv = Dev(engine, d, arc, fin, start, P.MAX)
    total, conv, flags = dv.converge()
    beta = dv.beta_host()
    assert (total, conv, flags) == (sweeps, 1, 0) and _same(beta, want)
    assert np.array_equal(np.isfinite(beta), R.live(np.asarray(d, np.int64), acc))
    a, f = dv.push()
    wa, wf = P.push(d, arc, fin, beta)
    assert _same(a, wa) and _same(f, wf) and dv.canaries_intact()
    assert dv.backward(8) == (sweeps, 1, 0, 0) and _same(dv.beta_host(), want)  # converged: a later call performs nothing


@pytest.mark.parametrize("name", NAMES)
def test_log_backward_weights(engine, name):
    """Within 1e-5 of the float64 fixed point.  The stop rule leaves tol * rho / (1 - rho) * max(1, |beta|) (rho <= 0.5, |beta|
    < 2.7 here: at most 2.6e-6) and the float32 restatement itself stands 2.4e-6 from the fixed point (`test_wfsa_push_cpu`
    prints it); the allowance is four times that, the device's exp / log need not be NumPy's to the last ulp."""
    d, acc, start, arc, fin, depth = _automaton(name)
    b64 = P.fixed_point64(d, arc, fin, P.LOG)
    live = R.live(np.asarray(d, np.int64), acc)
    _, ref_sweeps, _ = P.backward(d, arc, fin, P.LOG)
    dv = Dev(engine, d, arc, fin, start, P.LOG)
    total, conv, flags = dv.converge()
    beta = dv.beta_host()
    dist = np.abs(beta[live].astype(np.float64) - b64[live]).max()
    print(f"{name}: {total} sweeps (restatement {ref_sweeps}), max |beta - float64| = {dist:.3e}")
    assert (conv, flags) == (1, 0) and abs(total - ref_sweeps) <= 1
    assert np.array_equal(np.isfinite(beta), live) and np.isneginf(beta[~live]).all() and dist < 1e-5
    a, f = dv.push()
    wa, wf = P.push(d, arc, fin, beta)
    assert _same(a, wa) and _same(f, wf) and dv.canaries_intact()
    # a second run gives the same bits; one call of 64 sweeps performs what four calls of 16 do
    dv2 = Dev(engine, d, arc, fin, start, P.LOG)
    first = dv2.backward(64, 1)
    dv3 = Dev(engine, d, arc, fin, start, P.LOG)
    for k in range(4):
        last = dv3.backward(16, 1 if k == 0 else 0)
    assert first[:3] == last[:3] == (total, 1, 0) and first[3] == total and _same(dv2.beta_host(), beta) and _same(dv3.beta_host(), beta)
    assert dv2.canaries_intact() and dv3.canaries_intact()
    if depth is not None:  # acyclic: exact after depth + 1 sweeps - nothing moves at all - and further sweeps leave it so
        dv4 = Dev(engine, d, arc, fin, start, P.LOG)
        done = dv4.backward(depth + 1, 1, tol=0.0)
        # (sweep `depth` adds the longest strings' mass to the start state alone: in float32 it may or may not move it)
        assert done[0] in (depth, depth + 1) and done[1:] == (1, 0, done[0])
        exact = dv4.beta_host()
        assert np.abs(exact[live].astype(np.float64) - b64[live]).max() < 1e-5
        assert dv4.backward(4, 0, tol=0.0) == (done[0], 1, 0, 0) and _same(dv4.beta_host(), exact)
        assert dv4.backward(3, 1, tol=0.0)[:3] == (3, 0, 0)  # (an odd number of sweeps: the result is copied out of `scratch`)
        part = dv4.beta_host()
        b3 = np.asarray(fin, np.float32)
        for _ in range(3):
            b3 = P.sweep(np.asarray(d, np.int64), arc, fin, b3, P.LOG)
        assert np.array_equal(np.isfinite(part), np.isfinite(b3)) and np.abs(part[np.isfinite(b3)] - b3[np.isfinite(b3)]).max() < 1e-5
        assert dv4.backward(64, 0, tol=0.0)[:3] == (done[0], 1, 0) and _same(dv4.beta_host(), exact)


def test_weights_that_do_not_sum_raise(engine):
    """Zero weights on [0-9]+: ten arcs of mass one round a state.  Nothing faults - the device reports through status words."""
    from genlm_backend_amd.constraints import ByteWFSA, DeviceConstraint

    d, acc, start = R.automata()["digits"]
    wf = ByteWFSA(d, *W.zero_weights(d, acc), start)
    vocab, eos, skip = _vocab(300)
    with pytest.raises(ValueError, match=r'do not sum.*push="max".*push=None'):
        DeviceConstraint(engine, wf, vocab, eos, skip_ids=skip, push="log", push_max_sweeps=64)
    engine.check()
    c = DeviceConstraint(engine, wf, vocab, eos, skip_ids=skip, push="max")
    assert c.push_stats() == {"semiring": "max", "sweeps": 2} and c.start_logw == 0.0 and c.backward.cpu().tolist() == [0.0, 0.0]
    # a cycle that gains weight: "max" has no answer either
    arc = np.where(d >= 0, 0.25, -np.inf).astype(np.float32)
    with pytest.raises(ValueError, match="do not sum"):
        DeviceConstraint(engine, ByteWFSA(d, arc, W.zero_weights(d, acc)[1], start), vocab, eos, skip_ids=skip, push="max")
    # weights near the top of float32: the sums overflow and the flag word says so
    dv = Dev(engine, d, np.where(d >= 0, 3e38, -np.inf).astype(np.float32), W.zero_weights(d, acc)[1], start, P.MAX)
    total, conv, flags, _ = dv.backward(8, 1)
    assert flags == 1 and dv.canaries_intact()


def test_argument_errors_launch_nothing(engine):
    from genlm_backend_amd import _lib

    d, acc, start, arc, fin, _ = _automaton("random37")
    dv = Dev(engine, d, arc, fin, start, P.LOG)
    assert dv.backward(3, 1)[:3] == (3, 0, 0)
    dv.push()
    torch.cuda.synchronize()
    tensors = (dv.beta, dv.scratch, dv.arc_out, dv.final_out, dv.status)
    before = [t.clone() for t in tensors]
    lib, st = engine.lib, engine._stream()

    def broken(field, value):
        p = dv.args()
        setattr(p, field, value)
        return p

    both = [("struct_size", 0), ("struct_size", C.sizeof(_lib.DfaPushArgs) - 8), ("n_states", 0), ("n_states", -1), ("start", -1),
            ("start", dv.S), ("semiring", 2), ("sweeps", 0), ("sweeps", -1), ("tol", -1.0), ("tol", float("nan")), ("delta", None),
            ("arc_logw", None), ("final_logw", None), ("beta", None)]
    for fn, own in ((lib.glb_dfa_backward, [("scratch", None), ("status", None)]),
                    (lib.glb_dfa_push_weights, [("arc_out", None), ("final_out", None)])):
        assert fn(None, st) == _lib.GLB_EINVAL
        for field, value in both + own:
            assert fn(C.byref(broken(field, value)), st) == _lib.GLB_EINVAL and field in _lib.last_error(), (field, value)
    torch.cuda.synchronize()
    assert all(torch.equal(t, b) for t, b in zip(tensors, before))  # nothing ran
    assert dv.backward(64)[:3][1:] == (1, 0) and dv.canaries_intact()  # the unbroken block does run, from where it stood


# ---- the constraint -------------------------------------------------------------------------------------------------------------
def _pushed(engine, name, V, semiring, rows=None, **kw):
    """(constraint, restatement of its rows): a pushed constraint, its bank inside a canary-filled buffer, and
    `wfsa_ref.WRef` over `pushed_wfsa()`."""
    from genlm_backend_amd.constraints import ByteWFSA, DeviceConstraint

    vocab, eos, skip = _vocab(V)
    d, acc, start, arc, fin, _ = _automaton(name)
    ld = (V + 63) // 64 * 64
    c = DeviceConstraint(engine, ByteWFSA(d, arc, fin, start), vocab, eos, skip_ids=skip, push=semiring,
                         mask_bank_bytes=(256 << 20) if rows is None else rows * ld * 4, **kw)
    big = torch.full((c.capacity + 2, ld + 3), CANARY, dtype=torch.float32, device=engine.device)
    c._set_bank(big[:c.capacity])
    pw = c.pushed_wfsa()
    return c, big, pw, W.WRef(pw.delta, pw.arc_logw, pw.final_logw, start, vocab, eos, skip)


@pytest.mark.parametrize("semiring", ["log", "max"])
def test_public_api_of_a_pushed_constraint(engine, semiring):
    d, acc, start, arc, fin, _ = _automaton("random37")
    c, big, pw, ref = _pushed(engine, "random37", 300, semiring)
    beta = c.backward.cpu().numpy()
    assert c.backward.dtype == torch.float32 and c.backward.shape == (37,) and c.backward.device == engine.device
    assert isinstance(c.start_logw, float) and c.start_logw == float(beta[start]) and np.isfinite(c.start_logw)
    want, sweeps, _ = P.backward(d, arc, fin, semiring)
    assert c.push_stats()["semiring"] == semiring and abs(c.push_stats()["sweeps"] - sweeps) <= (semiring == "log")
    wa, wf = P.push(c.dfa.delta, c.dfa.arc_logw, c.dfa.final_logw, beta)
    assert _same(c._arc_logw.cpu().numpy(), wa) and _same(c._final_logw.cpu().numpy(), wf)
    assert _same(pw.final_logw, wf) and np.array_equal(pw.live, c.dfa.live)
    if semiring == "max":
        assert _same(beta, want)
    for s in P.accepted_strings(d, acc, start, 3):
        assert abs(float(pw.path_logw(s)) - (float(c.dfa.path_logw(s)) - c.start_logw)) < 1e-5
    # push=None: nothing of the above exists, the weights are the automaton's own
    from genlm_backend_amd.constraints import DeviceConstraint

    vocab, eos, skip = _vocab(300)
    plain = DeviceConstraint(engine, c.dfa, vocab, eos, skip_ids=skip)
    assert plain.push is None and plain.backward is None and plain.start_logw == 0.0
    assert plain.push_stats() == {"semiring": None, "sweeps": 0} and _same(plain.pushed_wfsa().arc_logw, c.dfa.arc_logw)


@pytest.mark.parametrize("name,V", [("random37", 300), ("trie", 2049)])
@pytest.mark.parametrize("semiring", ["log", "max"])
def test_fill_of_a_pushed_constraint_bit_for_bit(engine, name, V, semiring):
    c, big, pw, ref = _pushed(engine, name, V, semiring)
    S = c.dfa.n_states
    rng = np.random.default_rng(V)
    states = np.unique(np.concatenate([[c.dfa.start, S - 1], rng.integers(0, S, 35)])).astype(np.int32)
    ids = c.mask_rows(torch.from_numpy(states).to(engine.device)).cpu().numpy()
    c.check()
    bank = c.bank[:, :V].cpu().numpy()
    finite = 0
    for s, r in zip(states, ids):
        assert r >= 2 and _same(bank[r], ref.row(int(s))), (name, s)
        finite += int(np.isfinite(bank[r]).sum())
    assert finite > len(states) and not np.isnan(bank[ids]).any()
    assert bool((big[c.capacity:] == CANARY).all()) and bool((big[:, V:] == CANARY).all())
    # the same through an evicting bank of 8 + 2 rows: five calls of eight states
    e, ebig, epw, _ = _pushed(engine, name, V, semiring, rows=10, on_full="evict")
    assert e._evicting and _same(epw.arc_logw, pw.arc_logw) and _same(epw.final_logw, pw.final_logw)
    for k in range(0, 35, 7):
        part = states[k:k + 8]
        rows = e.mask_rows(torch.from_numpy(part).to(engine.device)).cpu().numpy()
        ebank = e.bank[:, :V].cpu().numpy()
        for s, r in zip(part, rows):
            assert r >= 2 and _same(ebank[r], ref.row(int(s))), (name, s)
    e.check()
    assert e.stats()["evictions"] > 0 and bool((ebig[10:] == CANARY).all()) and bool((ebig[:, V:] == CANARY).all())


@pytest.mark.parametrize("semiring", ["log", "max"])
def test_stateless_step_equals_a_registered_float_table(engine, semiring):
    """batch_next_token_step_device under a pushed constraint against the same call fed the float table the restatement makes
    of `pushed_wfsa()` on the host: logZ and tokens bit for bit, 48 contexts at V = 300 (the pattern of
    tests/test_wfsa_gpu.py::test_stateless_step_equals_a_registered_float_table)."""
    from genlm_backend_amd.constraints import ByteWFSA, DeviceConstraint
    from genlm_backend_amd.llm import MASK_F32

    V, n, cap, p = 300, 48, 8, 3
    m = _model(engine, V)
    vocab = _spread_vocab(V)
    d, acc, start = _mod3()
    arc, fin = P.substochastic_weights(d, acc, V)
    c = DeviceConstraint(m, ByteWFSA(d, arc, fin, start), vocab, 0, skip_ids=(0,), push=semiring)
    pw = c.pushed_wfsa()
    ref = W.WRef(pw.delta, pw.arc_logw, pw.final_logw, start, vocab, 0, (0,))
    rng = np.random.default_rng(n)
    tok = rng.integers(1, V, (n, cap)).astype(np.int32)
    for i in range(n):
        s = 0
        for j in range(p, cap):
            if rng.random() < 0.9:
                b = int(rng.integers(0, 256))
                tok[i, j] = 1 + (b if b % 3 != s else (b + 1) % 256)
            s = (s + 1) % 3
    ln = rng.integers(p, cap, n).astype(np.int32)
    tok[1, p], ln[1] = 0, p + 2  # dead contexts
    tok[2, p], ln[2] = 1, p + 1
    states = np.array([ref.advance(start, tok[i, p:ln[i]]) for i in range(n)])
    assert (states < 0).sum() >= 2 and len(set(states.tolist())) == 4
    table = np.stack([ref.wrow_dead(), ref.wrow_eos()] + [ref.row(s) for s in range(3)])
    ids = np.where(states >= 0, states + 2, 0).astype(np.int32)
    dev = engine.device
    tok_d, ln_d = torch.from_numpy(tok).to(dev), torch.from_numpy(ln).to(dev)
    pl_d = torch.full((n,), p, dtype=torch.int32, device=dev)
    m.set_rng("philox", 5)
    logZ_c, tok_c = m.batch_next_token_step_device(tok_d, ln_d, constraint=c, prompt_lengths=pl_d)
    assert m.register_masks(torch.from_numpy(table)) == 5 and m._mask_kind == MASK_F32
    m.set_rng("philox", 5)
    logZ_t, tok_t = m.batch_next_token_step_device(tok_d, ln_d, mask_ids=torch.from_numpy(ids).to(dev))
    engine.check()
    c.check()
    a, b = logZ_c.cpu().numpy(), logZ_t.cpu().numpy()
    assert a.tobytes() == b.tobytes() and torch.equal(tok_c, tok_t)
    dead = states < 0
    assert np.isneginf(a[dead]).all() and np.isfinite(a[~dead]).all() and (tok_c.cpu().numpy()[~dead] >= 0).all()


# ---- DeviceSIS ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semiring", ["log", "max"])
@pytest.mark.parametrize("kw", [dict(), dict(use_particle_kv=True), dict(use_particle_kv=True, share_kv=False),
                                dict(resample_ess=1.0)], ids=["plain", "shared-kv", "private-kv", "resample-every-step"])
def test_device_sis_forced_draws_weigh_what_the_path_weighs(byte_model, forced_total, kw, semiring):
    """tests/test_wfsa_gpu.py's one forced string under pushed weights: the particles start at `start_logw`, the pushed
    rows weigh (nearly) nothing, and every particle ends with the model's log-probability of string + EOS plus the path
    weight of the automaton as it was given - within the 1e-4 of the unpushed test."""
    from genlm_backend_amd.constraints import DeviceConstraint
    from genlm_backend_amd.sis import DeviceSIS

    m, wf, N, L = byte_model, _one_string(), 48, len(STRING)
    vocab = _byte_vocab()
    for max_tokens in (L, L + 1):
        c = DeviceConstraint(m, wf, vocab, 0, skip_ids=(0,), push=semiring)
        assert abs(c.start_logw - float(wf.path_logw(STRING))) < 1e-5  # one string: the backward weight is its weight
        assert float(c.pushed_wfsa().arc_logw[c.dfa.delta >= 0].min()) > -1e-5
        sis = DeviceSIS(m, N, PROMPT, max_tokens, 0, seed=21, constraint=c, **kw)
        assert sis.log_weights.cpu().tolist() == [np.float32(c.start_logw)] * N
        sis.run()
        ctx, lw = sis.results()
        assert int(sis.active.sum().item()) == 0 and all(bytes(t - 1 for t in cx) == STRING for cx in ctx)
        if "resample_ess" in kw:
            assert sis.n_resamples > 0
        err = np.abs(lw.astype(np.float64) - forced_total).max()
        print(f"push={semiring} max_tokens={max_tokens} {kw}: max |lw - float64| = {err:.3e}")
        assert err < TOL


def test_the_look_ahead_reaches_the_first_step(byte_model):
    """Three strings of unequal weight that part at their first byte.  Unpushed, the first step's rows weigh the three bytes
    alike (the weights sit on the final states); pushed, the row of the start state carries each branch's weight, and logZ
    is the float64 logsumexp of the model's log-probabilities plus the restated pushed row."""
    from genlm_backend_amd.constraints import ByteWFSA, DeviceConstraint

    m, vocab = byte_model, _byte_vocab()
    lex = {b"ax": float(np.log(0.9)), b"bx": float(np.log(0.01)), b"cy": float(np.log(0.09))}
    wf = ByteWFSA.from_weighted_strings(lex)
    with torch.no_grad():
        h = m._body(input_ids=torch.tensor([PROMPT], device=m.device), use_cache=False).last_hidden_state[0, -1]
        lp = torch.log_softmax(m._lm_head(h).to(torch.float64), dim=-1).cpu().numpy()
    tok = torch.tensor([PROMPT + [0] * 5] * 2, dtype=torch.int32, device=m.device)
    ln = torch.full((2,), len(PROMPT), dtype=torch.int32, device=m.device)
    logZ = {}
    for push in (None, "log", "max"):
        c = DeviceConstraint(m, wf, vocab, 0, skip_ids=(0,), push=push)
        beta = P.backward(wf.delta, wf.arc_logw, wf.final_logw, push)[0] if push else np.zeros(wf.n_states, np.float32)
        a, f = P.push(wf.delta, wf.arc_logw, wf.final_logw, beta) if push else (wf.arc_logw, wf.final_logw)
        row = W.WRef(wf.delta, a, f, 0, vocab, 0, (0,)).row(0).astype(np.float64)
        assert np.isfinite(row).sum() == 3
        x = (lp + row)[np.isfinite(row)]
        want = x.max() + np.log(np.exp(x - x.max()).sum())
        m.set_rng("philox", 5)
        got, _ = m.batch_next_token_step_device(tok, ln, constraint=c, prompt_lengths=ln)
        got = got.cpu().numpy().astype(np.float64)
        print(f"push={push}: first-step logZ {got[0]:.6f}, float64 {want:.6f}")
        assert np.abs(got - want).max() < 1e-4
        logZ[push] = got[0]
        if push == "log":  # the prior's total mass is one: the start state's backward weight is log 1
            assert abs(c.start_logw) < 1e-5
    assert abs(logZ["log"] - logZ[None]) > 0.1 and abs(logZ["max"] - logZ[None]) > 0.1
