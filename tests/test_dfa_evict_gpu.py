"""A mask bank smaller than the automaton on the GPU (glb_dfa_evict_*, DeviceConstraint(on_full="evict")): rows are compared
bit for bit against tests/dfa_ref.py / tests/wfsa_ref.py, the bookkeeping against tests/dfa_evict_ref.py - which rows a call
may take and how many, never row numbers - and whole runs against the same run over a bank that holds every state."""
import ast
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import dfa_evict_ref as E
from tests import dfa_ref as R
from tests import wfsa_ref as W

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_hotpath_tiny.npz")
CANARY_I, CANARY_F = 0x5ca1ab1e, 12345.0
NEW_MESSAGE = "smaller than one step's working set"
_CACHE = {}


def _vocab(V):
    if V not in _CACHE:
        _CACHE[V] = R.synth_vocab(V, V)
    return _CACHE[V]


class Bank:
    """An evicting constraint over `random37` whose bank of `rows` rows lies inside a canary-filled buffer (two rows behind
    it, three elements behind every row), its restatement, and the device's bookkeeping read back."""

    def __init__(self, engine, V, rows=10, weighted=False, on_full="evict"):
        from genlm_backend_amd.constraints import ByteDFA, ByteWFSA, DeviceConstraint

        vocab, eos, skip = _vocab(V)
        d, acc, start = R.automata()["random37"]
        self.V, self.S, self.weighted, self.dev = V, d.shape[0], weighted, engine.device
        if weighted:
            arc, fin = W.random_weights(d, acc, 100 + V)
            dfa, self.ref, elems = ByteWFSA(d, arc, fin, start), W.WRef(d, arc, fin, start, vocab, eos, skip), (V + 63) // 64 * 64
        else:
            dfa, self.ref, elems = ByteDFA(d, acc, start), R.Ref(d, acc, start, vocab, eos, skip), (V + 31) // 32
        c = DeviceConstraint(engine, dfa, vocab, eos, skip_ids=skip, mask_bank_bytes=rows * elems * 4, on_full=on_full)
        assert c.capacity == rows and c.bank.shape == (rows, elems) and c._evicting == (on_full == "evict" and rows < self.S + 2)
        self.big = torch.full((rows + 2, elems + 3), CANARY_F if weighted else CANARY_I, dtype=c.bank.dtype, device=self.dev)
        c._set_bank(self.big[:rows])
        self.c, self.used = c, V if weighted else elems
        self._rows = {}

    def canaries_intact(self):
        canary = CANARY_F if self.weighted else CANARY_I
        return bool((self.big[self.c.capacity:] == canary).all()) and bool((self.big[:, self.used:] == canary).all())

    def want(self, s):
        """The bank row of state s as bytes."""
        if s not in self._rows:
            row = self.ref.row(s) if self.weighted else self.ref.mask(s)
            self._rows[s] = np.ascontiguousarray(row).tobytes()
        return self._rows[s]

    def rows(self):
        return [r.tobytes() for r in self.c.bank[:, :self.used].cpu().numpy()]

    def tables(self):
        """(row_of_state, row_state, row_stamp, epoch) as the device holds them."""
        cap = self.c.capacity
        t = self.c._evict_tables.cpu().numpy()
        return self.c._row_of_state.cpu().numpy().copy(), t[:cap].copy(), t[cap:2 * cap].copy(), int(t[4 * cap + 4])

    def restatement(self):
        """tests/dfa_evict_ref.py standing where the device stands (ties may have gone either way on the device)."""
        ref = E.EvictRef(self.S, self.c.capacity)
        ros, rs, stamp, epoch = self.tables()
        ref.row_of_state[:], ref.row_state[:], ref.row_stamp[:], ref.epoch = ros, rs, stamp, epoch
        return ref

    def serve(self, states, done=None):
        """One `mask_rows` call checked against the restatement: the rows taken are `need` rows, all that must go and none
        that may not; stamps, the inverse tables and the ids agree; every row handed out has its state's contents; the
        canaries stand.  Returns (ids, the restatement's report, the rows taken)."""
        ref = self.restatement()
        before = ref.row_state.copy()
        up = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.int32)).to(self.dev)
        ids = self.c.mask_rows(up(states), done=up(done)).cpu().numpy()
        rep = ref.serve(states)
        ros, rs, stamp, epoch = self.tables()
        taken = {int(r) for r in np.nonzero(rs != before)[0]}
        assert len(taken) == rep["need"] and rep["must"] <= taken <= rep["may"], (rep, taken)
        assert epoch == ref.epoch and np.array_equal(stamp, ref.row_stamp)  # (taken rows and touched rows: this call's epoch)
        assert (rs[:2] == -1).all() and all(ros[rs[r]] == r for r in range(2, len(rs)) if rs[r] >= 0)
        assert all(rs[ros[s]] == s for s in range(self.S) if ros[s] >= 0) and (ros >= -1).all()
        assert int((ros >= 2).sum()) == int((rs >= 0).sum())  # distinct states, distinct rows
        bank, acc = self.rows(), self.ref.accepting
        served = 0
        for i, s in enumerate(states):
            ok = 0 <= s < self.S
            if done is not None and done[i]:
                assert ids[i] == (1 if ok and acc[s] else 0)
            elif not ok:
                assert ids[i] == 0
            elif ids[i]:
                assert ids[i] == ros[s] >= 2 and bank[ids[i]] == self.want(int(s)), (i, s)
                served += 1
            else:
                assert ros[s] == -1 and rep["excess"] > 0
        assert self.canaries_intact()
        return ids, rep, taken


# ---- contents under churn -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,weighted", [(300, False), (2049, False), (300, True)], ids=["bits-300", "bits-2049", "weights-300"])
def test_rows_stay_right_while_the_bank_churns(engine, V, weighted):
    b = Bank(engine, V, weighted=weighted)
    S, rng = b.S, np.random.default_rng(17 + V + weighted)
    first_used = 0
    for call in range(30):
        live = rng.choice(S, int(rng.integers(1, 9)), replace=False)
        st = live[rng.integers(0, len(live), 700)]
        st[rng.random(700) < 0.05] = -1
        st[rng.random(700) < 0.05] = S
        done = (rng.random(700) < 0.2).astype(np.int32)
        ids, rep, taken = b.serve(st, done)
        assert rep["excess"] == 0
        first_used = b.c.stats()["rows_in_use"] - 2
    b.c.check()
    stats = b.c.stats()
    assert first_used == 8 and stats["evictions"] > 0 and stats["fills"] == stats["evictions"] + first_used
    rows = b.rows()
    if weighted:
        assert rows[0] == b.ref.wrow_dead().tobytes() and rows[1] == b.ref.wrow_eos().tobytes()
    else:
        assert rows[0] == b.ref.row_dead().tobytes() and rows[1] == b.ref.row_eos().tobytes()
    assert not b.c.warm()  # (the bank cannot hold all states)


# ---- LRU order -------------------------------------------------------------------------------------------------------------------
def test_the_least_recently_requested_rows_go_first(engine):
    b = Bank(engine, 300)
    b.serve(list(range(8)))  # A
    row_a = b.tables()[0][:8].copy()
    assert sorted(row_a.tolist()) == list(range(2, 10))
    _, rep, taken = b.serve(list(range(6)))  # B: nothing to do
    assert rep["need"] == 0 and not taken and np.array_equal(b.tables()[0][:8], row_a)
    _, rep, taken = b.serve([0, 1, 8])  # C: the rows of 6 and 7 were last requested in A, all others in B
    ros = b.tables()[0]
    assert rep["may"] == {int(row_a[6]), int(row_a[7])} and ros[8] in (row_a[6], row_a[7])
    gone = 6 if ros[8] == row_a[6] else 7
    kept = 13 - gone
    assert ros[gone] == -1 and np.array_equal(ros[:6], row_a[:6]) and ros[kept] == row_a[kept]
    bank = b.rows()
    for s in [0, 1, 2, 3, 4, 5, kept, 8]:
        assert bank[ros[s]] == b.want(s), s
    _, rep, taken = b.serve([0, 1, 8, 9, 10])  # D: the other of 6 / 7 goes before any of 2 .. 5
    ros = b.tables()[0]
    assert rep["must"] == {int(row_a[kept])} and rep["may"] == {int(row_a[kept])} | {int(r) for r in row_a[2:6]}
    got = {int(ros[9]), int(ros[10])}
    assert int(row_a[kept]) in got and len(got & {int(r) for r in row_a[2:6]}) == 1 and ros[kept] == -1
    assert np.array_equal(ros[:2], row_a[:2]) and ros[8] == row_a[gone]  # requested in this call: never taken
    assert int((ros[2:6] == row_a[2:6]).sum()) == 3
    bank = b.rows()
    for s in np.nonzero(ros >= 2)[0]:
        assert bank[ros[s]] == b.want(int(s)), s
    b.c.check()
    assert b.c.stats() == {"rows_in_use": 10, "fills": 11, "evictions": 3}


# ---- more states in one call than rows --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["bits", "weights"])
def test_one_call_over_the_banks_rows_raises_with_the_new_message(engine, weighted):
    b = Bank(engine, 300, weighted=weighted)
    st = list(range(20, 32)) * 5
    ids, rep, taken = b.serve(st)
    assert rep["need"] == 8 and rep["excess"] == 4 and len(taken) == 8
    by_state = {s: {int(ids[i]) for i in range(len(st)) if st[i] == s} for s in range(20, 32)}
    assert all(len(v) == 1 for v in by_state.values())
    got = sorted(next(iter(v)) for v in by_state.values())
    assert got == [0, 0, 0, 0] + list(range(2, 10))
    assert int(b.c._overflow_word().item()) == 1 and b.c.stats() == {"rows_in_use": 10, "fills": 8, "evictions": 0}
    with pytest.raises(RuntimeError, match=NEW_MESSAGE):
        b.c.check()
    b.serve([20])
    with pytest.raises(RuntimeError, match="at least as many rows as the particles occupy distinct states"):  # sticky
        b.c.check()
    b.c._reset_bank()
    b.c.check()
    assert b.c.stats() == {"rows_in_use": 2, "fills": 0, "evictions": 0}
    ids, rep, _ = b.serve(list(range(5)))
    assert rep["need"] == 5 and (ids >= 2).all()
    ids, rep, _ = b.serve(list(range(5, 13)))
    assert rep["need"] == 8 and (ids >= 2).all() and b.c.stats()["evictions"] == 5
    b.c.check()


def test_a_bank_that_holds_every_state_takes_the_old_path(engine):
    """on_full="evict" with S + 2 rows: no eviction tables, `warm()` works, the claim path's counters."""
    b = Bank(engine, 300, rows=39)
    assert not b.c._evicting and b.c._evict_tables is None and b.c.warm()
    assert b.c.stats() == {"rows_in_use": 39, "fills": 37, "evictions": 0}
    e = Bank(engine, 300, rows=10, on_full="error")
    e.c.mask_rows(torch.arange(12, dtype=torch.int32, device=engine.device))
    with pytest.raises(RuntimeError, match="mask_bank_bytes") as err:
        e.c.check()
    assert NEW_MESSAGE not in str(err.value)


# ---- argument errors ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["bits", "weights"])
def test_argument_errors_launch_nothing(engine, weighted):
    from genlm_backend_amd import _lib

    b = Bank(engine, 300, weighted=weighted)
    c, lib, dev = b.c, engine.lib, engine.device
    b.serve([4, 9, 17])
    st = torch.tensor([1, 2, 3, 4], dtype=torch.int32, device=dev)  # a call that ran would take three rows
    out = torch.full((4,), -7, dtype=torch.int32, device=dev)
    a = c._args()
    a.n, a.state_in, a.out_rows, a.max_work = 4, st.data_ptr(), out.data_ptr(), 4
    torch.cuda.synchronize()
    snap = lambda: [t.clone() for t in (b.big, c._evict_tables, c._counters, c._row_of_state, c._work, out)]
    before = snap()

    def broken(field, value, inner=False):
        e = c._evict_args(a)
        setattr(e.dfa if inner else e, field, value)
        return e

    both = [broken("struct_size", C.sizeof(_lib.DfaEvictArgs) - 8), broken("struct_size", 0),
            broken("struct_size", C.sizeof(_lib.DfaArgs) + 8, inner=True), broken("struct_size", 0, inner=True),
            broken("capacity", 2, inner=True), broken("capacity", 1, inner=True), broken("capacity", 65536, inner=True)]
    both += [broken(k, None) for k in ("row_state", "row_stamp", "claimants", "victims", "ecounters", "epoch")]
    both += [broken(k, None, inner=True) for k in ("row_of_state", "work", "counters", "delta", "accepting", "live")]
    both += [broken("n_states", 0, inner=True), broken("start", 37, inner=True), broken("vocab", 0, inner=True)]
    if weighted:
        both += [broken("wbank", None), broken("arc_logw", None), broken("final_logw", None), broken("wbank_ld", 299)]
    else:
        both += [broken("bank", None, inner=True), broken("bank_ld", 9, inner=True), broken("arc_logw", c._delta.data_ptr())]
    serve_only = [broken("n", 0, inner=True), broken("state_in", None, inner=True), broken("out_rows", None, inner=True),
                  broken("max_work", 0, inner=True), broken("tok_ptr", None, inner=True), broken("tok_bytes", None, inner=True),
                  broken("skip", None, inner=True)]
    for fn, cases in ((lib.glb_dfa_evict_bank_init, both), (lib.glb_dfa_evict_serve, both + serve_only)):
        assert fn(None, engine._stream()) == _lib.GLB_EINVAL
        for e in cases:
            assert fn(C.byref(e), engine._stream()) == _lib.GLB_EINVAL
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(snap(), before))  # nothing ran
    # the unbroken block does run
    c._call("glb_dfa_evict_serve", c._evict_args(a))
    ros = c._row_of_state.cpu().numpy()
    assert out.cpu().tolist() == [ros[1], ros[2], ros[3], ros[4]] and (ros[1:5] >= 2).all()
    bank = b.rows()
    assert all(bank[ros[s]] == b.want(s) for s in (1, 2, 3, 4, 9, 17)) and b.canaries_intact()
    assert c.stats() == {"rows_in_use": 8, "fills": 6, "evictions": 0}


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
class Tok:
    pad_token_id = None
    eos_token_id = 0


@pytest.fixture()
def llm(engine):
    """The tiny seeded GPT-2 of tests/test_dfa_gpu.py (vocabulary 1000, EOS 0)."""
    from transformers import GPT2Config, GPT2LMHeadModel

    from genlm_backend_amd.llm import AsyncAmdLM

    gold = np.load(G)
    cfg = ast.literal_eval(bytes(gold["config_json"]).decode())
    model = GPT2LMHeadModel(GPT2Config(**cfg)).eval()
    model.load_state_dict({k[3:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("w::")})
    m = AsyncAmdLM(model.to(engine.device), None, batch_size=64, timeout=0.02, engine=engine)
    m.tokenizer = Tok()
    return m, [int(t) for t in gold["sis_prompt"]]


def _tiny_vocab():
    """1000 byte strings of 1 to 4 bytes (tests/test_dfa_gpu.py's, without its empty token): EOS (id 0, special), the 256
    single bytes, every string of 2 and 3 letters over abc, filler."""
    import itertools

    vocab = [b"<eos>"] + [bytes([b]) for b in range(256)]
    vocab += [bytes(p) for k in (2, 3) for p in itertools.product(b"abc", repeat=k)]
    vocab += [b"x%d" % i for i in range(1000 - len(vocab))]
    return vocab


def _counting(S):
    """State k goes to k + 1 on any byte, every state may end: the state is the number of bytes generated."""
    d = np.full((S, 256), -1, np.int32)
    d[:-1] = np.arange(1, S, dtype=np.int32)[:, None]
    return d, np.ones(S, np.bool_), 0


def _pair(m, vocab, S, rows, weighted):
    """(a constraint whose bank holds all S states, the same with an evicting bank of `rows` rows, the restatement)."""
    from genlm_backend_amd.constraints import ByteDFA, ByteWFSA, DeviceConstraint

    d, acc, start = _counting(S)
    if weighted:
        arc, fin = W.random_weights(d, acc, 23)
        dfa = ByteWFSA(d, arc, fin, start)
    else:
        dfa = ByteDFA(d, acc, start)
    big = DeviceConstraint(m, dfa, vocab, 0, skip_ids=(0,))
    small = DeviceConstraint(m, dfa, vocab, 0, skip_ids=(0,), mask_bank_bytes=rows * big.row_elems * 4, on_full="evict")
    assert big.capacity == S + 2 and not big._evicting and small.capacity == rows and small._evicting
    return big, small, R.Ref(d, acc, start, vocab, 0, (0,))


N_SIS, MAX_TOKENS = 8, 12  # every step adds a byte at least: 13 steps pass through more than 8 states, whatever is drawn


@pytest.mark.parametrize("kw,weighted", [(dict(), False), (dict(use_particle_kv=True), False),
                                         (dict(use_particle_kv=True, share_kv=False), False), (dict(resample_ess=1.0), False),
                                         (dict(), True)], ids=["plain", "pkv", "private-kv", "resample", "weights"])
def test_device_sis_over_an_evicting_bank_equals_the_run_over_a_full_one(llm, kw, weighted):
    """A counting automaton under 8 particles: a step's particles occupy at most 8 states, the run wanders through
    more - a bank of 8 + 2 rows serves every step and has to evict.  Contexts, lengths and log-weights bit for bit."""
    from genlm_backend_amd.sis import DeviceSIS

    m, prompt = llm
    vocab, S = _tiny_vocab(), 4 * MAX_TOKENS + 2
    big, small, ref = _pair(m, vocab, S, N_SIS + 2, weighted)
    full = DeviceSIS(m, N_SIS, prompt, MAX_TOKENS, 0, seed=31, constraint=big, **kw)
    evct = DeviceSIS(m, N_SIS, prompt, MAX_TOKENS, 0, seed=31, constraint=small, **kw)
    per_step = []
    for step in range(MAX_TOKENS + 1):
        ctx, ln, pl = (t.cpu().numpy() for t in (full.contexts, full.lengths, full.prompt_len))
        per_step.append({ref.advance(ref.start, ctx[i, pl[i]:ln[i]]) for i in range(N_SIS)} - {-1})  # what this step asks for
        assert per_step[-1] == set(full.states.cpu().tolist()) - {-1}
        full.step()
        evct.step()
        for name in ("contexts", "lengths", "active", "log_weights"):
            a, b = getattr(full, name).cpu().numpy(), getattr(evct, name).cpu().numpy()
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (step, name)
    # what makes the comparison mean something: every step fits the small bank, the run does not
    assert max(len(s) for s in per_step) <= small.capacity - 2 < len(set().union(*per_step))
    assert small.stats()["evictions"] > 0 and big.stats()["evictions"] == 0
    small.check()
    big.check()
    assert np.isfinite(full.log_weights.cpu().numpy()).any()
    if "resample_ess" in kw:
        assert full.n_resamples == evct.n_resamples > 0


def _step_model(engine, V):
    from transformers import GPT2Config

    from genlm_backend_amd.llm import AsyncAmdLM

    cfg = GPT2Config(vocab_size=V, n_positions=64, n_embd=64, n_layer=2, n_head=4, bos_token_id=0, eos_token_id=0)
    m = AsyncAmdLM.from_config(cfg, None, device=engine.device, seed=3, engine=engine, batch_size=64, timeout=0.02)
    m.tokenizer = Tok()
    return m


@pytest.mark.parametrize("weighted", [False, True], ids=["bits", "weights"])
def test_stateless_step_over_an_evicting_bank_equals_the_step_over_a_full_one(engine, weighted):
    """batch_next_token_step_device, 48 contexts at V = 300, six batches whose generated suffixes grow: a batch's byte counts
    take at most 8 values, the six together 13 - a bank of 2 + 8 rows.  logZ and tokens bit for bit."""
    V, n, p, cap = 300, 48, 2, 12
    m = _step_model(engine, V)
    rng = np.random.default_rng(V)
    vocab = [b"<eos>"] + [bytes([b]) for b in range(256)] + [bytes(rng.integers(0, 256, 2).astype(np.uint8)) for _ in range(V - 257)]
    big, small, ref = _pair(m, vocab, 32, 10, weighted)
    dev = engine.device
    asked = []
    for batch in range(6):
        tok = rng.integers(1, V, (n, cap)).astype(np.int32)
        ln = (p + batch + rng.integers(0, 2, n)).astype(np.int32)
        tok[n // 2:n // 2 + 6], ln[n // 2:n // 2 + 6] = tok[:6], ln[:6]  # contexts that coincide share a logits row
        asked.append({ref.advance(ref.start, tok[i, p:ln[i]]) for i in range(n)})
        tok_d, ln_d = torch.from_numpy(tok).to(dev), torch.from_numpy(ln).to(dev)
        pl_d = torch.full((n,), p, dtype=torch.int32, device=dev)
        got = []
        for c in (big, small):
            m.set_rng("philox", 5 + batch)
            got.append(m.batch_next_token_step_device(tok_d, ln_d, constraint=c, prompt_lengths=pl_d))
        (logZ_b, tok_b), (logZ_s, tok_s) = got
        assert logZ_b.cpu().numpy().tobytes() == logZ_s.cpu().numpy().tobytes() and torch.equal(tok_b, tok_s), batch
        assert np.isfinite(logZ_b.cpu().numpy()).all() and (tok_b >= 0).all()
    engine.check()
    assert all(-1 not in s for s in asked)
    assert max(len(s) for s in asked) <= small.capacity - 2 < len(set().union(*asked))
    assert small.stats()["evictions"] > 0
    small.check()
