"""Weighted byte automata on the GPU (glb_dfa_weight_bank_init / glb_dfa_fill_weights, constraints.DeviceConstraint over a
ByteWFSA, DeviceSIS and batch_next_token_step_device under one).  Rows, ids, logZ and tokens are compared exactly - bits and
integers - against the NumPy restatement tests/wfsa_ref.py; only a DeviceSIS log-weight against its float64 recomputation
has a tolerance, the one tests/test_host_gpu.py allows such a comparison (TOL = 1e-4, test_host_gpu.py:16, used at :178)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dfa_ref as R
from tests import wfsa_ref as W

pytestmark = pytest.mark.gpu
TOL = 1e-4  # tests/test_host_gpu.py:16
CANARY = 12345.0
NINF = np.float32(-np.inf)
_CACHE = {}


def _vocab(V):
    if V not in _CACHE:
        _CACHE[V] = R.synth_vocab(V, V)
    return _CACHE[V]


def _automaton(name):
    from genlm_backend_amd.constraints import ByteDFA

    if name == "strings":
        dfa = ByteDFA.from_strings([b"yes", b"no", b"yesno", b"123", b"12", b"0" * 70, b"9" * 69 + b"a"])
        return dfa.delta, dfa.accepting, dfa.start
    return R.automata()[name]


def _constraint(engine, name, V, rows=None, pad=(2, 3), zero=False):
    """A weighted constraint whose bank lies inside a canary-filled buffer: `pad` rows behind it, `pad` floats behind every
    row (and the row's own padding behind column V)."""
    from genlm_backend_amd.constraints import ByteWFSA, DeviceConstraint

    vocab, eos, skip = _vocab(V)
    d, acc, start = _automaton(name)
    arc, fin = W.zero_weights(d, acc) if zero else W.random_weights(d, acc, 100 + V)
    wf = ByteWFSA(d, arc, fin, start)
    ld = (V + 63) // 64 * 64
    c = DeviceConstraint(engine, wf, vocab, eos, skip_ids=skip, mask_bank_bytes=(256 << 20) if rows is None else rows * ld * 4)
    assert c.weighted and c.capacity == (wf.n_states + 2 if rows is None else rows)
    assert c.bank.shape == (c.capacity, ld) and c.bank.dtype == torch.float32
    big = torch.full((c.capacity + pad[0], ld + pad[1]), CANARY, dtype=torch.float32, device=engine.device)
    c._set_bank(big[:c.capacity])
    return c, big, W.WRef(d, arc, fin, start, vocab, eos, skip)


def _canaries_intact(c, big):
    return bool((big[c.capacity:] == CANARY).all()) and bool((big[:, c.vocab:] == CANARY).all())


def _same(a, b):
    return np.ascontiguousarray(a, np.float32).tobytes() == np.ascontiguousarray(b, np.float32).tobytes()


# ---- fill ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [300, 2049])
@pytest.mark.parametrize("name", ["strings", "digits", "everything", "trap", "random37"])
def test_fill_equals_the_restatement_bit_for_bit(engine, name, V):
    c, big, ref = _constraint(engine, name, V)
    S = c.dfa.n_states
    assert c.warm()
    c.check()
    assert c._rows_in_use() == S + 2 and _canaries_intact(c, big)
    bank = c.bank[:, :V].cpu().numpy()
    row_of = c._row_of_state.cpu().numpy()
    assert sorted(row_of.tolist()) == list(range(2, S + 2))
    assert _same(bank[0], ref.wrow_dead()) and _same(bank[1], ref.wrow_eos())
    for s in range(S):
        assert _same(bank[row_of[s]], ref.row(s)), (name, s)
    assert np.isfinite(bank[2:]).any() and not np.isnan(bank).any()
    # the ids are the boolean machinery's: a dead state and a finished particle that may not end -> row 0, a finished one in
    # an accepting state -> row 1
    st = torch.tensor([-1, 0, S - 1, S, 0, S - 1, -1], dtype=torch.int32, device=engine.device)
    done = torch.tensor([0, 0, 0, 0, 1, 1, 1], dtype=torch.int32, device=engine.device)
    acc = ref.accepting
    assert c.mask_rows(st, done=done).cpu().tolist() == [0, row_of[0], row_of[S - 1], 0, int(acc[0]), int(acc[S - 1]), 0]


def test_fill_at_gpt2_vocabulary_size_with_64_states(engine):
    """V = 50257 (197 workgroups a state, a half-used last wave), 64 states claimed in two calls."""
    from genlm_backend_amd.constraints import ByteWFSA, DeviceConstraint

    V, S = 50257, 64
    vocab, eos, skip = _vocab(V)
    rng = np.random.default_rng(9)
    d = rng.integers(0, S, (S, 256)).astype(np.int32)
    d[rng.random((S, 256)) < 0.3] = -1
    acc = rng.random(S) < 0.2
    arc, fin = W.random_weights(d, acc, 10)
    c = DeviceConstraint(engine, ByteWFSA(d, arc, fin, 0), vocab, eos, skip_ids=skip)
    ld = c.bank.shape[1]
    big = torch.full((c.capacity + 1, ld + 2), CANARY, dtype=torch.float32, device=engine.device)
    c._set_bank(big[:c.capacity])
    ref = W.WRef(d, arc, fin, 0, vocab, eos, skip)
    dev = engine.device
    first = c.mask_rows(torch.arange(0, 40, dtype=torch.int32, device=dev)).cpu().numpy()
    second = c.mask_rows(torch.arange(20, 64, dtype=torch.int32, device=dev)).cpu().numpy()
    assert np.array_equal(first[20:], second[:20]) and sorted(set(first) | set(second)) == list(range(2, 66))
    c.check()
    assert _canaries_intact(c, big)
    bank = c.bank[:, :V].cpu().numpy()
    rows = np.concatenate([first[:20], second])
    assert _same(bank[0], ref.wrow_dead()) and _same(bank[1], ref.wrow_eos())
    for s in range(S):
        assert _same(bank[rows[s]], ref.row(s)), s


@pytest.mark.parametrize("name", ["strings", "random37"])
def test_zero_weights_give_the_boolean_bank_expanded(engine, name):
    """The identity on the device: glb_dfa_fill_weights at all-zero weights against glb_dfa_fill_masks' bits."""
    from genlm_backend_amd.constraints import ByteDFA, DeviceConstraint

    V = 2049
    c, big, _ = _constraint(engine, name, V, zero=True)
    vocab, eos, skip = _vocab(V)
    b = DeviceConstraint(engine, ByteDFA(*_automaton(name)), vocab, eos, skip_ids=skip)
    assert c.warm() and b.warm() and not b.weighted
    wbank, bits = c.bank[:, :V].cpu().numpy(), b.bank.cpu().numpy().view(np.uint32)
    wrow, brow = c._row_of_state.cpu().numpy(), b._row_of_state.cpu().numpy()
    for r in (0, 1):
        assert _same(wbank[r], W.bits_to_weights(bits[r], V))
    for s in range(c.dfa.n_states):
        assert _same(wbank[wrow[s]], W.bits_to_weights(bits[brow[s]], V)), (name, s)
    assert _canaries_intact(c, big)


# ---- claim and ids with the float bank -----------------------------------------------------------------------------------------
def test_claim_gives_one_row_per_distinct_state(engine):
    c, big, ref = _constraint(engine, "random37", 300)
    rng = np.random.default_rng(2)
    distinct = np.array([4, 9, 17, 30, 36], np.int32)
    st = distinct[rng.integers(0, 5, 1024)]
    st[rng.random(1024) < 0.1] = -1
    st[:5] = distinct
    st_d = torch.from_numpy(st).to(engine.device)
    rows = c.mask_rows(st_d).cpu().numpy()
    assert c._rows_in_use() == 7
    by_state = {int(s): set(rows[st == s].tolist()) for s in distinct}
    assert all(len(v) == 1 for v in by_state.values())
    assert sorted(next(iter(v)) for v in by_state.values()) == [2, 3, 4, 5, 6] and (rows[st < 0] == 0).all()
    assert np.array_equal(c.mask_rows(st_d).cpu().numpy(), rows) and c._rows_in_use() == 7  # a second call adds none
    bank = c.bank[:, :300].cpu().numpy()
    for s in distinct:
        assert _same(bank[rows[st == s][0]], ref.row(int(s)))
    assert bool((big[7:c.capacity, :300] == CANARY).all())  # rows nobody claimed are not written
    assert (c._row_of_state.cpu().numpy() >= 2).sum() == 5 and _canaries_intact(c, big)
    c.check()


def test_a_full_bank_raises_and_writes_nothing_outside(engine):
    c, big, ref = _constraint(engine, "random37", 300, rows=3)
    st = torch.tensor([4, 9, 17, 30, 36] * 40, dtype=torch.int32, device=engine.device)
    rows = c.mask_rows(st).cpu().numpy()
    assert c.capacity == 3 and c._rows_in_use() == 3 and _canaries_intact(c, big)
    assert sorted(set(rows.tolist())) == [0, 2]  # one state found the only free row, the others are served row 0: all -inf
    winner = int(st.cpu().numpy()[rows == 2][0])
    bank = c.bank[:, :300].cpu().numpy()
    assert _same(bank[2], ref.row(winner)) and np.isneginf(bank[0]).all()
    assert int(c._overflow_word().item()) == 1
    with pytest.raises(RuntimeError, match="mask_bank_bytes"):
        c.check()
    assert not c.warm()
    c._reset_bank()
    c.check()


def test_a_bank_of_fewer_than_three_rows_is_refused(engine):
    from genlm_backend_amd.constraints import ByteWFSA, DeviceConstraint

    vocab, eos, skip = _vocab(300)
    d, acc, start = _automaton("digits")
    wf = ByteWFSA(d, *W.zero_weights(d, acc), start)
    with pytest.raises(ValueError, match="mask_bank_bytes.*1280 bytes"):  # 300 floats padded to 320
        DeviceConstraint(engine, wf, vocab, eos, skip_ids=skip, mask_bank_bytes=3 * 1280 - 1)
    assert DeviceConstraint(engine, wf, vocab, eos, skip_ids=skip, mask_bank_bytes=3 * 1280).capacity == 3


# ---- argument errors ------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(engine):
    from genlm_backend_amd import _lib

    c, big, ref = _constraint(engine, "random37", 300)
    lib, V = engine.lib, 300
    st = torch.tensor([4, 9], dtype=torch.int32, device=engine.device)
    a = c._args()
    a.n, a.state_in = 2, st.data_ptr()
    c._call("glb_dfa_claim_rows", a)  # two entries wait in the work list: a fill that ran would write rows 2 and 3
    a.max_work = 2
    torch.cuda.synchronize()
    before, counters = big.clone(), c._counters.clone()
    assert counters.cpu().tolist()[:2] == [4, 0]

    def broken(field, value, inner=False):
        w = c._weight_args(a)
        setattr(w.dfa if inner else w, field, value)
        return w

    cases = [broken("struct_size", C.sizeof(_lib.DfaWeightArgs) - 8), broken("struct_size", 0),
             broken("struct_size", C.sizeof(_lib.DfaArgs) + 8, inner=True), broken("struct_size", 0, inner=True),
             broken("wbank_ld", V - 1), broken("wbank_ld", 0), broken("arc_logw", None), broken("final_logw", None),
             broken("wbank", None), broken("delta", None, inner=True), broken("live", None, inner=True),
             broken("row_of_state", None, inner=True), broken("work", None, inner=True), broken("counters", None, inner=True),
             broken("capacity", 1, inner=True), broken("n_states", 0, inner=True)]
    for fn in (lib.glb_dfa_weight_bank_init, lib.glb_dfa_fill_weights):
        assert fn(None, engine._stream()) == _lib.GLB_EINVAL
        for w in cases:
            assert fn(C.byref(w), engine._stream()) == _lib.GLB_EINVAL
    assert "n_states" in _lib.last_error()
    for w in (broken("tok_ptr", None, inner=True), broken("skip", None, inner=True), broken("max_work", 0, inner=True)):
        assert lib.glb_dfa_fill_weights(C.byref(w), engine._stream()) == _lib.GLB_EINVAL
    w = broken("wbank_ld", V - 1)
    assert lib.glb_dfa_fill_weights(C.byref(w), engine._stream()) == _lib.GLB_EINVAL and "wbank_ld" in _lib.last_error()
    w = broken("struct_size", 12)
    assert lib.glb_dfa_fill_weights(C.byref(w), engine._stream()) == _lib.GLB_EINVAL and "struct_size" in _lib.last_error()
    torch.cuda.synchronize()
    assert torch.equal(big, before) and torch.equal(c._counters, counters)  # nothing ran
    # the unbroken block does run, and writes the two rows
    c._call("glb_dfa_fill_weights", c._weight_args(a))
    rows = c._row_of_state.cpu().numpy()
    bank = c.bank[:, :V].cpu().numpy()
    assert sorted([rows[4], rows[9]]) == [2, 3] and _same(bank[rows[4]], ref.row(4)) and _same(bank[rows[9]], ref.row(9))
    assert c._counters.cpu().tolist()[:2] == [4, 2] and _canaries_intact(c, big)


# ---- step level -----------------------------------------------------------------------------------------------------------------
class Tok:
    pad_token_id = None
    eos_token_id = 0


def _model(engine, V):
    from transformers import GPT2Config

    from genlm_backend_amd.llm import AsyncAmdLM

    cfg = GPT2Config(vocab_size=V, n_positions=64, n_embd=64, n_layer=2, n_head=4, bos_token_id=0, eos_token_id=0)
    m = AsyncAmdLM.from_config(cfg, None, device=engine.device, seed=3, engine=engine, batch_size=64, timeout=0.02)
    m.tokenizer = Tok()
    return m


def _mod3():
    """Three states that every byte moves round, each refusing the bytes of its own residue (tests/test_dfa_gpu.py); state 1
    may not end."""
    d = np.full((3, 256), -1, np.int32)
    for s in range(3):
        for b in range(256):
            if b % 3 != s:
                d[s, b] = (s + 1) % 3
    return d, np.array([True, False, True]), 0


def _spread_vocab(V):
    """EOS (id 0, special), the 256 single bytes, seeded two-byte tokens."""
    rng = np.random.default_rng(V)
    return [b"<eos>"] + [bytes([b]) for b in range(256)] + [bytes(rng.integers(0, 256, 2).astype(np.uint8)) for _ in range(V - 257)]


@pytest.mark.parametrize("V,n", [(300, 48), (5000, 700)])
def test_stateless_step_equals_a_registered_float_table(engine, V, n):
    """batch_next_token_step_device under the weighted constraint against the same call fed a float table built on the host
    by the restatement (register_masks) and the restated row ids: logZ and tokens bit for bit.  48 contexts at one chunk
    stay below 512 (unit, chunk) items - the two-launch form; 700 contexts at two chunks of 4096 tokens take the one-launch
    form (csrc/glb_api.hip `fused`)."""
    from genlm_backend_amd.constraints import ByteWFSA, DeviceConstraint

    m = _model(engine, V)
    vocab = _spread_vocab(V)
    d, acc, start = _mod3()
    arc, fin = W.random_weights(d, acc, V)
    ref = W.WRef(d, arc, fin, start, vocab, 0, (0,))
    c = DeviceConstraint(m, ByteWFSA(d, arc, fin, start), vocab, 0, skip_ids=(0,))
    rng = np.random.default_rng(n)
    cap, p = 8, 3
    tok = rng.integers(1, V, (n, cap)).astype(np.int32)
    # suffixes the automaton mostly takes: single bytes (ids 1 .. 256) of the residue each state allows, some random ids
    for i in range(n):
        s = 0
        for j in range(p, cap):
            if rng.random() < 0.9:
                b = int(rng.integers(0, 256))
                tok[i, j] = 1 + (b if b % 3 != s else (b + 1) % 256)
            s = (s + 1) % 3
    ln = rng.integers(p, cap, n).astype(np.int32)
    tok[1, p], ln[1] = 0, p + 2  # dead contexts: EOS (a skipped id) among the generated tokens, a byte state 0 refuses
    tok[2, p], ln[2] = 1, p + 1
    tok[n // 4:n // 4 + n // 8] = tok[:n // 8]  # contexts that coincide share a logits row
    ln[n // 4:n // 4 + n // 8] = ln[:n // 8]
    states = np.array([ref.advance(start, tok[i, p:ln[i]]) for i in range(n)])
    assert (states < 0).sum() >= 2 and len(set(states.tolist())) == 4  # dead contexts and every state
    table = np.stack([ref.wrow_dead(), ref.wrow_eos()] + [ref.row(s) for s in range(3)])
    ids = np.where(states >= 0, states + 2, 0).astype(np.int32)
    units = len({tuple(tok[i, :ln[i]].tolist()) for i in range(n)})
    nch = (V + 4095) // 4096
    assert (units * nch > 512) == (n == 700)  # which form the step takes: ids go per logits row (one prompt length)
    dev = engine.device
    tok_d, ln_d = torch.from_numpy(tok).to(dev), torch.from_numpy(ln).to(dev)
    pl_d = torch.full((n,), p, dtype=torch.int32, device=dev)
    m.set_rng("philox", 5)
    logZ_c, tok_c = m.batch_next_token_step_device(tok_d, ln_d, constraint=c, prompt_lengths=pl_d)
    assert m.register_masks(torch.from_numpy(table)) == 5
    from genlm_backend_amd.llm import MASK_F32
    assert m._mask_kind == MASK_F32  # (weights, not 0 / -inf: the table stays float)
    m.set_rng("philox", 5)
    logZ_t, tok_t = m.batch_next_token_step_device(tok_d, ln_d, mask_ids=torch.from_numpy(ids).to(dev))
    engine.check()
    c.check()
    a, b = logZ_c.cpu().numpy(), logZ_t.cpu().numpy()
    assert a.tobytes() == b.tobytes() and torch.equal(tok_c, tok_t)
    toks = tok_c.cpu().numpy()
    dead = states < 0
    assert np.isneginf(a[dead]).all() and (toks[dead] == -1).all()
    assert np.isfinite(a[~dead]).all() and (toks[~dead] >= 0).all() and (a[~dead] < 0).all()
    # the tokens drawn are tokens the state's row allows
    for i in np.nonzero(~dead)[0][:64]:
        assert np.isfinite(table[ids[i], toks[i]])


# ---- DeviceSIS ------------------------------------------------------------------------------------------------------------------
STRING = b"hello"
ARC_W = [-0.3, -1.7, -0.01, -2.5, -0.9]
FINAL_W = -1.1
PROMPT = [5, 17, 99]


def _byte_vocab():
    """EOS (id 0, special) and the 256 single bytes."""
    return [b"<eos>"] + [bytes([b]) for b in range(256)]


def _one_string():
    from genlm_backend_amd.constraints import ByteWFSA

    L = len(STRING)
    d = np.full((L + 1, 256), -1, np.int32)
    arc = np.full((L + 1, 256), -np.inf, np.float32)
    for i, b in enumerate(STRING):
        d[i, b], arc[i, b] = i + 1, ARC_W[i]
    fin = np.full(L + 1, -np.inf, np.float32)
    fin[L] = FINAL_W
    return ByteWFSA(d, arc, fin, 0)


@pytest.fixture(scope="module")
def byte_model(engine):
    return _model(engine, 257)


@pytest.fixture(scope="module")
def forced_total(byte_model):
    """float64: sum of log p(token | context) over the string's bytes and the EOS behind them, from a plain forward of the
    model over prompt + string, plus the string's path weight.  Computed once."""
    m = byte_model
    toks = [b + 1 for b in STRING]
    ids = torch.tensor([PROMPT + toks], device=m.device)
    with torch.no_grad():
        h = m._body(input_ids=ids, use_cache=False).last_hidden_state[0]
        logits = m._lm_head(h).to(torch.float64)
    lp = torch.log_softmax(logits, dim=-1).cpu().numpy()
    at = len(PROMPT) - 1
    total = sum(lp[at + t, tk] for t, tk in enumerate(toks + [0]))
    wf = _one_string()
    chain = np.float32(0.0)
    for w in ARC_W + [FINAL_W]:
        chain = np.float32(chain + np.float32(w))
    assert wf.path_logw(STRING) == chain and wf.accepts(STRING)
    return float(total) + float(wf.path_logw(STRING))


@pytest.mark.parametrize("kw", [dict(), dict(use_particle_kv=True), dict(use_particle_kv=True, share_kv=False),
                                dict(resample_ess=1.0)], ids=["plain", "shared-kv", "private-kv", "resample-every-step"])
def test_device_sis_forced_draws_weigh_what_the_path_weighs(byte_model, forced_total, kw):
    """One weighted string: every state allows exactly one token, so every particle spells it and its log-weight is the
    model's log-probability of string + EOS plus the path weight - whether it ends because it ran out of tokens (row 1, the
    final weight added by DeviceSIS) or chooses EOS from its state's own row."""
    from genlm_backend_amd.constraints import DeviceConstraint
    from genlm_backend_amd.sis import DeviceSIS

    m, wf, N, L = byte_model, _one_string(), 48, len(STRING)
    vocab = _byte_vocab()
    ref = W.WRef(wf.delta, wf.arc_logw, wf.final_logw, 0, vocab, 0, (0,))
    totals = []
    for max_tokens in (L, L + 1):
        c = DeviceConstraint(m, wf, vocab, 0, skip_ids=(0,))
        sis = DeviceSIS(m, N, PROMPT, max_tokens, 0, seed=21, constraint=c, **kw)
        sis.run()
        ctx, lw = sis.results()
        assert int(sis.active.sum().item()) == 0 and sis.t >= L + 1
        assert sis.constraint_raw_steps == sis.t  # a float bank is handed over in every step
        assert all(bytes(t - 1 for t in cx) == STRING for cx in ctx)
        assert sis.states.cpu().tolist() == [ref.advance(0, cx) for cx in ctx] == [L] * N
        if "resample_ess" in kw:
            assert sis.n_resamples > 0
        print(f"max_tokens={max_tokens} {kw}: max |lw - float64| = {np.abs(lw.astype(np.float64) - forced_total).max():.3e}")
        assert np.abs(lw.astype(np.float64) - forced_total).max() < TOL
        totals.append(lw)
    assert np.abs(totals[0].astype(np.float64) - totals[1].astype(np.float64)).max() < TOL


def test_a_weighted_run_is_deterministic(byte_model):
    from genlm_backend_amd.constraints import ByteWFSA, DeviceConstraint
    from genlm_backend_amd.sis import DeviceSIS

    m, vocab = byte_model, _byte_vocab()
    lex = {b"abc": -0.5, b"ab": -2.0, b"abcab": -0.1, b"cab": -1.0, b"cabba": -3.0, b"bb": -0.7, b"bca": -1.3, b"ba": -0.2}
    wf = ByteWFSA.from_weighted_strings(lex)
    runs = []
    for _ in range(2):
        c = DeviceConstraint(m, wf, vocab, 0, skip_ids=(0,))
        sis = DeviceSIS(m, 48, PROMPT, 5, 0, seed=9, constraint=c, use_particle_kv=True, resample_ess=0.5)
        sis.run()
        ctx, lw = sis.results()
        runs.append((ctx, lw, sis.states.cpu().tolist()))
    assert runs[0][0] == runs[1][0] and runs[0][1].tobytes() == runs[1][1].tobytes() and runs[0][2] == runs[1][2]
    ref = W.WRef(wf.delta, wf.arc_logw, wf.final_logw, 0, vocab, 0, (0,))
    assert runs[0][2] == [ref.advance(0, cx) for cx in runs[0][0]]
    texts = {bytes(t - 1 for t in cx) for cx, w in zip(runs[0][0], runs[0][1]) if np.isfinite(w)}
    assert texts and texts <= set(lex) and len(texts) > 1
