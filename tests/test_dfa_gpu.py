"""Byte-level DFA constraints on the GPU (glb_dfa_*, constraints.DeviceConstraint, DeviceSIS(constraint=...)): every
comparison is exact - bits and integers - against the NumPy restatement tests/dfa_ref.py."""
import ast
import os

import numpy as np
import pytest
import torch

from tests import dfa_ref as R

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_hotpath_tiny.npz")
CANARY = 0x5ca1ab1e
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


def _constraint(engine, name, V, rows=None, pad=(2, 3)):
    """A constraint whose bank lies inside a canary-filled buffer: `pad` rows behind it, `pad` words behind every row."""
    from genlm_backend_amd.constraints import ByteDFA, DeviceConstraint

    vocab, eos, skip = _vocab(V)
    d, acc, start = _automaton(name)
    dfa = ByteDFA(d, acc, start)
    W = (V + 31) // 32
    c = DeviceConstraint(engine, dfa, vocab, eos, skip_ids=skip,
                         mask_bank_bytes=(256 << 20) if rows is None else rows * W * 4)
    assert c.capacity == (dfa.n_states + 2 if rows is None else rows) and c.bank.shape == (c.capacity, W)
    big = torch.full((c.capacity + pad[0], W + pad[1]), CANARY, dtype=torch.int32, device=engine.device)
    c._set_bank(big[:c.capacity])
    return c, big, R.Ref(d, acc, start, vocab, eos, skip)


def _canaries_intact(c, big):
    W = c.words
    return bool((big[c.capacity:] == CANARY).all()) and bool((big[:, W:] == CANARY).all())


# ---- fill ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [300, 2049])
@pytest.mark.parametrize("name", ["strings", "digits", "everything", "trap", "random37"])
def test_fill_equals_the_restatement_bit_for_bit(engine, name, V):
    c, big, ref = _constraint(engine, name, V)
    S, W = c.dfa.n_states, c.words
    assert c.warm()
    c.check()
    assert c._rows_in_use() == S + 2 and _canaries_intact(c, big)
    bank = c.bank[:, :W].cpu().numpy().view(np.uint32)
    row_of = c._row_of_state.cpu().numpy()
    assert sorted(row_of.tolist()) == list(range(2, S + 2))
    assert not bank[0].any() and np.array_equal(bank[1], ref.row_eos())
    for s in range(S):
        assert np.array_equal(bank[row_of[s]], ref.mask(s)), (name, s)
    if V % 32:
        assert not (bank[:, -1] >> (V % 32)).any()  # the bits beyond V
    work = c._work.cpu().numpy()[:S]
    assert np.array_equal(row_of[work[:, 0]], work[:, 1]) and sorted(work[:, 1].tolist()) == list(range(2, S + 2))
    # the ids: a dead state and a finished particle that may not end -> row 0, a finished one in an accepting state -> row 1
    st = torch.tensor([-1, 0, S - 1, S, 0, S - 1, -1], dtype=torch.int32, device=engine.device)
    done = torch.tensor([0, 0, 0, 0, 1, 1, 1], dtype=torch.int32, device=engine.device)
    got = c.mask_rows(st, done=done).cpu().tolist()
    acc = ref.accepting
    assert got == [0, row_of[0], row_of[S - 1], 0, int(acc[0]), int(acc[S - 1]), 0]


def test_fill_at_gpt2_vocabulary_size_with_64_states(engine):
    """V = 50257 (197 workgroups a state, a half-used last wave), 64 states claimed in two calls."""
    from genlm_backend_amd.constraints import ByteDFA, DeviceConstraint

    V, S = 50257, 64
    vocab, eos, skip = _vocab(V)
    rng = np.random.default_rng(9)
    d = rng.integers(0, S, (S, 256)).astype(np.int32)
    d[rng.random((S, 256)) < 0.3] = -1
    acc = rng.random(S) < 0.2
    c = DeviceConstraint(engine, ByteDFA(d, acc, 0), vocab, eos, skip_ids=skip)
    ref = R.Ref(d, acc, 0, vocab, eos, skip)
    dev = engine.device
    first = c.mask_rows(torch.arange(0, 40, dtype=torch.int32, device=dev)).cpu().numpy()
    second = c.mask_rows(torch.arange(20, 64, dtype=torch.int32, device=dev)).cpu().numpy()
    assert np.array_equal(first[20:], second[:20]) and sorted(set(first) | set(second)) == list(range(2, 66))
    c.check()
    bank = c.bank.cpu().numpy().view(np.uint32)
    rows = np.concatenate([first[:20], second])
    for s in range(S):
        assert np.array_equal(bank[rows[s]], ref.mask(s)), s
    assert not (bank[:, -1] >> (V % 32)).any()


# ---- advance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["strings", "digits", "random37"])
def test_advance_equals_the_restatement(engine, name):
    V = 300
    c, _, ref = _constraint(engine, name, V)
    S, dev = c.dfa.n_states, engine.device
    rng = np.random.default_rng(4)
    n, ld = 700, 9
    # tokens the automaton can take (so that walks survive), some others, the ids -1 and V
    good = [t for t in range(V) if any(ref.next(s, t) >= 0 for s in range(S))]
    tok = rng.choice(good, (n, ld)).astype(np.int32)
    noise = rng.random((n, ld))
    tok[noise < 0.05] = rng.integers(0, V, int((noise < 0.05).sum()))
    tok[3, 2], tok[4, 0], tok[5, 1], tok[6, 0] = -1, V, 256, 257  # outside the vocabulary, the empty token, a special
    frm = rng.integers(0, ld + 1, n).astype(np.int32)
    to = np.minimum(frm + rng.integers(0, 4, n), ld).astype(np.int32)
    frm[3:7], to[3:7] = 0, 4
    frm[:3], to[:3] = [0, 4, ld], [0, 4, ld]  # from == to copies the state
    st = rng.integers(-1, S, n).astype(np.int32)
    st[3:7] = c.dfa.start
    up = lambda a: torch.from_numpy(a).to(dev)
    want = np.array([ref.advance(int(st[i]), tok[i, frm[i]:to[i]]) for i in range(n)])
    got = c.advance(up(st), up(tok), up(frm), up(to)).cpu().numpy()
    assert np.array_equal(got, want)
    assert (got[st < 0] == -1).all() and np.array_equal(got[:3], st[:3]) and (got[3:7] == -1).all()
    assert (want >= 0).sum() > n // 10  # (the walks do survive)
    # one token at a time, in place, arrives at the same states as the whole range at once; null state_in = the start state
    frm0 = np.zeros(n, np.int32)
    whole = c.advance(None, up(tok), up(frm0), up(np.full(n, 4, np.int32))).cpu().numpy()
    cur = c.states0(n)
    for j in range(4):
        c.advance(cur, up(tok), up(frm0 + j), up(frm0 + j + 1), out=cur)
    assert np.array_equal(cur.cpu().numpy(), whole)
    assert np.array_equal(whole, [ref.advance(c.dfa.start, tok[i, :4]) for i in range(n)])
    # ranges that leave the matrix give dead, not a read outside it
    bad_to = np.full(n, ld + 1, np.int32)
    assert (c.advance(None, up(tok), up(frm0), up(bad_to)).cpu().numpy() == -1).all()
    assert (c.advance(None, up(tok), up(frm0 - 1), up(frm0 + 1)).cpu().numpy() == -1).all()
    assert (c.advance(None, up(tok), up(frm0 + 3), up(frm0 + 2)).cpu().numpy() == -1).all()


# ---- claim --------------------------------------------------------------------------------------------------------------------
def test_claim_gives_one_row_per_distinct_state(engine):
    c, big, ref = _constraint(engine, "random37", 300)
    dev = engine.device
    rng = np.random.default_rng(2)
    distinct = np.array([4, 9, 17, 30, 36], np.int32)
    st = distinct[rng.integers(0, 5, 1024)]
    st[rng.random(1024) < 0.1] = -1
    st[:5] = distinct
    st_d = torch.from_numpy(st).to(dev)
    rows = c.mask_rows(st_d).cpu().numpy()
    assert c._rows_in_use() == 7
    by_state = {int(s): set(rows[st == s].tolist()) for s in distinct}
    assert all(len(v) == 1 for v in by_state.values())
    assert sorted(next(iter(v)) for v in by_state.values()) == [2, 3, 4, 5, 6] and (rows[st < 0] == 0).all()
    again = c.mask_rows(st_d).cpu().numpy()
    assert np.array_equal(again, rows) and c._rows_in_use() == 7  # a second call adds none
    bank = c.bank[:, :c.words].cpu().numpy().view(np.uint32)
    for s in distinct:
        assert np.array_equal(bank[rows[st == s][0]], ref.mask(int(s)))
    assert (c._row_of_state.cpu().numpy() >= 2).sum() == 5 and _canaries_intact(c, big)
    c.check()


def test_a_full_bank_raises_and_writes_nothing_outside(engine):
    c, big, ref = _constraint(engine, "random37", 300, rows=3)
    dev = engine.device
    st = torch.tensor([4, 9, 17, 30, 36] * 40, dtype=torch.int32, device=dev)
    rows = c.mask_rows(st).cpu().numpy()
    assert c.capacity == 3 and c._rows_in_use() == 3 and _canaries_intact(c, big)
    got = sorted(set(rows.tolist()))
    assert got == [0, 2]  # one state found the bank's only free row, the others are served the empty mask
    winner = int(st.cpu().numpy()[rows == 2][0])
    assert np.array_equal(c.bank[2, :c.words].cpu().numpy().view(np.uint32), ref.mask(winner))
    assert int(c._overflow_word().item()) == 1
    with pytest.raises(RuntimeError, match="mask_bank_bytes"):
        c.check()
    c.mask_rows(st[:1])
    with pytest.raises(RuntimeError, match="mask_bank_bytes"):  # sticky
        c.check()
    assert not c.warm()
    c._reset_bank()
    c.check()


# ---- end to end ----------------------------------------------------------------------------------------------------------------
class Tok:
    pad_token_id = None
    eos_token_id = 0


@pytest.fixture()
def llm(engine):
    """The tiny seeded GPT-2 of tests/test_host_gpu.py (vocabulary 1000, EOS 0)."""
    from transformers import GPT2Config, GPT2LMHeadModel

    from genlm_backend_amd.llm import AsyncAmdLM

    gold = np.load(G)
    cfg = ast.literal_eval(bytes(gold["config_json"]).decode())
    model = GPT2LMHeadModel(GPT2Config(**cfg)).eval()
    model.load_state_dict({k[3:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("w::")})
    m = AsyncAmdLM(model.to(engine.device), None, batch_size=64, timeout=0.02, engine=engine)
    m.tokenizer = Tok()
    return m, [int(t) for t in gold["sis_prompt"]]


LANGUAGE = [b"abc", b"ab", b"abcab", b"cab", b"cabba", b"bb", b"bca", b"ccccc", b"acb", b"ba"]


def _tiny_vocab():
    """1000 byte strings: EOS (id 0, special), the 256 single bytes, every string of 2 and 3 letters over abc, an empty
    token, filler that the language never takes."""
    import itertools

    vocab = [b"<eos>"] + [bytes([b]) for b in range(256)]
    vocab += [bytes(p) for k in (2, 3) for p in itertools.product(b"abc", repeat=k)] + [b""]
    vocab += [b"x%d" % i for i in range(1000 - len(vocab))]
    return vocab


def _decode(vocab, ctx):
    return b"".join(vocab[t] for t in ctx)


def _old_way_masks(sis, ref, max_tokens):
    """What a user does today: walk the automaton over every particle's own context on the host, pack the bit rows, push
    them (`update_particle_masks`)."""
    ctx = sis.contexts.cpu().numpy()
    ln, pl = sis.lengths.cpu().numpy(), sis.prompt_len.cpu().numpy()
    made = {}  # (a state's mask is walked once a step, however many particles are in it)
    rows = []
    for i in range(sis.N):
        key = (ref.advance(ref.start, ctx[i, pl[i]:ln[i]]), bool(ln[i] - pl[i] >= max_tokens))
        if key not in made:
            made[key] = ref.particle_mask(key[0], int(ln[i] - pl[i]), max_tokens)
        rows.append(made[key])
    rows = np.stack(rows)
    sis.update_particle_masks(torch.arange(sis.N, dtype=torch.int32, device=sis.dev),
                              torch.from_numpy(rows.view(np.int32)).to(sis.dev))


@pytest.mark.parametrize("N", [48, 600])
@pytest.mark.parametrize("kw", [dict(), dict(use_particle_kv=True), dict(resample_ess=0.5),
                                dict(use_particle_kv=True, resample_ess=0.5), dict(use_particle_kv=True, share_kv=False)],
                         ids=["plain", "pkv", "ess", "pkv-ess", "private-kv"])
def test_device_sis_under_a_constraint_equals_host_built_masks(llm, N, kw):
    """A finite language: its contexts are prefixes of ten strings, so the distinct contexts - the step's units when the
    prompts have one length - stay far below 512 and every step is served gathered rows, whatever N.  Only private KV rows
    (no dedup: a unit per particle) with 600 particles hand the bank over, from their second step on.  The hand-over of the
    bank under dedup is `test_the_bank_handed_over_as_it_is_equals_host_built_masks`."""
    from genlm_backend_amd.constraints import ByteDFA, DeviceConstraint
    from genlm_backend_amd.sis import DeviceSIS

    m, prompt = llm
    vocab, dfa = _tiny_vocab(), ByteDFA.from_strings(LANGUAGE)
    ref = R.Ref(dfa.delta, dfa.accepting, dfa.start, vocab, 0, (0,))
    max_tokens = 5  # the longest string's bytes: a particle that gets there has spelled it byte by byte
    c = DeviceConstraint(m, dfa, vocab, 0, skip_ids=(0,))
    new = DeviceSIS(m, N, prompt, max_tokens, 0, seed=31, constraint=c, **kw)
    pm = torch.zeros((N + 1, ref.W), dtype=torch.int32, device=m.device)
    pm[N] = torch.from_numpy(ref.row_eos().view(np.int32)).to(m.device)
    old = DeviceSIS(m, N, prompt, max_tokens, 0, seed=31, particle_masks=pm, **kw)
    for step in range(max_tokens + 1):
        _old_way_masks(old, ref, max_tokens)
        old.step()
        new.step()
        for name in ("contexts", "lengths", "active", "log_weights"):
            a, b = getattr(new, name).cpu().numpy(), getattr(old, name).cpu().numpy()
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (step, name)
        # the stored states are the states of the contexts
        want = c.advance(None, new.contexts, new.prompt_len, new.lengths)
        assert torch.equal(new.states, want), step
    private_600 = kw.get("share_kv") is False and N == 600
    assert new.constraint_raw_steps == (max_tokens if private_600 else 0)
    ctx, lw = new.results()
    assert np.isfinite(lw).any() and int(new.active.sum().item()) == 0
    if "resample_ess" in kw:
        assert new.n_resamples > 0 and new.n_resamples == old.n_resamples
    host_states = [ref.advance(ref.start, cx) for cx in ctx]
    assert new.states.cpu().tolist() == host_states
    for cx, w in zip(ctx, lw):
        if np.isfinite(w):
            assert _decode(vocab, cx) in LANGUAGE
    new.reset()
    assert new.states.cpu().tolist() == [dfa.start] * N


def _mod3():
    """Three states that every byte moves round, each refusing the bytes of its own residue: permissive enough for a
    population to spread over hundreds of contexts, and every state's mask is different (state 1 may not end)."""
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


@pytest.mark.parametrize("kw", [dict(), dict(use_particle_kv=True)], ids=["plain", "pkv"])
@pytest.mark.parametrize("V,N", [(1000, 2000), (5000, 700)])  # one chunk of 4096 tokens and two
def test_the_bank_handed_over_as_it_is_equals_host_built_masks(engine, llm, V, N, kw):
    """One prompt length, so mask ids go per logits row, and more than 512 (distinct context, chunk) items from the
    second or third step on: those steps hand the bank itself to the one-launch step with `row_mask_id` = bank rows - the form
    a 1024-particle run over a real vocabulary takes.  Same contexts, lengths and weights, bit for bit, as a population fed
    host-built `particle_masks` before every step; the test asserts which steps took which form."""
    from transformers import GPT2Config

    from genlm_backend_amd.constraints import ByteDFA, DeviceConstraint
    from genlm_backend_amd.llm import AsyncAmdLM
    from genlm_backend_amd.sis import DeviceSIS

    m, prompt = llm
    if V != 1000:
        cfg = GPT2Config(vocab_size=V, n_positions=64, n_embd=64, n_layer=2, n_head=4, bos_token_id=0, eos_token_id=0)
        m = AsyncAmdLM.from_config(cfg, None, device=engine.device, seed=3, engine=engine, batch_size=64, timeout=0.02)
        m.tokenizer = Tok()
    vocab = _spread_vocab(V)
    d, acc, start = _mod3()
    dfa = ByteDFA(d, acc, start)
    ref = R.Ref(d, acc, start, vocab, 0, (0,))
    steps, max_tokens = 4, 6  # (no particle runs out of tokens: that rule is the finite-language tests')
    c = DeviceConstraint(m, dfa, vocab, 0, skip_ids=(0,))
    new = DeviceSIS(m, N, prompt, max_tokens, 0, seed=13, constraint=c, **kw)
    pm = torch.zeros((N + 1, ref.W), dtype=torch.int32, device=m.device)
    pm[N] = torch.from_numpy(ref.row_eos().view(np.int32)).to(m.device)
    old = DeviceSIS(m, N, prompt, max_tokens, 0, seed=13, particle_masks=pm, **kw)
    nch = (V + 4095) // 4096
    forms = []
    for step in range(steps):
        _old_way_masks(old, ref, max_tokens)
        old.step()
        before = new.constraint_raw_steps
        new.step()
        units = new.last_stats["n_unique"]
        forms.append(new.constraint_raw_steps > before)
        assert forms[-1] == (units * nch > 512), (step, units)  # the form is the one the unit count calls for
        for name in ("contexts", "lengths", "active", "log_weights"):
            a, b = getattr(new, name).cpu().numpy(), getattr(old, name).cpu().numpy()
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (step, name)
        assert torch.equal(new.states, c.advance(None, new.contexts, new.prompt_len, new.lengths)), step
    assert forms[0] is False and forms[2:] == [True, True], forms  # one shared prompt first, a spread population later
    ctx, lw = new.results()
    assert new.states.cpu().tolist() == [ref.advance(ref.start, cx) for cx in ctx]
    assert len(set(new.states.cpu().tolist()) - {-1}) == 3 and np.isfinite(lw).sum() > N // 2
    c.check()


def test_a_particle_out_of_tokens_in_a_state_that_may_not_end_dies(llm):
    from genlm_backend_amd.constraints import ByteDFA, DeviceConstraint
    from genlm_backend_amd.sis import DeviceSIS

    m, prompt = llm
    vocab, dfa = _tiny_vocab(), ByteDFA.from_strings([b"abcab", b"cc"])
    c = DeviceConstraint(m, dfa, vocab, 0, skip_ids=(0,))
    sis = DeviceSIS(m, 64, prompt, 2, 0, seed=8, constraint=c, use_particle_kv=True)
    sis.run()
    ctx, lw = sis.results()
    texts = [_decode(vocab, cx) for cx in ctx]
    assert any(np.isfinite(w) for w in lw) and any(not np.isfinite(w) for w in lw)
    for t, cx, w in zip(texts, ctx, lw):
        assert len(cx) <= 2
        assert np.isfinite(w) == (t in (b"abcab", b"cc")), (t, w)  # two tokens spell a string of the language, or the weight is zero


def test_stateless_step_under_a_constraint_equals_the_device_sis_step(llm):
    from genlm_backend_amd.constraints import ByteDFA, DeviceConstraint
    from genlm_backend_amd.sis import DeviceSIS

    m, prompt = llm
    vocab, dfa = _tiny_vocab(), ByteDFA.from_strings(LANGUAGE)
    c = DeviceConstraint(m, dfa, vocab, 0, skip_ids=(0,))
    N, steps = 600, 3
    prompts = [prompt if i % 2 else prompt[:5] for i in range(N)]  # two prompt lengths: ids per particle
    sis = DeviceSIS(m, N, prompts, 8, 0, seed=77, constraint=c)
    eng = m.engine
    ctx, ln, pl = sis.contexts.clone(), sis.lengths.clone(), sis.prompt_len.clone()
    act, lw = sis.active.clone(), sis.log_weights.clone()
    m.set_rng("philox", 77)
    with pytest.raises(ValueError):
        m.batch_next_token_step_device(ctx, ln, mask_ids=torch.zeros_like(ln), constraint=c)
    for step in range(steps):
        sis.step()
        logZ, tok = m.batch_next_token_step_device(ctx, ln, constraint=c, prompt_lengths=pl)
        eng.particles_advance(ctx, ln, act, lw, logZ, tok, 0, sis.cap)
        for a, b in ((ctx, sis.contexts), (ln, sis.lengths), (act, sis.active), (lw, sis.log_weights)):
            assert np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32)), step
    assert int(act.sum().item()) > 0 and len({tuple(r) for r in ctx.cpu().numpy().tolist()}) > 10
    c.check()
