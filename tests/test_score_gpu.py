"""glb_score_rows / HipEngine.score_rows / batch_sequence_logprobs* on the GPU against the float64 reference tests/score_ref.py.

Tolerances (tests/test_importance_gpu.py's derivation): a log-sum-exp is within 1e-4 of the exact value of the widened inputs
(the library's contract), so `lse` is held to 1e-4 and every output that is a difference involving two log-sum-exps or a
log-sum-exp and a float32-rounded logit (`logp`, `logZ`, `logp_masked`) to 2e-4.  -inf is matched exactly; no NaN anywhere."""
import math

import numpy as np
import pytest
import torch

from tests import score_ref as SR

pytestmark = pytest.mark.gpu

NAMES = ("logp", "lse", "logZ", "logp_masked")
TOLS = (2e-4, 1e-4, 2e-4, 2e-4)
NAN = float("nan")
CANARY = 12345.0
DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def _logits(seed, n, V):
    """2 N(0, 1) clipped to 30; a tenth -inf in every third row; (n >= 3) row 1 all -inf, row 2 one finite entry."""
    rs = np.random.default_rng(seed)
    x = np.clip(2 * rs.standard_normal((n, V)), -30, 30).astype(np.float32)
    for r in range(0, n, 3):
        x[r, rs.random(V) < 0.1] = -np.inf
    if n >= 3:
        x[1] = -np.inf
        x[2] = -np.inf
        x[2, int(rs.integers(V))] = 1.5
    return x


def _targets(seed, x):
    """index 0, V - 1, a -inf entry, -1 and V among random ones."""
    n, V = x.shape
    rs = np.random.default_rng(seed + 7)
    t = rs.integers(0, V, n).astype(np.int32)
    special = [0, V - 1, -1, V]
    for r, v in zip(range(n - 1, -1, -1), special):
        t[r] = v
    if n > 8:
        dead = np.flatnonzero(np.isneginf(x[3]))
        if len(dead):
            t[3] = dead[0]
    return t


def _dev_matrix(x32, dtype, dev, pad=5):
    """x as a device matrix of `dtype` with pitch V + pad, NaN in the padding, its base one element past the allocation's
    (no 16-byte alignment anywhere); and the values it holds, float32 (exact)."""
    n, V = x32.shape
    flat = torch.full((n * (V + pad) + 1,), NAN, dtype=dtype, device=dev)
    t = flat[1:].view(n, V + pad)
    t[:, :V] = torch.from_numpy(x32).to(dev).to(dtype)
    return t[:, :V], t[:, :V].float().cpu().numpy()


def _mask_table(seed, V):
    """bool [6, V] allowed (tests/test_importance_gpu.py's table): two random rows, a row allowing nothing, one allowing one
    token, one with a whole chunk forbidden (the first 4096 tokens; the first half of a shorter row), one allowing only the tail
    of the last chunk."""
    rs = np.random.default_rng(seed + 1000)
    ok = np.zeros((6, V), bool)
    ok[0] = rs.random(V) < 0.6
    ok[1] = rs.random(V) < 0.3
    ok[3, int(rs.integers(V))] = True
    ok[4] = rs.random(V) < 0.5
    ok[4, :4096 if V > 4096 else V // 2] = False
    last = (V - 1) // 4096 * 4096
    ok[5, max(last, V - 50):] = True
    return ok


def _bits(ok, pad=2):
    """int32 bit rows [n, words + pad]; the padding words and the bits beyond V are set (garbage a reader must ignore)."""
    n, V = ok.shape
    words = (V + 31) // 32
    full = np.ones((n, words * 32), bool)
    full[:, :V] = ok
    w = np.packbits(full.reshape(n, words, 32), axis=-1, bitorder="little").view(np.uint32).reshape(n, words)
    return np.concatenate([w, np.full((n, pad), 0xFFFFFFFF, np.uint32)], axis=1).view(np.int32)


def _floats(seed, ok, pad=3):
    """float32 rows [n, V + pad]: finite weights where allowed, -inf elsewhere, NaN in the padding."""
    n, V = ok.shape
    rs = np.random.default_rng(seed + 2000)
    w = np.where(ok, rs.standard_normal((n, V)), -np.inf).astype(np.float32)
    return np.concatenate([w, np.full((n, pad), np.nan, np.float32)], axis=1)


def _compare(got, ref, what):
    for k, (name, tol) in enumerate(zip(NAMES, TOLS)):
        if name not in got:
            continue
        g = got[name].cpu().numpy().astype(np.float64)
        r = ref[:, k]
        assert not np.isnan(g).any(), (what, name)
        inf = np.isneginf(r)
        assert np.array_equal(np.isneginf(g), inf), (what, name, np.flatnonzero(np.isneginf(g) != inf)[:5])
        err = np.abs(g[~inf] - r[~inf]).max() if (~inf).any() else 0.0
        print(f"{what} {name}: max err {err:.3g}")
        assert err <= tol, (what, name, err)


@pytest.mark.parametrize("n", [1, 3, 67])
@pytest.mark.parametrize("V", [1, 31, 33, 4095, 4096, 4097, 8193])
def test_values(engine, V, n):
    dev = engine.device
    x32 = _logits(V * 131 + n, n, V)
    tok = _targets(V + n, x32)
    tok_d = torch.from_numpy(tok).to(dev)
    ok = _mask_table(V, V)
    ids = (np.arange(n) % 6).astype(np.int32)
    bits, ids_d = torch.from_numpy(_bits(ok)).to(dev), torch.from_numpy(ids).to(dev)
    for dtype in DTYPES:
        x_d, xv = _dev_matrix(x32, dtype, dev)
        for scale in (1.0, 0.5):
            got = engine.score_rows(x_d, tok_d, logit_scale=scale, want=NAMES)
            _compare(got, SR.score_rows(xv, tok, scale), f"V={V} n={n} {dtype} scale={scale} plain")
            assert torch.equal(got["logp"].view(torch.int32), got["logp_masked"].view(torch.int32))
            got = engine.score_rows(x_d, tok_d, logit_scale=scale, mask_kind=1, mask=bits, row_mask_id=ids_d, want=NAMES)
            _compare(got, SR.score_rows(xv, tok, scale, 1, _bits(ok, 0), ids), f"V={V} n={n} {dtype} scale={scale} bits")


@pytest.mark.parametrize("shape,dtype", [((4, 50257), torch.float32), ((2, 128256), torch.bfloat16)])
def test_values_at_model_vocabularies(engine, shape, dtype):
    dev = engine.device
    n, V = shape
    x32 = _logits(V, n, V)
    tok = _targets(V, x32)
    x_d, xv = _dev_matrix(x32, dtype, dev)
    ok = _mask_table(V, V)[[0, 4, 5, 3][:n]]
    got = engine.score_rows(x_d, torch.from_numpy(tok).to(dev), logit_scale=0.5, mask_kind=1, mask=torch.from_numpy(_bits(ok)).to(dev),
                            want=NAMES)  # (no ids: n_masks == n_rows)
    _compare(got, SR.score_rows(xv, tok, 0.5, 1, _bits(ok, 0)), f"{shape} {dtype}")


@pytest.mark.parametrize("V", [33, 4097, 8193])
def test_masks(engine, V):
    """The six-row table as bit rows and as float rows; ids given, null with one mask, null with one mask per row; an id out of
    range is a row whose mask allows nothing."""
    dev = engine.device
    n = 12
    x32 = _logits(V + 5, n, V)
    tok = _targets(V, x32)
    tok_d = torch.from_numpy(tok).to(dev)
    ok = _mask_table(V, V)
    ids = (np.arange(n) % 6).astype(np.int32)
    ids[4], ids[5] = 6, -1  # out of range
    tables = {1: (_bits(ok), _bits(ok, 0)), 2: (_floats(V, ok), _floats(V, ok, 0))}
    for dtype in DTYPES:
        x_d, xv = _dev_matrix(x32, dtype, dev)
        for kind, (padded, plain) in tables.items():
            tab_d = torch.from_numpy(padded).to(dev)
            view = tab_d[:, :plain.shape[1] + 1]  # a pitch beyond the row, garbage / NaN behind it
            got = engine.score_rows(x_d, tok_d, mask_kind=kind, mask=view, row_mask_id=torch.from_numpy(ids).to(dev), want=NAMES)
            _compare(got, SR.score_rows(xv, tok, 1.0, kind, plain, ids), f"V={V} {dtype} kind={kind} ids")
            assert np.isneginf(got["logZ"][4:6].cpu().numpy()).all() and np.isneginf(got["logp_masked"][4:6].cpu().numpy()).all()
            got = engine.score_rows(x_d, tok_d, mask_kind=kind, mask=view[:1], want=NAMES)
            _compare(got, SR.score_rows(xv, tok, 1.0, kind, plain[:1]), f"V={V} {dtype} kind={kind} one mask")
            per_row = np.ascontiguousarray(padded[ids % 6])
            got = engine.score_rows(x_d, tok_d, mask_kind=kind, mask=torch.from_numpy(per_row).to(dev), want=NAMES)
            _compare(got, SR.score_rows(xv, tok, 1.0, kind, plain[ids % 6]), f"V={V} {dtype} kind={kind} a mask per row")


@pytest.mark.parametrize("dtype", DTYPES)
def test_cut_invariance(engine, dtype):
    """67 rows in one call, in calls of 1 + 66, and in 67 calls of one row: the same bits."""
    dev = engine.device
    n, V = 67, 8193
    x32 = _logits(99, n, V)
    tok_d = torch.from_numpy(_targets(99, x32)).to(dev)
    x_d, _ = _dev_matrix(x32, dtype, dev)
    ids = torch.from_numpy((np.arange(n) % 6).astype(np.int32)).to(dev)
    bits = torch.from_numpy(_bits(_mask_table(V, V))).to(dev)

    def run(a, b):
        return engine.score_rows(x_d[a:b], tok_d[a:b].contiguous(), logit_scale=0.5, mask_kind=1, mask=bits, row_mask_id=ids[a:b].contiguous(),
                                 want=NAMES)

    whole = run(0, n)
    split = [run(0, 1), run(1, n)]
    single = [run(r, r + 1) for r in range(n)]
    for name in NAMES:
        w = whole[name].view(torch.int32)
        assert torch.equal(w, torch.cat([p[name] for p in split]).view(torch.int32)), name
        assert torch.equal(w, torch.cat([p[name] for p in single]).view(torch.int32)), name


def test_sequence_sums(engine):
    dev = engine.device
    n, V = 40, 4097
    x32 = _logits(5, n, V)
    tok = _targets(5, x32)
    tok[10] = 7  # (keep a finite row in the second sequence)
    x_d, _ = _dev_matrix(x32, torch.float32, dev)
    starts = np.array([0, 0, 1, 9, 9, 20, 37, 40, 40], np.int64)  # empty first, in the middle and last
    bits = torch.from_numpy(_bits(_mask_table(V, V)[:1])).to(dev)
    got = engine.score_rows(x_d, torch.from_numpy(tok).to(dev), mask_kind=1, mask=bits, seq_start=torch.from_numpy(starts).to(dev),
                            want=NAMES)
    assert "seq_lse" not in got
    some_inf = False
    for name in ("logp", "logZ", "logp_masked"):
        rows = got[name].cpu().numpy()
        want = SR.seq_sums(rows, starts)
        have = got["seq_" + name].cpu().numpy()
        assert np.array_equal(want.view(np.int32), have.view(np.int32)), (name, want, have)
        assert have[0] == 0.0 and have[3] == 0.0 and have[-1] == 0.0
        some_inf |= bool(np.isneginf(have).any()) and bool(np.isfinite(have[[1, 2, 4, 5, 6]]).any())
        alone = engine.score_seq_sums(got[name], torch.from_numpy(starts).to(dev))
        assert torch.equal(alone.view(torch.int32), got["seq_" + name].view(torch.int32))
    assert some_inf  # -inf propagated in some sequences, not in all
    assert float(np.float32(math.fsum([1e-3, 2.5]))) == float(SR.seq_sums(np.array([1e-3, 2.5], np.float32), [0, 2])[0])


def test_canaries_and_null_outputs(engine):
    import ctypes as C

    from genlm_backend_amd import _lib

    dev = engine.device
    n, V, n_seq = 5, 4097, 2
    x32 = _logits(3, n, V)
    x_d, xv = _dev_matrix(x32, torch.float32, dev)
    tok = _targets(3, x32)
    tok_d = torch.from_numpy(tok).to(dev)
    starts = torch.tensor([0, 2, 5], dtype=torch.int64, device=dev)
    bufs = {k: torch.full((64 + (n_seq if k.startswith("out_seq") else n) + 64,), CANARY, dtype=torch.float32, device=dev)
            for k in ("out_logp", "out_lse", "out_logZ", "out_logp_masked", "out_seq_logp", "out_seq_logZ", "out_seq_logp_masked")}

    def call(given):
        a = _lib.ScoreArgs()
        a.struct_size = C.sizeof(_lib.ScoreArgs)
        a.logits, a.dtype, a.ld = x_d.data_ptr(), _lib.F32, x_d.stride(0)
        a.n_rows, a.vocab, a.logit_scale, a.token = n, V, 1.0, tok_d.data_ptr()
        a.seq_start, a.n_seq = starts.data_ptr(), n_seq
        for k in given:
            setattr(a, k, bufs[k].data_ptr() + 64 * 4)
        assert engine.lib.glb_score_rows(C.byref(a), engine._stream()) == _lib.GLB_OK
        torch.cuda.synchronize(dev)

    call(("out_logp", "out_seq_logp"))  # the others null: not written
    for k, t in bufs.items():
        body = t[64:-64]
        assert bool((t[:64] == CANARY).all()) and bool((t[-64:] == CANARY).all()), k
        assert bool((body == CANARY).all()) == (k not in ("out_logp", "out_seq_logp")), k
    call(tuple(bufs))
    for k, t in bufs.items():
        assert bool((t[:64] == CANARY).all()) and bool((t[-64:] == CANARY).all()) and not bool((t[64:-64] == CANARY).any()), k
    ref = SR.score_rows(xv, tok, 1.0)
    _compare({nm: bufs["out_" + nm][64:-64] for nm in NAMES}, ref, "raw call")
    from genlm_backend_amd.engine import PreparedMasks

    with pytest.raises(TypeError, match="prepared"):
        engine.score_rows(x_d, tok_d, mask=PreparedMasks(None, 6, V, _lib.F32))
    with pytest.raises(ValueError, match="int32"):
        engine.score_rows(x_d, tok_d.long())
    with pytest.raises(ValueError, match="engine on"):
        engine.score_rows(x_d, tok_d.cpu())
    with pytest.raises(ValueError, match="want names"):
        engine.score_rows(x_d, tok_d, want=("entropy",))


# ---- the public interface ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(engine):
    from tests.test_wfsa_gpu import _model

    return _model(engine, 257)


PROMPTS = [[5], [6, 7], [9, 10, 11], [12, 13, 14, 15], [17, 3, 4, 5, 6, 8]]
CONTS = [[20, 21, 22, 23, 24, 25, 26], [], [30], [40, 41, 42, 43], [50, 51]]


def test_against_next_token_logprobs(model):
    s = model.batch_sequence_logprobs_sync(PROMPTS, CONTS)
    got = s.tolist()
    sums = s.logprobs.tolist()
    assert s.starts.tolist() == [0, 7, 7, 8, 12, 14]
    for i, (p, c) in enumerate(zip(PROMPTS, CONTS)):
        want = [float(model.batch_next_token_logprobs_sync([p + c[:t]])[0][c[t]]) for t in range(len(c))]
        assert len(got[i]) == len(c)
        for t in range(len(c)):
            assert abs(got[i][t] - want[t]) <= 1e-4, (i, t, got[i][t], want[t])
        assert abs(sums[i] - sum(want)) <= max(1, len(c)) * 1e-4
    assert sums[1] == 0.0


def test_temperature_and_chunks(model):
    s = model.batch_sequence_logprobs_sync(PROMPTS, CONTS, temperature=2.0)
    got = s.tolist()
    for i, (p, c) in enumerate(zip(PROMPTS, CONTS)):
        if not c:
            continue
        with torch.no_grad():
            logits = model.model(input_ids=torch.tensor([p + c], device=model.device)).logits[0].double()
        lp = torch.log_softmax(logits / 2, -1)
        for t, tk in enumerate(c):
            assert abs(got[i][t] - float(lp[len(p) - 1 + t, tk])) <= 1e-4, (i, t)
    keep = model.score_chunk_bytes
    try:
        model.score_chunk_bytes = 2 * 257 * 4  # two rows a chunk: boundaries inside sequences
        cut = model.batch_sequence_logprobs_sync(PROMPTS, CONTS, temperature=2.0)
    finally:
        model.score_chunk_bytes = keep
    assert torch.equal(cut.token_logprobs.view(torch.int32), s.token_logprobs.view(torch.int32))
    assert torch.equal(cut.logprobs.view(torch.int32), s.logprobs.view(torch.int32))


PATTERN = rb"(ab|cd)*[xyz]?"
WALK_PROMPTS = [[5, 17, 99][: 1 + i % 3] for i in range(8)]


def _tokens(texts):
    """Byte strings over the byte vocabulary (EOS is id 0, byte b is token b + 1)."""
    return [[b + 1 for b in s] for s in texts]


def _check_walk(model, constraint, conts, start, mask_of, step, n_inside=4):
    """Scores `conts` (the first `n_inside` in the language, the rest leaving it) behind WALK_PROMPTS under `constraint` and
    compares token_logZ / token_logprobs_masked with tests/score_ref.py fed the mask values `mask_of(state)` (float64 [V]) of a
    CPU reference walk `step(state, token)` from `start`.  The logits the reference reads come from the model's own forward,
    a second path to the same rows: 1e-4 (TOL of tests/test_host_gpu.py: one log-prob across two paths) on top of the
    kernel's 2e-4.  Returns the scores."""
    s = model.batch_sequence_logprobs_sync(WALK_PROMPTS, conts, constraint=constraint)
    lz, lpm, lp = s.tolist("token_logZ"), s.tolist("token_logprobs_masked"), s.tolist()
    worst = 0.0
    for i, (p, cn) in enumerate(zip(WALK_PROMPTS, conts)):
        with torch.no_grad():
            logits = model.model(input_ids=torch.tensor([p + cn], device=model.device)).logits[0].float().cpu().numpy()
        st, left = start, False
        for t, tk in enumerate(cn):
            want = SR.score_row(logits[len(p) - 1 + t], tk, 1.0, mask_of(st))
            assert np.isfinite(lp[i][t])
            for g, w in ((lz[i][t], want[2]), (lpm[i][t], want[3])):
                assert not np.isnan(g)
                if np.isneginf(w):
                    assert g == w, (i, t, g, w)
                else:
                    worst = max(worst, abs(g - w))
                    assert abs(g - w) <= 2e-4 + 1e-4, (i, t, g, w)
            left |= bool(np.isneginf(want[3]))
            assert not left or lpm[i][t] == -np.inf, (i, t)  # (-inf from the first forbidden token on)
            st = step(st, tk)
        assert np.isneginf(float(s.logprobs_masked[i])) == (i >= n_inside), i
        assert np.isfinite(float(s.logprobs[i]))
    print(f"{type(constraint).__name__}: max |err| = {worst:.3g}")
    return s


def test_device_constraint_on_a_finite_language(model):
    """`ByteDFA.from_strings`; and an evicting bank of working set + 2 rows gives the same bits."""
    from genlm_backend_amd.constraints import ByteDFA, DeviceConstraint
    from tests import dfa_ref
    from tests.test_wfsa_gpu import _byte_vocab

    dfa = ByteDFA.from_strings([b"abcd", b"cdabx", b"ab", b"z", b"cdab"])
    vocab = _byte_vocab()
    ref = dfa_ref.Ref(dfa.delta, dfa.accepting, dfa.start, vocab, 0, (0,))
    conts = _tokens([b"abcd", b"cdabx", b"ab", b"z", b"abq", b"ba", b"abxa", b"cdcc"])
    mask_of = lambda st: SR.mask_values(1, ref.mask(st) if st >= 0 else ref.row_dead(), 257)
    c = DeviceConstraint(model, dfa, vocab, 0, skip_ids=(0,))
    s = _check_walk(model, c, conts, ref.start, mask_of, ref.next)
    distinct = 0
    for t in range(max(map(len, conts))):
        distinct = max(distinct, len({ref.advance(ref.start, cn[:t]) for cn in conts if len(cn) > t}))
    small = DeviceConstraint(model, dfa, vocab, 0, skip_ids=(0,), mask_bank_bytes=(distinct + 2 + 2) * c.row_elems * 4, on_full="evict")
    assert small._evicting
    e = model.batch_sequence_logprobs_sync(WALK_PROMPTS, conts, constraint=small)
    for f in ("token_logprobs", "token_logZ", "token_logprobs_masked", "logZ", "logprobs_masked"):
        assert torch.equal(getattr(e, f).view(torch.int32), getattr(s, f).view(torch.int32)), f


def test_pda_constraint_on_balanced_brackets(model):
    """`PDAConstraint(BytePDA.dyck(...), max_depth=4)` against the configuration walk of tests/pda_ref.py."""
    from genlm_backend_amd.constraints import BytePDA, PDAConstraint
    from tests import pda_ref
    from tests.test_wfsa_gpu import _byte_vocab

    pda = BytePDA.dyck([(b"(", b")"), (b"[", b"]")], other=b"ab")
    vocab = _byte_vocab()
    ref = pda_ref.Ref(pda, vocab, 0, (0,), max_depth=4)
    conts = _tokens([b"(a)[b]", b"((([a])))", b"ab", b"([])", b"(]", b")", b"(((((", b"a(c"])  # (five deep: one too many)

    def mask_of(config):
        if config is None:
            return np.full(257, -np.inf)
        ok = np.array([ref.token(config, t) is not None for t in range(257)])
        ok[0] = ref.accepts(config)
        return np.where(ok, 0.0, -np.inf)

    step = lambda config, tk: None if config is None else ref.token(config, tk)
    c = PDAConstraint(model, pda, vocab, 0, skip_ids=(0,), max_depth=4)
    _check_walk(model, c, conts, ref.order[0], mask_of, step)


def test_weighted_lexicon_constraint(model):
    """A `ByteWFSA` lexicon: the bank is float rows (GLB_MASK_F32), logZ and the masked log-probabilities carry the weights of
    tests/wfsa_ref.py's rows."""
    from genlm_backend_amd.constraints import ByteWFSA, DeviceConstraint
    from tests import wfsa_ref
    from tests.test_wfsa_gpu import _byte_vocab

    lex = {b"abc": -0.5, b"ab": -2.0, b"abcab": -0.1, b"cab": -1.0, b"cabba": -3.0, b"bb": -0.7, b"bca": -1.3, b"ba": -0.2}
    wf = ByteWFSA.from_weighted_strings(lex)
    vocab = _byte_vocab()
    ref = wfsa_ref.WRef(wf.delta, wf.arc_logw, wf.final_logw, wf.start, vocab, 0, (0,))
    conts = _tokens([b"abc", b"cabba", b"bb", b"abcab", b"abd", b"cc", b"bbb", b"x"])
    mask_of = lambda st: (ref.row(st) if st >= 0 else ref.wrow_dead()).astype(np.float64)
    c = DeviceConstraint(model, wf, vocab, 0, skip_ids=(0,))
    assert c.weighted
    s = _check_walk(model, c, conts, ref.start, mask_of, ref.next)
    assert not torch.equal(s.token_logprobs_masked[:3], s.token_logprobs[:3])


def test_rescore_gives_the_runs_weights(model):
    """64 particles, 4 constrained steps without a proposal: the run's log-weights are the sums of the per-step logZ, which
    rescoring the particles under a fresh constraint of the same automaton recomputes."""
    from genlm_backend_amd.constraints import ByteDFA, DeviceConstraint
    from genlm_backend_amd.sis import DeviceSIS
    from tests.test_wfsa_gpu import _byte_vocab

    dfa = ByteDFA.from_regex(PATTERN)
    sis = DeviceSIS(model, 64, [5, 17, 99], 8, 0, seed=17, constraint=DeviceConstraint(model, dfa, _byte_vocab(), 0, skip_ids=(0,)))
    before = (sis.contexts.clone(), sis.lengths.clone(), sis.log_weights.clone())
    sis.run(max_steps=4)
    lw = sis.log_weights.clone()
    r = sis.rescore(constraint=DeviceConstraint(model, dfa, _byte_vocab(), 0, skip_ids=(0,)))
    assert torch.equal(sis.log_weights, lw) and not torch.equal(sis.lengths, before[1])  # (the run's state is untouched)
    gen = (sis.lengths - sis.prompt_len + (1 - sis.active)).cpu().numpy()  # (a particle that ended: its EOS is scored too)
    assert r.starts.cpu().numpy().tolist() == [0] + np.cumsum(gen).tolist() and gen.max() == 4
    lw, z = lw.cpu().numpy().astype(np.float64), r.logZ.cpu().numpy().astype(np.float64)
    fin = np.isfinite(lw)
    assert fin.sum() >= 32 and np.isfinite(z[fin]).all()
    print("rescore: max |logZ - log_weights| =", np.abs(lw[fin] - z[fin]).max())
    assert np.abs(lw[fin] - z[fin]).max() <= 4 * 2e-4
    other = sis.rescore(prompt_ids=[7, 8])
    assert other.token_logZ is None and torch.equal(other.starts, r.starts) and bool(torch.isfinite(other.logprobs).all())


def test_rescore_of_particles_made_to_end(model):
    """A run to the end with max_tokens = 3: particles out of tokens were served the EOS-only row; rescoring serves it too."""
    from genlm_backend_amd.constraints import ByteDFA, DeviceConstraint
    from genlm_backend_amd.sis import DeviceSIS
    from tests.test_wfsa_gpu import _byte_vocab

    dfa = ByteDFA.from_regex(PATTERN)
    sis = DeviceSIS(model, 64, [5, 17, 99], 3, 0, seed=5, constraint=DeviceConstraint(model, dfa, _byte_vocab(), 0, skip_ids=(0,)))
    sis.run()
    assert int(sis.active.sum().item()) == 0
    r = sis.rescore(constraint=DeviceConstraint(model, dfa, _byte_vocab(), 0, skip_ids=(0,)))
    gen = (sis.lengths - sis.prompt_len).cpu().numpy()
    lw, z = sis.log_weights.cpu().numpy().astype(np.float64), r.logZ.cpu().numpy().astype(np.float64)
    fin = np.isfinite(lw)
    assert (fin & (gen == 3)).sum() >= 8  # particles that were made to end, and ended
    assert np.isfinite(z[fin]).all()
    print("rescore at max_tokens: max |logZ - log_weights| =", np.abs(lw[fin] - z[fin]).max())
    assert np.abs(lw[fin] - z[fin]).max() <= 4 * 2e-4  # (four steps a particle at the most: three tokens and the EOS)


def test_score_seq_sums_refuses_a_strided_view(engine):
    dev = engine.device
    v = torch.zeros(8, dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match="contiguous"):
        engine.score_seq_sums(v[::2], torch.tensor([0, 4], dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="positive and finite"):
        engine.score_rows(v[None], torch.zeros(1, dtype=torch.int32, device=dev), logit_scale=0.0)
