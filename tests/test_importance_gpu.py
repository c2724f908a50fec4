"""glb_importance_step on the GPU against the float64 reference (tests/importance_ref.py): every particle's token inside the
two-stage CDF intervals its Philox words select, dlogw / lse / logZ within 2e-4, the fused step's logZ with no proposal,
results bit for bit however the call is cut, the distribution of 65536 draws, canaries, and `DeviceSIS` with a tempered
proposal and with a second model as proposal.

Tolerances (derived, not measured).  CDF intervals are widened by EPS = 1e-5 of the stage's mass: a term is within 2.7e-6
(the hardware exponential used here is closer), sixteen float32 additions add at most 1e-6, EPS is three times
their sum.  Log-sum-exps: 2e-4 = two of them at the library's 1e-4 contract."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import importance_ref as IR

pytestmark = pytest.mark.gpu

EPS = 1e-5
TOL = 2e-4
CANARY = 12345.0
NAN = float("nan")
_TORCH = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MASKS = ("none", "bits_particle", "bits_row", "f32_row")


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def _logits(seed, n_rows, V):
    """p, q float32 [n_rows, V]: 2 N(0, 1) clipped to 30; row r has -inf entries in p (r % 3 == 0), in q (1), in both (2)."""
    rs = np.random.default_rng(seed)
    p = np.clip(2 * rs.standard_normal((n_rows, V)), -30, 30).astype(np.float32)
    q = np.clip(2 * rs.standard_normal((n_rows, V)), -30, 30).astype(np.float32)
    for r in range(n_rows):
        if r % 3 in (0, 2):
            p[r, rs.random(V) < 0.1] = -np.inf
        if r % 3 in (1, 2):
            q[r, rs.random(V) < 0.1] = -np.inf
    return p, q


def _mask_table(seed, V):
    """bool [6, V] allowed: two random rows, a row allowing nothing, one allowing one token, one with a whole chunk forbidden
    (the first 4096 tokens; the first half of a shorter row), one allowing only the tail of the last chunk."""
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


def _dev_matrix(x32, dtype, dev, pad=13):
    """x as a device matrix of `dtype` with pitch V + pad and NaN in the padding; and its exact values as float64."""
    n, V = x32.shape
    t = torch.full((n, V + pad), NAN, dtype=dtype, device=dev)
    t[:, :V] = torch.from_numpy(x32).to(dev).to(dtype)
    view = t[:, :V]
    host = view.float().cpu().numpy()  # (16-bit -> float32 is exact)
    return view, host


class Case:
    """One call's inputs on the device, and the float64 reference row of every (logits row, mask row) pair on demand."""

    def __init__(self, dev, seed, V, n_rows, n, dts, mask, scale, with_q=True):
        rs = np.random.default_rng(seed + 7)
        self.V, self.n_rows, self.n, self.scale, self.mask = V, n_rows, n, scale, mask
        p32, q32 = _logits(seed, n_rows, V)
        self.p_d, self.p_h = _dev_matrix(p32, _TORCH[dts[0]], dev)
        self.q_d, self.q_h = _dev_matrix(q32, _TORCH[dts[1]], dev) if with_q else (None, self.p_h)
        self.row_of = np.sort(rs.integers(0, n_rows, n)).astype(np.int32)  # (sorted: a row's particles are consecutive)
        self.ok = _mask_table(seed, V)
        self.kw, self.mask_of_particle = {}, np.zeros(n, np.int64)
        if mask == "bits_particle":
            mid = rs.integers(0, 6, n).astype(np.int32)
            self.kw = dict(mask_kind=1, mask=torch.from_numpy(_bits(self.ok)).to(dev)[:, :(V + 31) // 32 + 1],
                           mask_id=torch.from_numpy(mid).to(dev))
            self.mask_of_particle = mid
        elif mask in ("bits_row", "f32_row"):
            rid = rs.integers(0, 6, n_rows).astype(np.int32)
            if mask == "bits_row":
                tab, kind = torch.from_numpy(_bits(self.ok)).to(dev)[:, :(V + 31) // 32 + 1], 1
            else:
                self.weights = np.where(self.ok, rs.standard_normal((6, V)).astype(np.float32), np.float32(-np.inf))
                big = torch.full((6, V + 5), NAN, dtype=torch.float32, device=dev)
                big[:, :V] = torch.from_numpy(self.weights).to(dev)
                tab, kind = big[:, :V], 2
            self.kw = dict(mask_kind=kind, mask=tab, row_mask_id=torch.from_numpy(rid).to(dev))
            self.mask_of_particle = rid[self.row_of]
        self.row_of_d = torch.from_numpy(self.row_of).to(dev)
        self._rows = {}

    def ref(self, i):
        r, m = int(self.row_of[i]), int(self.mask_of_particle[i])
        if (r, m) not in self._rows:
            if self.mask == "none":
                mv = np.zeros(self.V)
            elif self.mask == "f32_row":
                mv = self.weights[m].astype(np.float64)
            else:
                mv = np.where(self.ok[m], 0.0, -np.inf)
            y = IR.proposal_values(self.q_h[r], self.scale)
            self._rows[(r, m)] = IR.Row(self.p_h[r].astype(np.float64), y, mv)
        return self._rows[(r, m)]


def _same_inf(got, want):
    return np.isinf(got) == np.isinf(want) and (not np.isinf(want) or np.sign(got) == np.sign(want))


def _check(case, out, seed, offset, base=0, worst=None):
    """Every particle of a call against the reference.  Returns the number of particles with a token."""
    dlogw, tok, lse, logZq = (t.cpu().numpy() for t in out)
    drawn = 0
    for i in range(case.n):
        r = case.ref(i)
        t = int(tok[i])
        want_d = -np.inf
        if r.empty:
            assert t == -1, (i, t)
        else:
            assert 0 <= t < case.V and r.qt[t] > 0 and np.isfinite(r.m[t]), (i, t)
            u1, u2 = IR.uniforms(seed, offset, base + i)
            lo, hi = r.chunk_interval(t // IR.CHUNK)
            assert lo - EPS <= u1 <= hi + EPS, ("chunk", i, t, u1, lo, hi)
            lo, hi = r.elem_interval(t)
            assert lo - EPS <= u2 <= hi + EPS, ("element", i, t, u2, lo, hi)
            want_d = r.dlogw(t)
            drawn += 1
        for name, got, want in (("dlogw", dlogw[i], want_d), ("lse_target", lse[i], r.lse_p), ("logZ_proposal", logZq[i], r.logZ_proposal)):
            assert _same_inf(got, want), (name, i, got, want)
            if np.isfinite(want):
                assert abs(got - want) <= TOL, (name, i, got, want)
                if worst is not None:
                    worst[name] = max(worst.get(name, 0.0), abs(float(got) - want))
    return drawn


def _call(engine, case, seed, offset, **over):
    kw = dict(proposal_scale=case.scale, vocab=case.V, row_of=case.row_of_d, seed=seed, offset=offset, want_lse=True,
              want_logZ_proposal=True, **case.kw)
    kw.update(over)
    return engine.importance_step(case.p_d, case.q_d, **kw)


_CASES = []
for _iv, _V in enumerate((1, 33, 4095, 4096, 4097, 8200)):
    for _k, _dts in enumerate((("f32", "f32"), ("bf16", "bf16"), ("f32", "bf16"), ("f16", "f32"))):
        _CASES.append(pytest.param(_V, (1, 3, 65)[(_iv + _k) % 3], (1, 64, 65, 1000)[(_iv + 2 * _k + _k // 2) % 4], _dts,
                                   MASKS[(_iv + _k) % 4], (1.0, 0.7)[_k % 2],
                                   id=f"V{_V}-{_dts[0]}-{_dts[1]}-{MASKS[(_iv + _k) % 4]}"))
_WORST = {}


@pytest.mark.parametrize("V,n_rows,n,dts,mask,scale", _CASES)
def test_every_particle_against_float64(engine, V, n_rows, n, dts, mask, scale):
    case = Case(engine.device, V * 31 + n, V, n_rows, n, dts, mask, scale)
    seed, offset = (5 << 32) | (V + 1), (3 << 32) | n
    out = _call(engine, case, seed, offset)
    torch.cuda.synchronize()
    drawn = _check(case, out, seed, offset, worst=_WORST)
    print(f"V={V} rows={n_rows} n={n} {dts} {mask}: {drawn} drawn; largest errors so far {_WORST}")
    assert mask != "none" or drawn > 0 or V == 1


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("dts", [("f32", "f32"), ("bf16", "f16")], ids=["f32", "bf16-f16"])
def test_every_mask_kind_over_two_chunks_and_a_tail(engine, mask, dts):
    """V = 8200, 65 rows, 1000 particles: every special mask row (nothing, one token, a chunk forbidden, only the tail) meets
    rows with -inf entries; and typical token masses are large against EPS, so a walk that is off by one fails."""
    case = Case(engine.device, 99, 8200, 65, 1000, dts, mask, 1.0)
    r = case.ref(0)
    assert r.qt[r.qt >= 1e-4].sum() > 0.5 or r.empty  # most draws land on tokens a hundred times EPS and more
    out = _call(engine, case, 77, 5)
    torch.cuda.synchronize()
    drawn = _check(case, out, 77, 5, worst=_WORST)
    tok = out[1].cpu().numpy()
    empties = sum(case.ref(i).empty for i in range(case.n))
    assert drawn + empties == case.n and (tok == -1).sum() == empties
    if mask != "none":
        assert empties > 0 and {int(m) for m in case.mask_of_particle} == set(range(6))
    print(f"{mask} {dts}: {drawn} drawn, {empties} empty; largest errors so far {_WORST}")


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_no_proposal_gives_the_fused_steps_logZ(engine, dt):
    case = Case(engine.device, 5, 8200, 65, 1000, (dt, dt), "bits_particle", 1.0, with_q=False)
    dlogw, tok, _, _ = _call(engine, case, 9, 2)
    logZ, _, tok_f = engine.step(case.p_d, vocab=case.V, row_of=case.row_of_d, rng_mode=1, seed=9, offset=2,
                                 **{**case.kw, "mask": case.kw["mask"].contiguous()})
    torch.cuda.synchronize()
    engine.check()
    a, b = dlogw.cpu().numpy(), logZ.cpu().numpy()
    assert np.array_equal(np.isinf(a), np.isinf(b)) and np.array_equal(tok.cpu().numpy() == -1, tok_f.cpu().numpy() == -1)
    fin = np.isfinite(b)
    print(f"{dt}: max |dlogw - logZ| = {np.abs(a[fin] - b[fin]).max():.3e} over {fin.sum()} particles")
    assert fin.sum() > 500 and np.abs(a[fin] - b[fin]).max() <= TOL
    _check(case, _call(engine, case, 9, 2), 9, 2)


def _bytes(out):
    return [None if t is None else t.cpu().numpy().tobytes() for t in out]


@pytest.mark.parametrize("mask", ["none", "bits_particle", "f32_row"])
def test_shards_with_particle_base_equal_one_call(engine, mask):
    case = Case(engine.device, 21, 8200, 65, 1000, ("f32", "bf16"), mask, 0.8)
    whole = _bytes(_call(engine, case, 4, 6, particle_base=1 << 33))
    parts = []
    for s in range(4):
        sl = slice(250 * s, 250 * s + 250)
        over = dict(row_of=case.row_of_d[sl].contiguous(), particle_base=(1 << 33) + 250 * s)
        if "mask_id" in case.kw:
            over["mask_id"] = case.kw["mask_id"][sl].contiguous()
        parts.append([t.cpu().numpy() for t in _call(engine, case, 4, 6, **over)])
    for k in range(4):
        assert np.concatenate([p[k] for p in parts]).tobytes() == whole[k], k


@pytest.mark.parametrize("mask", ["none", "bits_row"])
def test_a_row_alone_equals_the_row_among_65(engine, mask):
    case = Case(engine.device, 22, 4097, 65, 1000, ("bf16", "f32"), mask, 1.0)
    among = [t.cpu().numpy() for t in _call(engine, case, 8, 1)]
    r = 40
    idx = np.nonzero(case.row_of == r)[0]
    assert len(idx) > 3 and idx[-1] - idx[0] == len(idx) - 1  # (row_of is sorted: a row's particles are consecutive)
    over = dict(row_of=torch.zeros(len(idx), dtype=torch.int32, device=engine.device), particle_base=int(idx[0]))
    if "row_mask_id" in case.kw:
        over["row_mask_id"] = case.kw["row_mask_id"][r:r + 1].contiguous()
    alone = engine.importance_step(case.p_d[r:r + 1], case.q_d[r:r + 1], proposal_scale=1.0, vocab=case.V, seed=8, offset=1,
                                   want_lse=True, want_logZ_proposal=True, **{**case.kw, **over})
    for k in range(4):
        assert alone[k].cpu().numpy().tobytes() == among[k][idx].tobytes(), k


@pytest.mark.parametrize("mask", ["none", "bits_row"])
def test_a_shared_row_equals_private_copies(engine, mask):
    dev, n = engine.device, 700
    case = Case(dev, 23, 8200, 1, n, ("f32", "f32"), mask, 0.9)
    shared = _bytes(_call(engine, case, 3, 3))
    over = dict(row_of=torch.arange(n, dtype=torch.int32, device=dev))
    if "row_mask_id" in case.kw:
        over["row_mask_id"] = case.kw["row_mask_id"].repeat(n)
    private = engine.importance_step(case.p_d.repeat(n, 1), case.q_d.repeat(n, 1), proposal_scale=0.9, vocab=case.V, seed=3,
                                     offset=3, want_lse=True, want_logZ_proposal=True, **{**case.kw, **over})
    assert _bytes(private) == shared


# ---- distribution --------------------------------------------------------------------------------------------------------------
def _small_row(dev, with_q):
    rs = np.random.default_rng(37)
    V, n = 37, 65536
    p = (2 * rs.standard_normal((1, V))).astype(np.float32)
    q = (2 * rs.standard_normal((1, V))).astype(np.float32)
    ok = np.ones((1, V), bool)
    ok[0, rs.choice(V, 9, replace=False)] = False
    row = IR.Row(p[0].astype(np.float64), (q if with_q else p)[0].astype(np.float64), np.where(ok[0], 0.0, -np.inf))
    kw = dict(mask_kind=1, mask=torch.from_numpy(_bits(ok, 0)).to(dev), row_mask_id=torch.zeros(1, dtype=torch.int32, device=dev),
              row_of=torch.zeros(n, dtype=torch.int32, device=dev), seed=123, offset=1)
    return torch.from_numpy(p).to(dev), torch.from_numpy(q).to(dev) if with_q else None, row, ok[0], kw, n


def test_65536_draws_follow_the_proposal(engine):
    p, _, row, ok, kw, n = _small_row(engine.device, False)
    _, tok, _ = engine.importance_step(p, None, **kw)
    counts = np.bincount(tok.cpu().numpy(), minlength=37)
    assert counts.sum() == n and counts[~ok].sum() == 0
    checked = 0
    for j in np.nonzero(ok)[0]:
        e = n * row.qt[j]
        if e >= 50:
            assert abs(counts[j] - e) <= 5 * np.sqrt(e * (1 - row.qt[j])), (j, counts[j], e)
            checked += 1
    assert checked >= 15


def test_mean_weight_estimates_the_targets_mass(engine):
    p, q, row, ok, kw, n = _small_row(engine.device, True)
    dlogw, tok, _ = engine.importance_step(p, q, **kw)
    w = np.exp(dlogw.cpu().numpy().astype(np.float64))
    Z = row.target_mass()
    live = row.qt > 0
    var = float(np.sum(row.qt[live] * np.exp(row.dlogw()[live]) ** 2) - Z * Z)
    se = np.sqrt(var / n)
    print(f"mean exp(dlogw) = {w.mean():.6f}, Z = {Z:.6f}, standard error {se:.2e}")
    assert 0 < Z < 1 and abs(w.mean() - Z) <= 5 * se
    assert bool(ok[tok.cpu().numpy()].all())  # forbidden tokens never appear


# ---- isolation -----------------------------------------------------------------------------------------------------------------
def test_canaries_and_null_outputs(engine):
    from genlm_backend_amd import _lib

    dev = engine.device
    case = Case(dev, 31, 4097, 3, 65, ("f32", "f16"), "bits_particle", 1.0)
    n = case.n
    need = engine.lib.glb_importance_workspace_bytes(n, 3, case.V)
    assert need == n * 2 * 64
    ws = torch.full((need // 4 + 64,), CANARY, dtype=torch.float32, device=dev)
    outs = {k: torch.full((n + 16,), CANARY if k != "out_token" else 12345, dtype=torch.int32 if k == "out_token" else torch.float32,
                          device=dev) for k in ("out_token", "out_dlogw", "out_lse_target", "out_logZ_proposal")}

    def run(names):
        a = _lib.ImportanceArgs()
        a.struct_size = C.sizeof(_lib.ImportanceArgs)
        a.target, a.target_dtype, a.ld_p = case.p_d.data_ptr(), _lib.F32, case.p_d.stride(0)
        a.proposal, a.proposal_dtype, a.ld_q = case.q_d.data_ptr(), _lib.F16, case.q_d.stride(0)
        a.n_rows, a.vocab, a.proposal_scale, a.n_particles = 3, case.V, 1.0, n
        a.row_of = case.row_of_d.data_ptr()
        m = case.kw["mask"]
        a.mask_kind, a.mask, a.mask_ld, a.n_masks = 1, m.data_ptr(), m.stride(0), m.shape[0]
        a.mask_id = case.kw["mask_id"].data_ptr()
        a.seed, a.offset = 1, 2
        for k in names:
            setattr(a, k, outs[k].data_ptr())
        a.workspace, a.workspace_bytes = ws.data_ptr(), need
        _lib.check(engine.lib.glb_importance_step(C.byref(a), engine._stream()))
        torch.cuda.synchronize()

    run(["out_token"])
    assert all(bool((outs[k] == CANARY).all()) for k in outs if k != "out_token")  # outputs passed as null: not written
    tok_only = outs["out_token"][:n].clone()
    run(list(outs))
    assert torch.equal(outs["out_token"][:n], tok_only)
    for k, t in outs.items():
        assert bool((t[n:] == (12345 if k == "out_token" else CANARY)).all()), k
    assert bool((ws[need // 4:] == CANARY).all()) and not bool((ws[:need // 4] == CANARY).all())
    _check(case, (outs["out_dlogw"][:n], outs["out_token"][:n], outs["out_lse_target"][:n], outs["out_logZ_proposal"][:n]), 1, 2)
    # too small a workspace is refused, nothing launched
    a_ws = need - 64
    a = _lib.ImportanceArgs()
    a.struct_size = C.sizeof(_lib.ImportanceArgs)
    a.target, a.target_dtype, a.ld_p = case.p_d.data_ptr(), _lib.F32, case.p_d.stride(0)
    a.n_rows, a.vocab, a.proposal_scale, a.n_particles, a.row_of = 3, case.V, 1.0, n, case.row_of_d.data_ptr()
    a.mask_kind, a.mask, a.mask_ld, a.n_masks = 1, case.kw["mask"].data_ptr(), case.kw["mask"].stride(0), 6
    a.mask_id = case.kw["mask_id"].data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), a_ws
    assert engine.lib.glb_importance_step(C.byref(a), engine._stream()) == _lib.GLB_ENOSPC
    from genlm_backend_amd.engine import PreparedMasks

    with pytest.raises(TypeError, match="prepared"):
        engine.importance_step(case.p_d, None, vocab=case.V, mask=PreparedMasks(None, 6, case.V, _lib.F32))


# ---- DeviceSIS -----------------------------------------------------------------------------------------------------------------
PROMPT = [5, 17, 99]
PATTERN = rb"(ab|cd)*[xyz]?"
N_SIS, MAX_TOKENS = 512, 6


@pytest.fixture(scope="module")
def models(engine):
    from transformers import GPT2Config

    from genlm_backend_amd.llm import AsyncAmdLM
    from tests.test_wfsa_gpu import Tok, _model

    target = _model(engine, 257)
    cfg = GPT2Config(vocab_size=257, n_positions=64, n_embd=64, n_layer=2, n_head=4, bos_token_id=0, eos_token_id=0)
    other = AsyncAmdLM.from_config(cfg, None, device=engine.device, seed=11, engine=engine, batch_size=64, timeout=0.02)
    other.tokenizer = Tok()
    return target, other


def _run(models, **kw):
    from genlm_backend_amd.constraints import ByteDFA, DeviceConstraint
    from genlm_backend_amd.sis import DeviceSIS
    from tests.test_wfsa_gpu import _byte_vocab

    target, _ = models
    c = DeviceConstraint(target, ByteDFA.from_regex(PATTERN), _byte_vocab(), 0, skip_ids=(0,))
    sis = DeviceSIS(target, N_SIS, PROMPT, MAX_TOKENS, 0, seed=17, constraint=c, **kw)
    sis.run()
    ctx, lw = sis.results()
    assert int(sis.active.sum().item()) == 0
    return ctx, lw


def _all_logprobs(llm, seqs):
    """float64 log-softmax rows [len(seqs), L, V] of a plain forward over prompt + tokens, right-padded (a causal model: the
    padding changes nothing before it)."""
    L = len(PROMPT) + MAX_TOKENS
    ids = torch.zeros((len(seqs), L), dtype=torch.long, device=llm.device)
    for i, s in enumerate(seqs):
        ids[i, :len(PROMPT) + len(s)] = torch.tensor(PROMPT + list(s))
    with torch.no_grad():
        h = llm._body(input_ids=ids, use_cache=False).last_hidden_state
        return llm._lm_head(h).to(torch.float64).cpu().numpy()


def _recompute(models, ctx, temperature, use_other):
    """sum_t [log p_t(tok) - log qt_t(tok)] of every particle from its own tokens, float64."""
    from genlm_backend_amd.constraints import ByteDFA

    target, other = models
    dfa = ByteDFA.from_regex(PATTERN)
    seqs = sorted({tuple(int(t) for t in cx) for cx in ctx})
    lp = _all_logprobs(target, seqs)
    lq = _all_logprobs(other, seqs) if use_other else lp
    total = {}
    for k, s in enumerate(seqs):
        state, w = dfa.start, 0.0
        for t in range(len(s) + 1):
            at = len(PROMPT) - 1 + t
            allowed = np.zeros(257, bool)
            if t < MAX_TOKENS:
                allowed[1:] = dfa.delta[state] >= 0
            allowed[0] = bool(dfa.accepting[state])
            tok = s[t] if t < len(s) else 0
            assert allowed[tok]
            p = lp[k, at] - IR.lse(lp[k, at])
            y = np.float32(1.0 / temperature) * lq[k, at].astype(np.float32) if temperature != 1.0 else lq[k, at]
            z = np.where(allowed, y.astype(np.float64), -np.inf)
            w += p[tok] - (z[tok] - IR.lse(z))
            if tok != 0:
                state = int(dfa.delta[state, tok - 1])
        total[s] = w
    return np.array([total[tuple(int(t) for t in cx)] for cx in ctx])


def _log_mean_exp(lw):
    lw = lw.astype(np.float64)
    m = lw.max()
    w = np.exp(lw - m)
    return m + np.log(w.mean()), w.std(ddof=1) / (w.mean() * np.sqrt(len(w)))


def test_device_sis_with_a_proposal(models):
    from genlm_backend_amd.constraints import ByteDFA

    dfa = ByteDFA.from_regex(PATTERN)
    plain_ctx, plain_lw = _run(models)
    none_ctx, none_lw = _run(models, proposal_temperature=None, proposal=None)
    assert none_ctx == plain_ctx and none_lw.tobytes() == plain_lw.tobytes()
    est0, se0 = _log_mean_exp(plain_lw)
    for name, kw, T, use_other in (("tempered", dict(proposal_temperature=2.0), 2.0, False),
                                   ("second model", dict(proposal=models[1]), 1.0, True)):
        ctx, lw = _run(models, **kw)
        assert np.isfinite(lw).all()
        assert all(dfa.accepts(bytes(t - 1 for t in cx)) and len(cx) <= MAX_TOKENS for cx in ctx)
        want = _recompute(models, ctx, T, use_other)
        err = np.abs(lw.astype(np.float64) - want).max()
        est, se = _log_mean_exp(lw)
        print(f"{name}: {len({tuple(c) for c in ctx})} distinct sequences, max |log-weight - float64| = {err:.3e}; "
              f"log mean weight {est:.4f} +- {se:.4f} against {est0:.4f} +- {se0:.4f} without a proposal")
        assert err <= 1e-3
        assert abs(est - est0) <= 5 * np.sqrt(se * se + se0 * se0)
        assert ctx != plain_ctx  # (another draw than the target's own)
