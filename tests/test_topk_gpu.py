"""glb_topk_rows / glb_beam_select (HipEngine.topk_rows / beam_select) on the GPU against tests/topk_ref.py.

The token ids are exact: a key is one rounded multiply and one rounded add, which the reference restates in float32, and the
selection compares keys and indices only - so `token` must equal the reference's, -1 included, and -inf must sit where the
reference has it.  Tolerances of the floats (tests/test_score_gpu.py's derivation): a log-sum-exp is within 1e-4 of the exact
value of the widened inputs (the library's contract), so `lse` is held to 1e-4 and every output that is a difference involving
two log-sum-exps or a log-sum-exp and a float32 key (`logp`, `logp_masked`, `logZ`) to 2e-4.  No NaN anywhere.
glb_beam_select's value is one float32 addition: its three outputs must equal the reference's exactly."""
import numpy as np
import pytest
import torch

from tests import topk_ref as TR

pytestmark = pytest.mark.gpu

NAMES = ("logp", "logp_masked", "lse", "logZ")
TOLS = dict(logp=2e-4, logp_masked=2e-4, lse=1e-4, logZ=2e-4)
NAN = float("nan")
CANARY = 12345.0
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
KS = (1, 5, 64)


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


def _dev_matrix(x32, dtype, dev, pad=5):
    """x as a device matrix of `dtype` with pitch V + pad, NaN in the padding, its base one element past the allocation's
    (no 16-byte alignment anywhere); and the values it holds, float32 (exact)."""
    n, V = x32.shape
    flat = torch.full((n * (V + pad) + 1,), NAN, dtype=dtype, device=dev)
    t = flat[1:].view(n, V + pad)
    t[:, :V] = torch.from_numpy(x32).to(dev).to(dtype)
    return t[:, :V], t[:, :V].float().cpu().numpy()


def _mask_table(seed, V):
    """bool [6, V] allowed (tests/test_score_gpu.py's table): two random rows, a row allowing nothing, one allowing one token,
    one with a whole chunk forbidden (the first 4096 tokens; the first half of a shorter row), one allowing only the tail of
    the last chunk."""
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


def _compare(got, ref, k, what):
    """`ref` was made with k = 64: its first k columns are the reference for any smaller k."""
    tok = got["token"].cpu().numpy()
    want = ref["token"][:, :k]
    assert tok.dtype == np.int32 and tok.shape == want.shape
    bad = np.argwhere(tok != want)
    assert len(bad) == 0, (what, "token", bad[:5].tolist(), tok[tuple(bad[0])], want[tuple(bad[0])])
    for name in NAMES:
        if name not in got:
            continue
        g = got[name].cpu().numpy().astype(np.float64)
        r = ref[name][:, :k] if name.startswith("logp") else ref[name]
        assert g.shape == r.shape, (what, name)
        assert not np.isnan(g).any(), (what, name)
        inf = np.isneginf(r)
        assert np.array_equal(np.isneginf(g), inf), (what, name, np.argwhere(np.isneginf(g) != inf)[:5].tolist())
        err = np.abs(g[~inf] - r[~inf]).max() if (~inf).any() else 0.0
        print(f"{what} {name}: max err {err:.3g}")
        assert err <= TOLS[name], (what, name, err)
        if name.startswith("logp"):
            assert np.array_equal(inf, want < 0), (what, name)  # -inf exactly where the token is -1


@pytest.mark.parametrize("n", [1, 3, 67])
@pytest.mark.parametrize("V", [1, 33, 4095, 4096, 4097, 8200, 16500])
def test_values(engine, V, n):
    """Every dtype, k in {1, 5, 64}; no mask at scale 1, the six-row table as bit rows at scale 0.5 and as float rows with
    weights at scale 1 / 0.7 (ids 0..5 round the rows, then one out of range on either side)."""
    dev = engine.device
    x32 = _logits(V * 131 + n, n, V)
    ok = _mask_table(V, V)
    ids = (np.arange(n) % 6).astype(np.int32)
    if n > 8:
        ids[7], ids[8] = 6, -1
    ids_d = torch.from_numpy(ids).to(dev)
    tables = {1: (_bits(ok), _bits(ok, 0)), 2: (_floats(V, ok), _floats(V, ok, 0))}
    for dtype in DTYPES:
        x_d, xv = _dev_matrix(x32, dtype, dev)
        for kind, scale in ((0, 1.0), (1, 0.5), (2, 1 / 0.7)):
            kw, ref_kw = {}, {}
            if kind:
                padded, plain = tables[kind]
                tab_d = torch.from_numpy(padded).to(dev)
                kw = dict(mask_kind=kind, mask=tab_d[:, :plain.shape[1] + 1], row_mask_id=ids_d)  # (a pitch beyond the row)
                ref_kw = dict(kind=kind, table=plain, row_mask_id=ids)
            ref = TR.topk_rows(xv, 64, scale, **ref_kw)
            for k in KS:
                got = engine.topk_rows(x_d, k, logit_scale=scale, want=NAMES, **kw)
                _compare(got, ref, k, f"V={V} n={n} {dtype} k={k} kind={kind}")
                if not kind:
                    assert torch.equal(got["logp"].view(torch.int32), got["logp_masked"].view(torch.int32))


def _hostile(V):
    """float32 [11, V] and what each row is."""
    rs = np.random.default_rng(V)
    names = ["all equal", "ascending", "descending", "8 levels", "all -inf", "one finite", "3 finite", "40 finite",
             "-0 before +0", "+0 before -0", "random"]
    x = np.zeros((len(names), V), np.float32)
    x[0] = 0.75
    x[1] = (np.arange(V) - V // 2) * np.float32(1 / 1024)
    x[2] = x[1][::-1]
    x[3] = rs.integers(0, 8, V).astype(np.float32) - 4
    x[4] = -np.inf
    x[5] = -np.inf
    x[5, V - 1] = -3.0
    x[6] = -np.inf
    x[6, rs.choice(V, min(3, V), replace=False)] = np.float32(1.25)
    x[7] = -np.inf
    x[7, rs.choice(V, min(40, V), replace=False)] = rs.integers(0, 4, min(40, V)).astype(np.float32)
    x[8] = -1.0
    x[9] = -1.0
    if V >= 3:
        x[8, V // 3], x[8, 2 * V // 3] = -0.0, 0.0
        x[9, V // 3], x[9, 2 * V // 3] = 0.0, -0.0
    x[10] = rs.standard_normal(V)
    return x, names


@pytest.mark.parametrize("V", [33, 4097, 16500])
def test_hostile_rows(engine, V):
    """Ties across chunk and wave boundaries, sorted rows, rows with fewer than k finite keys, rows with fewer than k allowed
    tokens (a bit mask of 3 tokens; the table's one-token and empty rows), signed zeros."""
    dev = engine.device
    x32, names = _hostile(V)
    n = len(names)
    few = np.zeros((1, V), bool)
    few[0, [0, V // 2, V - 1]] = True
    ok = np.concatenate([_mask_table(V, V), few])
    ids = (np.arange(n) % 7).astype(np.int32)
    ids[[0, 1, 3]] = 6  # the tied and the sorted rows under the three-token mask
    bits_d, ids_d = torch.from_numpy(_bits(ok)).to(dev), torch.from_numpy(ids).to(dev)
    for dtype in DTYPES:
        x_d, xv = _dev_matrix(x32, dtype, dev)
        ref = TR.topk_rows(xv, 64)
        ref_m = TR.topk_rows(xv, 64, 1.0, 1, _bits(ok, 0), ids)
        assert (ref["token"][4] == -1).all() and (ref["token"][5] == [V - 1] + [-1] * 63).all()
        if V >= 3:
            assert ref["token"][8, 0] == V // 3 and ref["token"][9, 0] == V // 3  # (-0 equals +0: the lower index first)
            assert sorted(ref_m["token"][0][:3]) == [0, V // 2, V - 1] and ref_m["token"][0][3] == -1
        for k in KS:
            _compare(engine.topk_rows(x_d, k, want=NAMES), ref, k, f"hostile V={V} {dtype} k={k}")
            got = engine.topk_rows(x_d, k, mask_kind=1, mask=bits_d, row_mask_id=ids_d, want=NAMES)
            _compare(got, ref_m, k, f"hostile V={V} {dtype} k={k} bits")


@pytest.mark.parametrize("shape,dtype", [((4, 50257), torch.float32), ((2, 128256), torch.bfloat16)])
def test_values_at_model_vocabularies(engine, shape, dtype):
    dev = engine.device
    n, V = shape
    x32 = _logits(V, n, V)
    x_d, xv = _dev_matrix(x32, dtype, dev)
    ok = _mask_table(V, V)[[0, 4, 5, 3][:n]]
    got = engine.topk_rows(x_d, 64, logit_scale=0.5, mask_kind=1, mask=torch.from_numpy(_bits(ok)).to(dev), want=NAMES)  # (no ids)
    _compare(got, TR.topk_rows(xv, 64, 0.5, 1, _bits(ok, 0)), 64, f"{shape} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_cut_invariance(engine, dtype):
    """67 rows in one call, in calls of 1 + 66, and in 67 calls of one row: the same bytes."""
    dev = engine.device
    n, V, k = 67, 8200, 5
    x32 = _logits(99, n, V)
    x32[5] = np.round(x32[5])  # (ties)
    x_d, _ = _dev_matrix(x32, dtype, dev)
    ids = torch.from_numpy((np.arange(n) % 6).astype(np.int32)).to(dev)
    bits = torch.from_numpy(_bits(_mask_table(V, V))).to(dev)

    def run(a, b):
        return engine.topk_rows(x_d[a:b], k, logit_scale=0.5, mask_kind=1, mask=bits, row_mask_id=ids[a:b].contiguous(), want=NAMES)

    whole = run(0, n)
    split = [run(0, 1), run(1, n)]
    single = [run(r, r + 1) for r in range(n)]
    for name in ("token",) + NAMES:
        w = whole[name].view(torch.int32)
        assert torch.equal(w, torch.cat([p[name] for p in split]).view(torch.int32)), name
        assert torch.equal(w, torch.cat([p[name] for p in single]).view(torch.int32)), name


def test_under_stream_capture(engine):
    """A graph of this one launch: its replay gives the eager call's bytes."""
    dev = engine.device
    n, V, k = 9, 8200, 5
    x_d, _ = _dev_matrix(_logits(7, n, V), torch.float32, dev)
    bits = torch.from_numpy(_bits(_mask_table(V, V))).to(dev)
    ids = torch.from_numpy((np.arange(n) % 6).astype(np.int32)).to(dev)
    eager = engine.topk_rows(x_d, k, mask_kind=1, mask=bits, row_mask_id=ids, want=NAMES)
    torch.cuda.synchronize(dev)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        got = engine.topk_rows(x_d, k, mask_kind=1, mask=bits, row_mask_id=ids, want=NAMES)
    gr.replay()
    torch.cuda.synchronize(dev)
    for name in ("token",) + NAMES:
        assert torch.equal(got[name].view(torch.int32), eager[name].view(torch.int32)), name


def test_canaries_and_null_outputs(engine):
    import ctypes as C

    from genlm_backend_amd import _lib

    dev = engine.device
    n, V, k = 5, 4097, 5
    x32 = _logits(3, n, V)
    x_d, xv = _dev_matrix(x32, torch.float32, dev)
    size = dict(out_token=n * k, out_logp=n * k, out_logp_masked=n * k, out_lse=n, out_logZ=n)
    bufs = {name: torch.full((64 + m + 64,), CANARY, dtype=torch.float32, device=dev) for name, m in size.items()}

    def call(given):
        a = _lib.TopkArgs()
        a.struct_size = C.sizeof(_lib.TopkArgs)
        a.logits, a.dtype, a.ld = x_d.data_ptr(), _lib.F32, x_d.stride(0)
        a.n_rows, a.vocab, a.logit_scale, a.k = n, V, 1.0, k
        for name in given:
            setattr(a, name, bufs[name].data_ptr() + 64 * 4)
        assert engine.lib.glb_topk_rows(C.byref(a), engine._stream()) == _lib.GLB_OK
        torch.cuda.synchronize(dev)

    call(("out_token", "out_lse"))  # the others null: not written
    for name, t in bufs.items():
        assert bool((t[:64] == CANARY).all()) and bool((t[-64:] == CANARY).all()), name
        assert bool((t[64:-64] == CANARY).all()) == (name not in ("out_token", "out_lse")), name
    call(tuple(bufs))
    for name, t in bufs.items():
        assert bool((t[:64] == CANARY).all()) and bool((t[-64:] == CANARY).all()) and not bool((t[64:-64] == CANARY).any()), name
    got = {name[4:]: bufs[name][64:-64].view(n, k) if size[name] == n * k else bufs[name][64:-64] for name in bufs}
    got["token"] = got["token"].view(torch.int32)
    _compare(got, TR.topk_rows(xv, 64), k, "raw call")
    from genlm_backend_amd.engine import PreparedMasks

    with pytest.raises(TypeError, match="prepared"):
        engine.topk_rows(x_d, k, mask=PreparedMasks(None, 6, V, _lib.F32))
    with pytest.raises(ValueError, match="k must"):
        engine.topk_rows(x_d, 65)
    with pytest.raises(ValueError, match="want names"):
        engine.topk_rows(x_d, k, want=("entropy",))
    with pytest.raises(ValueError, match="positive and finite"):
        engine.topk_rows(x_d, k, logit_scale=0.0)


# ---- glb_beam_select -----------------------------------------------------------------------------------------------------------
def _beam_case(seed, G, B, k):
    """Scores, alive flags and candidate arrays as a search meets them.  Group g is of kind g % 6: 0 - one live beam only (the
    first step); 1 - every beam finished; 2 - fewer than B candidates (one live beam with two tokens, the rest empty);
    3 - values tied across beams (scores and log-probabilities in quarters); 4 - random with -1 tokens and -inf values in the
    candidate arrays; 5 - random, with finished and empty beams."""
    rs = np.random.default_rng(seed)
    n = G * B
    score = -rs.random(n).astype(np.float32) * 4
    alive = np.ones(n, np.int32)
    tok = rs.integers(0, 1000, (n, k)).astype(np.int32)
    lp = -np.sort(rs.random((n, k)).astype(np.float32) * 6, axis=1)
    for g in range(G):
        s = slice(g * B, (g + 1) * B)
        kind = g % 6
        if kind == 0:
            score[s] = -np.inf
            score[g * B] = 0.0
        elif kind == 1:
            alive[s] = 0
            score[g * B + B // 2] = score[g * B]  # (a tie between finished beams)
        elif kind == 2:
            score[s] = -np.inf
            score[g * B + B - 1] = -1.5
            tok[g * B + B - 1, 2:] = -1
            lp[g * B + B - 1, 2:] = -np.inf
        elif kind == 3:
            score[s] = -rs.integers(0, 3, B).astype(np.float32) / 4
            lp[s] = -np.sort(rs.integers(0, 4, (B, k)).astype(np.float32) / 4, axis=1)
            alive[g * B + B // 2] = 0 if B > 1 else 1
        elif kind == 4:
            cut = rs.integers(0, k + 1, B)
            for b in range(B):
                tok[g * B + b, cut[b]:] = -1
                lp[g * B + b, cut[b]:] = -np.inf
            lp[g * B, 0] = -np.inf  # (a -inf value with a token)
        else:
            alive[s] = rs.random(B) < 0.6
            score[s][rs.random(B) < 0.2] = -np.inf
    return score, alive, tok, lp


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("B", [1, 4, 64])
@pytest.mark.parametrize("G", [1, 3, 65])
def test_beam_select(engine, G, B, k):
    dev = engine.device
    for seed in ((0, 1, 2, 3, 4, 5) if G == 1 else (0,)):  # (one group: every kind in turn)
        score, alive, tok, lp = _beam_case(G * 1000 + B * 10 + k + seed, max(G, seed + 1), B, k)
        if G == 1:
            g = seed
            score, alive, tok, lp = score[g * B:(g + 1) * B], alive[g * B:(g + 1) * B], tok[g * B:(g + 1) * B], lp[g * B:(g + 1) * B]
        want = TR.beam_select(score, alive, tok, lp, B)
        got = engine.beam_select(*(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (score, alive, tok, lp)), B)
        for name, g_, w_ in zip(("parent", "token", "score"), got, want):
            g_ = g_.cpu().numpy()
            assert g_.dtype == w_.dtype and not np.isnan(g_.astype(np.float64)).any()
            assert np.array_equal(g_, w_), (G, B, k, seed, name, np.flatnonzero(g_ != w_)[:5], g_[:8], w_[:8])
        assert ((want[0] < 0) == np.isneginf(want[2])).all()
