"""glb_truncate_rows (HipEngine.truncate_rows) and the truncated samplers on the GPU against tests/truncate_ref.py.

What is exact and what is held to a bound (include/glb.h):
  * a key is one rounded multiply and one rounded add, restated in float32 by the reference; tau_k is a count and tau_m one
    rounded add - so with top_p off the threshold equals the reference's bit for bit, and always the bits are {key >= tau} for
    the device's own tau, `kept` their popcount, pad bits 0, nothing written beyond ceil(V / 32) words;
  * the nucleus boundary is the exact answer for some p' within 1e-4 of top_p (the library's log-sum-exp contract): tau must be
    max(tau_k, tau_m, t) for a key t between the reference's answers at top_p + 1e-4 and top_p - 1e-4; where the row is built so
    that top_p lies at least 5e-4 from every cumulative mass, t is the reference's own;
  * logmass is within 1e-4 of float64 for the set the device kept."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import truncate_ref as TQ

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = 0x5A5A5A5A
CANARY = 12345.0
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
OFF = dict(top_k=0, top_p=1.0, min_p=0.0)


def _gauss(seed, n, V):
    """Flat rows: N(0, 1) in the even rows and 3 N(0, 1) in the odd ones, a tenth -inf in every third row."""
    rs = np.random.default_rng(seed)
    x = rs.standard_normal((n, V)).astype(np.float32)
    x[1::2] *= 3
    for r in range(0, n, 3):
        if V > 4:
            x[r, rs.random(V) < 0.1] = -np.inf
    return x


def _dev_matrix(x32, dtype, dev, pad=5):
    """x as a device matrix of `dtype` with pitch V + pad, NaN behind every row, its base one element past the allocation's (no
    16-byte alignment anywhere); and the values it holds, float32 (exact)."""
    n, V = x32.shape
    flat = torch.full((n * (V + pad) + 1,), NAN, dtype=dtype, device=dev)
    t = flat[1:].view(n, V + pad)
    t[:, :V] = torch.from_numpy(x32).to(dev).to(dtype)
    return t[:, :V], t[:, :V].float().cpu().numpy()


def _run(engine, x_d, *, top_k=0, top_p=1.0, min_p=0.0, scale=1.0, kind=0, mask=None, ids=None, pad_words=2):
    """The call through the C ABI into sentinel-filled buffers: bit rows of pitch words + pad_words with a guard row on either
    side, a guard element around the three [n] outputs.  Returns (bits uint32 [n, words], tau, kept, logmass) after checking
    that every sentinel survived."""
    from genlm_backend_amd import _lib
    from genlm_backend_amd.engine import _DT

    dev = engine.device
    n, V = x_d.shape
    words = (V + 31) // 32
    ld = words + pad_words
    buf = torch.full((n + 2, ld), SENT, dtype=torch.int32, device=dev)
    thr = torch.full((n + 2,), CANARY, dtype=torch.float32, device=dev)
    lm = torch.full((n + 2,), CANARY, dtype=torch.float32, device=dev)
    kept = torch.full((n + 2,), SENT, dtype=torch.int32, device=dev)
    a = _lib.TruncateArgs()
    a.struct_size = C.sizeof(_lib.TruncateArgs)
    a.logits, a.dtype = x_d.data_ptr(), _DT[x_d.dtype]
    a.n_rows, a.vocab, a.ld, a.logit_scale = n, V, (x_d.stride(0) if n > 1 else V), scale
    a.top_k, a.top_p, a.log_min_p = top_k, top_p, float(TQ.log_min_p(min_p))
    a.mask_kind = kind
    if kind:
        a.mask, a.n_masks, a.mask_ld = mask.data_ptr(), mask.shape[0], (mask.stride(0) if mask.shape[0] > 1 else mask.shape[1])
        a.row_mask_id = None if ids is None else ids.data_ptr()
    a.out_bits, a.out_ld = buf[1].data_ptr(), ld
    a.out_threshold, a.out_kept, a.out_logmass = thr[1:].data_ptr(), kept[1:].data_ptr(), lm[1:].data_ptr()
    rc = engine.lib.glb_truncate_rows(C.byref(a), engine._stream())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    b = buf.cpu().numpy().view(np.uint32)
    assert (b[0] == SENT).all() and (b[-1] == SENT).all(), "a guard row of the bit rows was written"
    assert (b[1:-1, words:] == SENT).all(), "words beyond ceil(V / 32) were written"
    for t, s in ((thr, CANARY), (lm, CANARY), (kept, SENT)):
        assert t[0].item() == s and t[-1].item() == s
    return b[1:-1, :words].copy(), thr[1:-1].cpu().numpy(), kept[1:-1].cpu().numpy(), lm[1:-1].cpu().numpy()


def _check_exact(got, refs, V, what):
    """What holds for every row whatever the options: the bits are {key > -inf, key >= tau} for the device's own tau, kept is
    their popcount, the pad bits are 0, no NaN; an empty row gives tau +inf, logmass -inf; logmass within 1e-4 of float64."""
    bits, thr, kept, lm = got
    allb = TQ.unpack_bits(bits)
    assert not allb[:, V:].any(), (what, "pad bits")
    assert not np.isnan(thr).any() and not np.isnan(lm).any(), what
    for r, ref in enumerate(refs):
        key = ref["key"]
        fin = key > -np.inf
        want = fin & (key >= thr[r])
        assert np.array_equal(allb[r, :V], want), (what, r, int(allb[r, :V].sum()), int(want.sum()), thr[r])
        assert kept[r] == want.sum(), (what, r)
        if not fin.any():
            assert thr[r] == np.inf and lm[r] == -np.inf and kept[r] == 0, (what, r)
            continue
        assert want[np.argmax(key)], (what, r, "the largest key is kept")
        w = np.exp(key[fin].astype(np.float64) - float(key[fin].max()))
        exact = np.log(w[want[fin]].sum() / w.sum())
        assert abs(lm[r] - exact) <= 1e-4, (what, r, lm[r], exact)


def _check_tau(got, refs, what, exact_p=False):
    """tau against the reference: equal when the nucleus is off (or exact_p: the row's boundary is unambiguous); else
    max(tau_k, tau_m, t) for a key t of the row inside the reference's interval."""
    thr = got[1]
    for r, ref in enumerate(refs):
        if not (ref["key"] > -np.inf).any():
            continue
        base = max(ref["tau_k"], ref["tau_m"])
        if ref["tau_p"] == -np.inf or exact_p:
            assert thr[r] == ref["tau"], (what, r, thr[r], ref["tau"], ref["margin"])
            if exact_p:
                assert np.array_equal(TQ.unpack_bits(got[0])[r, :len(ref["keep"])], ref["keep"]), (what, r)
            continue
        assert thr[r] >= base, (what, r, thr[r], base)
        if thr[r] > base:  # then it is the nucleus boundary: a key of the row inside the interval
            assert (ref["key"] == thr[r]).any(), (what, r, "tau is not a key of the row")
            assert ref["tau_p_lo"] <= thr[r] <= ref["tau_p_hi"], (what, r, thr[r], ref["tau_p_lo"], ref["tau_p_hi"])
        else:  # the boundary lies at or below the other two thresholds
            assert ref["tau_p_lo"] <= base, (what, r, base, ref["tau_p_lo"])
        assert thr[r] == ref["tau_m"] or (ref["key"] == thr[r]).any(), (what, r, "tau is neither a key nor tau_m")


def _options(V):
    ks = [dict(top_k=k) for k in (1, 2, 64, 65, 1000, V)]
    ms = [dict(min_p=0.05), dict(min_p=0.5)]
    ps = [dict(top_p=0.5), dict(top_p=0.9), dict(top_k=5, top_p=0.8, min_p=0.05), dict(top_k=1000, top_p=0.95, min_p=0.001)]
    return ks + ms + ps


@pytest.mark.parametrize("n", [1, 4, 9])
@pytest.mark.parametrize("V", [1, 31, 32, 33, 257, 4099, 8193])
def test_rows(engine, V, n):
    """Every dtype; top-k alone (tau == tau_k: k of 1, 2, 64, 65, 1000 and V), min-p alone (tau == tau_m), and the nucleus alone
    and with the others (valid) - at scale 1 and 1 / 0.7.  Every row is checked, none skipped."""
    x32 = _gauss(V * 17 + n, n, V)
    for dtype in DTYPES:
        x_d, xv = _dev_matrix(x32, dtype, engine.device)
        for i, opts in enumerate(_options(V)):
            scale = 1.0 if i % 2 else float(np.float32(1 / 0.7))
            what = f"V={V} n={n} {dtype} {opts} scale={scale:.3f}"
            refs = TQ.truncate_rows(xv, scale=scale, **opts)
            got = _run(engine, x_d, scale=scale, **opts)
            _check_exact(got, refs, V, what)
            _check_tau(got, refs, what)


@pytest.mark.parametrize("V,dtype", [(50257, torch.float32), (128256, torch.bfloat16)])
def test_big_rows(engine, V, dtype):
    x_d, xv = _dev_matrix(_gauss(V, 4, V), dtype, engine.device)
    for opts in (dict(top_k=50), dict(top_k=1000), dict(top_p=0.9), dict(min_p=0.02), dict(top_k=40, top_p=0.9, min_p=0.01), OFF):
        refs = TQ.truncate_rows(xv, **opts)
        got = _run(engine, x_d, **opts)
        _check_exact(got, refs, V, f"V={V} {opts}")
        _check_tau(got, refs, f"V={V} {opts}")
        if opts is OFF:
            assert (got[1] == -np.inf).all() and (got[3][[1, 2]] == 0.0).all()


def _boundary_cases(key):
    """(top_p, boundary index) for one multiset: top_p at the midpoint between the cumulative masses on either side of the first
    token, of the second, and of the deepest token whose share is at least 1e-3 - so top_p lies at least 5e-4 from both."""
    ks = np.sort(key.astype(np.float64))[::-1]
    w = np.exp(ks - ks[0])
    share = w / w.sum()
    C = np.cumsum(w) / w.sum()
    deep = int(np.nonzero(share >= 1e-3)[0].max())
    out = []
    for i in sorted({0, 1, deep}):
        assert share[i] >= 1e-3
        p = float(np.float32(((C[i - 1] if i else 0.0) + C[i]) / 2))
        out.append((p, i))
    return out


@pytest.mark.parametrize("V,sigma,dtype", [(4099, 6.0, torch.float32), (257, 4.0, torch.float16), (8193, 6.0, torch.bfloat16),
                                           (50257, 6.0, torch.float32)])
def test_exact_nucleus(engine, V, sigma, dtype):
    """Rows whose boundary is unambiguous by construction: the rows of a call are distinct permutations of one multiset, top_p
    the midpoint between two consecutive cumulative masses around a token of share >= 1e-3.  tau and the bits must be the
    reference's, every row asserted.  (V = 4099, sigma = 6, top_p = 0.5: such a boundary in every row as well.)"""
    rs = np.random.default_rng(V)
    base = (sigma * rs.standard_normal(V)).astype(np.float32)
    base = torch.from_numpy(base).to(dtype).float().numpy()  # (the multiset as the dtype holds it)
    x32 = np.stack([base[rs.permutation(V)] for _ in range(5)])
    assert len({x.tobytes() for x in x32}) == 5
    x_d, xv = _dev_matrix(x32, dtype, engine.device)
    cases = _boundary_cases(base)
    assert cases[-1][1] >= 3
    for p, i in cases:
        refs = TQ.truncate_rows(xv, top_p=p)
        for ref in refs:
            assert ref["margin"] >= 4.9e-4 and ref["kept"] >= i + 1, (p, i, ref["margin"])
        got = _run(engine, x_d, top_p=p)
        _check_exact(got, refs, V, f"V={V} p={p} i={i}")
        _check_tau(got, refs, f"V={V} p={p} i={i}", exact_p=True)
    if V == 4099:
        x32 = (6 * np.random.default_rng(100).standard_normal((6, V))).astype(np.float32)
        x_d, xv = _dev_matrix(x32, dtype, engine.device)
        refs = TQ.truncate_rows(xv, top_p=0.5)
        assert min(ref["margin"] for ref in refs) >= 5e-4
        _check_tau(_run(engine, x_d, top_p=0.5), refs, "sigma 6, top_p 0.5", exact_p=True)


def _hostile(V):
    rs = np.random.default_rng(V)
    x = np.full((8, V), -1.0, np.float32)
    x[0] = 2.5                                    # all equal
    x[1] = rs.standard_normal(V) - 10             # a tie group straddling the fifth place: 3 at 5.0, 6 at 4.0
    pos = np.array([i for i in rs.permutation(V) if i not in (3, 7, 20, V - 1)][:9])
    x[1, pos[:3]], x[1, pos[3:]] = 5.0, 4.0
    x[2, 3 % V], x[2, 20] = -0.0, 0.0             # -0 against +0 at the top
    x[3] = -np.inf                                # nothing
    x[4] = -np.inf
    x[4, V - 1] = 1.5                             # one finite key
    x[5] = -np.inf                                # keys whose fixed-point mass is 0: they count for top_k all the same
    x[5, 7], x[5, pos] = 0.0, -200.0
    x[6] = -0.5 * np.arange(V)                    # a geometric row: shares 0.39, 0.24, 0.14, ...
    x[7] = -np.inf
    x[7, pos[:4]] = [-0.0, -300.0, -300.0, -3.0e5]
    return x


@pytest.mark.parametrize("V", [33, 4099])
def test_ties_and_hostile_rows(engine, V):
    x_d, xv = _dev_matrix(_hostile(V), torch.float32, engine.device)
    kept = {}
    for name, opts in (("k1", dict(top_k=1)), ("k5", dict(top_k=5)), ("p01", dict(top_p=0.01)), ("k5p99", dict(top_k=5, top_p=0.99)),
                       ("m", dict(min_p=0.5)), ("off", OFF)):
        refs = TQ.truncate_rows(xv, **opts)
        got = _run(engine, x_d, **opts)
        _check_exact(got, refs, V, f"hostile V={V} {opts}")
        # (every boundary of these rows is a tie or a gap of more than 1e-3 of the mass: one right answer)
        _check_tau(got, refs, f"hostile V={V} {opts}", exact_p=True)
        kept[name] = got[2]
    assert kept["k1"][0] == V and kept["p01"][0] == V        # all equal: every tie is kept
    assert kept["k5"][1] == 9                               # the tie group at the fifth place, whole
    assert kept["k1"][2] == 2                               # -0 and +0 tie
    assert kept["off"][3] == 0 and kept["k1"][4] == 1
    assert kept["k5"][5] == 10 and kept["k5p99"][5] == 1    # ten keys (the top and nine massless ties), then the nucleus
    assert kept["k5"][7] == 4 and kept["p01"][7] == 1


def test_masks(engine):
    """A bit mask that forbids the top token, a float mask with weights, an id out of range on either side, one mask for all."""
    V, n = 4099, 6
    dev = engine.device
    rs = np.random.default_rng(5)
    x_d, xv = _dev_matrix(_gauss(11, n, V), torch.float32, dev)
    ok = rs.random((3, V)) < 0.5
    ok[0, np.argmax(np.where(np.isfinite(xv[0]), xv[0], -1e9))] = False
    ok[1, np.argmax(xv[1])] = False
    ok[2] = False
    ok[2, 17] = True
    bits = np.concatenate([TQ.pack_bits(ok) | np.uint32(0), np.full((3, 2), 0xFFFFFFFF, np.uint32)], axis=1)
    bits[:, (V + 31) // 32 - 1] |= np.uint32(0xFFFFFFFF) << np.uint32(V % 32)  # (garbage in the pad bits: a reader ignores it)
    fl = np.where(ok, rs.standard_normal((3, V)), -np.inf).astype(np.float32)
    ids = np.array([0, 1, 2, 3, -1, 0], np.int32)
    ids_d = torch.from_numpy(ids).to(dev)
    for opts in (dict(top_k=3), dict(top_p=0.7), dict(top_k=100, top_p=0.9, min_p=0.01)):
        for kind, tab in ((1, bits.view(np.int32)), (2, fl)):
            tab_d = torch.from_numpy(tab).to(dev)
            refs = TQ.truncate_rows(xv, kind=kind, table=tab, row_mask_id=ids, **opts)
            got = _run(engine, x_d, kind=kind, mask=tab_d, ids=ids_d, **opts)
            _check_exact(got, refs, V, f"mask kind {kind} {opts}")
            _check_tau(got, refs, f"mask kind {kind} {opts}")
            assert got[2][3] == 0 and got[2][4] == 0 and got[2][2] == 1
            assert not TQ.unpack_bits(got[0])[0, np.argmax(np.where(np.isfinite(xv[0]), xv[0], -1e9))]
            one = tab_d[1:2]  # n_masks == 1: everybody's
            refs = TQ.truncate_rows(xv, kind=kind, table=tab[1:2], **opts)
            got = _run(engine, x_d, kind=kind, mask=one, **opts)
            _check_exact(got, refs, V, f"one mask, kind {kind} {opts}")
            _check_tau(got, refs, f"one mask, kind {kind} {opts}")


def test_engine_call_and_its_bits_feed_the_other_kernels(engine):
    """HipEngine.truncate_rows returns what the C call writes, and its rows are raw MASK_BITS rows: topk_rows under them gives
    the largest kept keys and a logZ equal to logmass."""
    V, n = 8193, 5
    x_d, xv = _dev_matrix(_gauss(3, n, V), torch.bfloat16, engine.device)
    opts = dict(top_k=50, top_p=0.9, min_p=0.01)
    raw = _run(engine, x_d, scale=0.5, **opts)
    got = engine.truncate_rows(x_d, logit_scale=0.5, want=("threshold", "kept", "logmass"), **opts)
    assert got["bits"].dtype == torch.int32 and got["bits"].shape == (n, (V + 31) // 32)
    assert np.array_equal(got["bits"].cpu().numpy().view(np.uint32), raw[0])
    for name, r in zip(("threshold", "kept", "logmass"), raw[1:]):
        assert np.array_equal(got[name].cpu().numpy(), r), name
    assert set(engine.truncate_rows(x_d, top_k=3)) == {"bits"}
    top = engine.topk_rows(x_d, 8, logit_scale=0.5, mask_kind=1, mask=got["bits"], want=("logZ",))
    keep = TQ.unpack_bits(raw[0])[:, :V]
    for r in range(n):
        key = TQ.truncate_row(xv[r], scale=0.5)["key"]
        want = np.argsort(-np.where(keep[r], key, -np.inf).astype(np.float64), kind="stable")[:min(8, keep[r].sum())]
        assert top["token"][r].cpu().numpy()[:len(want)].tolist() == want.tolist()
    assert np.abs(top["logZ"].cpu().numpy() - raw[3]).max() <= 2e-4
    with pytest.raises(ValueError, match="top_p"):
        engine.truncate_rows(x_d, top_p=0.0)
    with pytest.raises(ValueError, match="want names"):
        engine.truncate_rows(x_d, want=("lse",))


def test_determinism(engine):
    """A row's outputs are the same bytes alone, among others, with the call cut in two, and run twice."""
    V, n = 8193, 6
    x_d, _ = _dev_matrix(_gauss(9, n, V), torch.float32, engine.device)
    opts = dict(top_k=300, top_p=0.9, min_p=0.001)
    whole = _run(engine, x_d, **opts)
    again = _run(engine, x_d, **opts)
    parts = [_run(engine, x_d[:2], **opts), _run(engine, x_d[2:], **opts)]
    alone = [_run(engine, x_d[r:r + 1], **opts) for r in range(n)]
    for i in range(4):
        view = lambda a: np.ascontiguousarray(a).view(np.uint32)
        assert np.array_equal(view(whole[i]), view(again[i])), i
        assert np.array_equal(view(whole[i]), view(np.concatenate([p[i] for p in parts]))), i
        assert np.array_equal(view(whole[i]), view(np.concatenate([a[i] for a in alone]))), i
    assert (whole[2] > 1).all()


def test_bad_arguments_launch_nothing(engine):
    from genlm_backend_amd import _lib

    dev = engine.device
    x = torch.zeros((2, 64), device=dev)
    out = torch.full((2, 4), SENT, dtype=torch.int32, device=dev)
    mask = torch.zeros((3, 64), dtype=torch.int32, device=dev)

    def block():
        a = _lib.TruncateArgs()
        a.struct_size = C.sizeof(_lib.TruncateArgs)
        a.logits, a.dtype, a.ld = x.data_ptr(), _lib.F32, 64
        a.n_rows, a.vocab, a.logit_scale = 2, 50, 1.0
        a.top_k, a.top_p, a.log_min_p = 3, 0.9, -1.0
        a.out_bits, a.out_ld = out.data_ptr(), 4
        return a

    call = lambda a: engine.lib.glb_truncate_rows(C.byref(a), engine._stream())
    assert engine.lib.glb_truncate_rows(None, None) == _lib.GLB_EINVAL
    bad = [("struct_size", 1, "struct_size"), ("logits", 0, "logits is null"), ("out_bits", 0, "out_bits is null"),
           ("out_bits", out.data_ptr() + 2, "out_bits pointer misaligned"), ("out_ld", 1, "out_ld"), ("top_k", -1, "top_k"),
           ("top_p", 0.0, "top_p"), ("top_p", -0.5, "top_p"), ("top_p", 1.5, "top_p"), ("top_p", NAN, "top_p"),
           ("log_min_p", 0.5, "log_min_p"), ("log_min_p", NAN, "log_min_p"), ("vocab", (1 << 24) + 1, "2^24"),
           ("dtype", 3, "dtype"), ("dtype", -1, "dtype"), ("n_rows", 0, "positive"), ("vocab", 0, "positive"), ("n_rows", -1, "positive"),
           ("n_rows", 1 << 31, "31 bits"), ("ld", 49, "ld"), ("logits", x.data_ptr() + 2, "aligned"),
           ("logit_scale", NAN, "NaN"), ("logit_scale", 0.0, "positive and finite"), ("logit_scale", -1.0, "positive and finite"),
           ("logit_scale", float("inf"), "positive and finite"), ("mask_kind", _lib.MASK_PREPARED, "GLB_MASK_PREPARED"),
           ("mask_kind", 4, "mask_kind"), ("mask_kind", -1, "mask_kind")]
    for field, value, word in bad:
        a = block()
        setattr(a, field, value)
        if field == "vocab" and value > 64:
            a.ld, a.out_ld = value, value
        assert call(a) == _lib.GLB_EINVAL, field
        assert word in _lib.last_error(), (field, _lib.last_error())
    a = block()
    a.mask_kind = _lib.MASK_BITS
    assert call(a) == _lib.GLB_EINVAL and "mask table missing" in _lib.last_error()
    a.mask, a.n_masks, a.mask_ld = mask.data_ptr(), 3, 1
    assert call(a) == _lib.GLB_EINVAL and "mask_ld" in _lib.last_error()
    a.mask_ld = 2
    assert call(a) == _lib.GLB_EINVAL and "neither 1 nor" in _lib.last_error()
    a.mask, a.n_masks = mask.data_ptr() + 2, 2
    assert call(a) == _lib.GLB_EINVAL and "misaligned" in _lib.last_error()
    a.mask, a.mask_kind, a.mask_ld = mask.data_ptr(), _lib.MASK_F32, 49
    assert call(a) == _lib.GLB_EINVAL and "mask_ld" in _lib.last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == SENT).all()
    a = block()  # (the block itself is good: top_k above the vocabulary, top_p 1 and log_min_p -inf are "off")
    a.top_k, a.top_p, a.log_min_p = 1 << 40, 1.0, float("-inf")
    assert call(a) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32)[:, :2] == [0xFFFFFFFF, 0x3FFFF]).all()


# ---- the samplers ------------------------------------------------------------------------------------------------------------
SV, EOS = 1000, 0


@pytest.fixture(scope="module")
def llm(engine):
    from transformers import GPT2Config

    from genlm_backend_amd.llm import AsyncAmdLM

    cfg = GPT2Config(vocab_size=SV, n_positions=64, n_embd=64, n_layer=2, n_head=2, bos_token_id=EOS, eos_token_id=EOS,
                     initializer_range=0.35)  # (a wide init: the next-token distributions are not flat)
    return AsyncAmdLM.from_config(cfg, None, device=engine.device, dtype=torch.float32, seed=3, engine=engine, batch_size=64)


PROMPTS = [[5, 17, 230, 8], [901, 44]]
OPTS = dict(top_k=5, top_p=0.8, min_p=0.05)
T = 0.7


def _host_loop(m, prompts, max_tokens, seed, opts, temperature):
    """The reference's loop (one generator per sequence, seeded alike; softmax of logprobs / temperature) with the row filtered
    by tests/truncate_ref.py before the draw.  Returns (ids, keep sets per sequence and step, the smallest margin)."""
    ids, keeps, margin = [], [], np.inf
    for p in prompts:
        g = torch.Generator()
        g.manual_seed(seed)
        out, ks = [], []
        for _ in range(max_tokens):
            lp = m.next_token_logprobs_sync(p + out).float().cpu()
            ref = TQ.truncate_row((lp / temperature).numpy(), **opts)
            gap_k = np.sort(ref["key"])[::-1][opts["top_k"] - 1] - np.sort(ref["key"])[::-1][opts["top_k"]] if opts.get("top_k") else np.inf
            margin = min(margin, ref["margin"], gap_k, np.abs(ref["key"] - ref["tau_m"]).min())
            probs = torch.softmax(torch.where(torch.from_numpy(ref["keep"]), lp / temperature, torch.tensor(-np.inf)), dim=-1)
            tok = torch.multinomial(probs, num_samples=1, generator=g).item()
            ks.append(ref["keep"])
            if tok == EOS:
                break
            out.append(tok)
        ids.append(out)
        keeps.append(ks)
    return ids, keeps, margin


def test_seeded_sampler_matches_the_host_loop(llm):
    want, _, margin = _host_loop(llm, PROMPTS, 6, 11, OPTS, T)
    print("smallest boundary margin", margin)
    assert margin >= 1e-3, margin  # (no step's boundary is ambiguous: a disagreement below cannot hide behind one)
    got = llm.batch_sample_sync(PROMPTS, 6, [EOS], temperature=T, seed=11, **OPTS)
    assert got == want, (got, want)


def test_unseeded_sampler_draws_inside_the_keep_set(llm):
    got = llm.batch_sample_sync(PROMPTS, 6, [EOS], temperature=T, **OPTS)
    for p, row in zip(PROMPTS, got):
        for t, tok in enumerate(row):
            lp = llm.next_token_logprobs_sync(p + row[:t]).float().cpu()
            ref = TQ.truncate_row((lp / T).numpy(), **OPTS)
            assert ref["keep"][tok] or ref["margin"] < 1e-3, (t, tok)
            assert ref["kept"] <= 5


def test_top_k_one_is_greedy_and_defaults_change_nothing(llm):
    got = llm.batch_sample_sync(PROMPTS, 6, [], temperature=T, top_k=1)
    for p, row in zip(PROMPTS, got):
        assert len(row) == 6
        for t, tok in enumerate(row):
            assert tok == int(llm.next_token_logprobs_sync(p + row[:t]).argmax())
    plain = llm.batch_sample_sync(PROMPTS, 6, [EOS], temperature=T, seed=5)
    assert llm.batch_sample_sync(PROMPTS, 6, [EOS], temperature=T, seed=5, top_k=0, top_p=1.0, min_p=0.0) == plain
