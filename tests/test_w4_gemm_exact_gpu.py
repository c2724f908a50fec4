"""glb_w4_gemm where its answer is known exactly, at the smallest shapes it serves and at every kind of K split
(tests/w4_gemm_ref.py: edge_grid, M_GRID): selections through X and through W, dense integers with a per-block absmax -
each compared bit for bit, and only after exact_sum_ok has shown that no order of float32 additions can round; rows,
row permutations and repeated calls compared with each other; NaN, infinities, infinite and zero weight blocks and the
largest finite activations contained in their row or column; and W4Linear.forward over the same layers.  Every call goes
through a padded X (pitch k + 8, NaN in the padding) and a padded, guarded Y.  The one tolerance of the file is the
2x-of-F.linear rule of tests/test_quant4_gpu.py, for the inputs that W4Linear hands to the dequantise path.

Measured on an MI355X (this file alone, 153 tests): 10.4 s of wall time; the slowest parametrisation is the dense-integer
case at 128 x 65536 x 256, 0.93 s, so M_GRID was not thinned anywhere."""
import numpy as np
import pytest
import torch

from tests import quant4_engine as Q
from tests import w4_gemm_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
DTYPES = (torch.bfloat16, torch.float16)
NAN = float("nan")
EXACT = tuple(float(v) for v in R.EXACT_CB)


def _id(v):
    return {torch.bfloat16: "bf16", torch.float16: "f16"}.get(v, "-".join(map(str, v)) if isinstance(v, tuple) else str(v))


def _cases(shapes):
    return [pytest.param(nk, dt, id=f"{nk[0]}x{nk[1]}-{_id(dt)}") for nk in shapes for dt in DTYPES]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _guarded(rows, cols, pad, dtype, fill):
    ld = cols + pad
    buf = torch.full((GUARD + rows * ld + GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + rows * ld].view(rows, ld)[:, :cols], ld


def _gemm(engine, x, img, n, cb, bias=None):
    """One glb_w4_gemm call on host operands: X rows at a pitch of k + 8 with NaN between them, Y at a pitch of n + 8 inside
    guard elements that must come back untouched.  Returns Y on the host."""
    m, k = x.shape
    _, xd, _ = _guarded(m, k, 8, x.dtype, NAN)
    xd.copy_(x)
    ybuf, yd, ld = _guarded(m, n, 8, x.dtype, 7.0)
    got = engine.w4_gemm(xd, img, n, cb, None if bias is None else bias.to(DEV), out=yd)
    assert got is not None, (m, n, k)
    torch.cuda.synchronize()
    host = ybuf.cpu()
    body = host[GUARD:GUARD + m * ld].view(m, ld)
    assert bool((host[:GUARD] == 7.0).all() and (host[GUARD + m * ld:] == 7.0).all() and (body[:, n:] == 7.0).all()), (m, n, k)
    return body[:, :n].contiguous()


def _image(engine, w, cb):
    img = engine.w4_quantize(w.to(DEV), cb)
    assert img is not None
    return img


def _gauss_weights(n, k, seed, scale=1.0):
    """float32 Gaussian weights whose blocks have scales spread over e^-3 .. e^1."""
    g = torch.Generator().manual_seed(seed)
    s = torch.exp(torch.rand(n, k // 64, 1, generator=g) * 4.0 - 3.0)
    return (torch.randn(n, k // 64, 64, generator=g) * s * scale).view(n, k)


def _gauss_case(engine, n, k, dtype, seed, name="nf4", scale=1.0):
    """(x [128, k], bias, image, W' as the dtype on the host, codebook) of Gaussian operands: sums that round."""
    g = torch.Generator().manual_seed(seed + 1)
    cb = tuple(Q.codebook(name))
    w = _gauss_weights(n, k, seed, scale)
    x = torch.randn(R.M_MAX, k, generator=g).to(dtype)
    b = (torch.randn(n, generator=g) * 0.5).to(dtype)
    img = _image(engine, w, cb)
    wq = engine.w4_dequantize(img, n, k, cb, dtype=dtype).cpu()
    return x, b, img, wq, cb, w


# ---- the grid ---------------------------------------------------------------------------------------------------------------
def test_grid_holds_every_split_class(engine):
    found = R.ksplit_classes(engine)
    print("\nksplit classes of the edge grid (n, k, ksplit):")
    for c, v in found.items():
        print(f"  {c}: {v}")
    missing = [c for c, v in found.items() if not v]
    assert not missing, f"the edge grid no longer holds: {missing} (have the constants of glb_quant.hip changed?)"
    for n, k in R.edge_grid():  # the split does not depend on m
        assert len({R.ksplit_of(engine, m, n, k) for m in R.m_grid(n, k)}) == 1


# ---- a: selection through X -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nk,dtype", _cases(R.SMALL_NK))
def test_selection_through_x(engine, nk, dtype):
    """One-hot rows of X pick columns of W': every nibble of every unit, the lane-to-k assignment of both MFMAs of a block,
    every slice edge.  NF4 and FP4 images of Gaussian weights against glb_w4_dequantize's own 16-bit elements, and the
    EXACT_CB weights against values known on the host.  (A -0 of W' - FP4 has the code - reaches Y as +0: the accumulator
    starts at +0 and +0 + -0 is +0.)"""
    n, k = nk
    m = R.M_MAX
    phases = R.spread_phases(m, k)
    seen = set()
    for name in ("nf4", "fp4"):
        cb = tuple(Q.codebook(name))
        img = _image(engine, _gauss_weights(n, k, seed=n + k), cb)
        wq = engine.w4_dequantize(img, n, k, cb, dtype=dtype).cpu()
        assert bool(torch.isfinite(wq).all())
        for phase in range(phases):
            x, kidx, _ = R.onehot_x(m, k, phase, dtype, unit=True)
            seen.update(kidx.tolist())
            assert R.exact_sum_ok(x, wq)
            want = wq[:, kidx].T
            want = torch.where(want == 0, torch.zeros_like(want), want)
            assert _same_bits(_gemm(engine, x, img, n, cb), want), (name, phase)
            if phase == 0:  # an all-zero bias changes nothing
                assert _same_bits(_gemm(engine, x, img, n, cb, torch.zeros(n, dtype=dtype)), want), name
    assert seen == set(range(k))
    img = None
    for phase in range(phases):
        x, w, _, want = R.onehot_x_case(m, n, k, phase, dtype)
        assert R.exact_sum_ok(x, w)
        img = _image(engine, w, EXACT) if img is None else img
        assert _same_bits(_gemm(engine, x, img, n, EXACT), want), ("exact", phase)


# ---- b: selection through W -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nk,dtype", _cases(R.edge_grid()))
def test_selection_through_w(engine, nk, dtype):
    """A single -s per column of Y picks a column of a full-mantissa X: X's staging at every k, the clamp of the rows past m,
    the C/D lane map of every fragment.  Phase 0 runs every m of the grid; the other phases, which move the nonzero over
    the rest of K, run two each."""
    n, k = nk
    ms = R.m_grid(n, k)
    for phase in range(R.spread_phases(n, k)):
        x128, w, _, want128 = R.onehot_w_case(R.M_MAX, n, k, phase, dtype)  # (asserts X's full mantissas)
        assert R.exact_sum_ok(x128, w)
        img = _image(engine, w, EXACT)
        for m in ms if phase == 0 else (ms[(5 * phase) % len(ms)], R.M_MAX):
            x, wm, _, want = R.onehot_w_case(m, n, k, phase, dtype)
            assert torch.equal(x, x128[:m]) and torch.equal(wm, w) and torch.equal(want, want128[:m])
            assert _same_bits(_gemm(engine, x, img, n, EXACT), want), (phase, m)


# ---- c: dense integers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nk,dtype", _cases(R.edge_grid()))
def test_dense_integers(engine, nk, dtype):
    """Integer X, weights c * 2^e with e of its own per (row, block), integer bias: a block multiplied by a neighbour's
    absmax, a block skipped or added twice at a slice edge, a dropped row or lane changes the sum."""
    n, k = nk
    x128, w, b, want128 = R.dense_int_case(R.M_MAX, n, k, dtype)
    assert R.exact_sum_ok(x128, w, b) and R.exact_sum_ok(x128, w)
    img = _image(engine, w, EXACT)
    back = engine.w4_dequantize(img, n, k, EXACT, dtype=dtype).cpu()
    assert _same_bits(back, w.to(dtype)) and torch.equal(back.float(), w)  # W' is W: the device's round trip is exact too
    for m in R.m_grid(n, k):
        for with_bias in (True, False):
            x, _, bm, want = R.dense_int_case(m, n, k, dtype, with_bias)
            assert torch.equal(x, x128[:m]) and (bm is None or torch.equal(bm, b))
            got = _gemm(engine, x, img, n, EXACT, bm)
            assert torch.equal(got, want), (m, with_bias, int((got != want).sum()))


# ---- d: rows do not depend on the batch -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nk,dtype", _cases([(80, 448), (32, 704)]))
def test_row_bits_do_not_depend_on_the_batch(engine, nk, dtype):
    """Gaussian operands: these sums round, and what is compared is two runs of the same arithmetic.  Rows 0 .. m - 1 of an
    m-row call (every instantiation MF = 1 .. 8, first and last m of each) have the bits of the 128-row call; permuting X's
    rows permutes Y's; a second call gives the same bits."""
    n, k = nk
    x, b, img, _, cb, _ = _gauss_case(engine, n, k, dtype, seed=3 * n + k)
    full = _gemm(engine, x, img, n, cb, b)
    assert bool(torch.isfinite(full).all())
    assert _same_bits(_gemm(engine, x, img, n, cb, b), full)
    for m in R.M_GRID:
        assert _same_bits(_gemm(engine, x[:m], img, n, cb, b), full[:m]), m
    g = torch.Generator().manual_seed(n)
    for m in (R.M_MAX, 49, 17):
        perm = torch.randperm(R.M_MAX, generator=g)[:m]
        assert _same_bits(_gemm(engine, x[perm], img, n, cb, b), full[perm]), m
    assert _same_bits(_gemm(engine, x[77:78], img, n, cb, b), full[77:78])  # a row alone


# ---- e: containment -------------------------------------------------------------------------------------------------------------
def _column64(x, wrow, bias_j):
    """One column of Y in float64, term by term (no BLAS between the test and an infinity)."""
    return (x.double() * wrow.double()[None, :]).sum(1) + float(bias_j)


@pytest.mark.parametrize("m", [17, 49, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_nonfinite_x_stays_in_its_row(engine, dtype, m):
    n, k = 80, 448
    x, b, img, wq, cb, _ = _gauss_case(engine, n, k, dtype, seed=11)
    x = x[:m].clone()
    clean = _gemm(engine, x, img, n, cb, b)
    assert bool(torch.isfinite(clean).all())
    plants = [([(NAN, 3)], m - 1), ([(float("inf"), 200)], 0), ([(float("-inf"), k - 1)], m // 2),
              ([(NAN, 64), (float("inf"), 65), (float("-inf"), 300)], m - 1)]  # (row m - 1 is the one the rows past m re-read)
    for values, row in plants:
        bad = x.clone()
        for v, kk in values:
            bad[row, kk] = v
        got = _gemm(engine, bad, img, n, cb, b)
        keep = torch.ones(m, dtype=torch.bool)
        keep[row] = False
        assert _same_bits(got[keep], clean[keep]), (values, row)
        ref = torch.stack([_column64(bad[row:row + 1], wq[j], b[j])[0] for j in range(n)])
        assert not bool(torch.isfinite(ref).all())
        assert not bool(torch.isfinite(got[row][~torch.isfinite(ref)]).any()), (values, row)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_infinite_and_zero_weight_blocks_stay_in_their_column(engine, dtype):
    """One float32 block whose absmax is beyond the 16-bit dtype (1e5 for float16, 3.4e38 for bfloat16: W' is infinite
    there) and one all-zero block: every other column of Y keeps the bits of the call without them; the two columns are
    finite or not as the float64 product on the dequantised W' is."""
    n, k, m = 80, 448, 49
    x, b, img, wq, cb, w = _gauss_case(engine, n, k, dtype, seed=12)
    x = x[:m]
    clean = _gemm(engine, x, img, n, cb, b)
    j_inf, j_zero = 37, 16
    bad = w.clone()
    blk = bad[j_inf, 128:192]
    bad[j_inf, 128:192] = blk / blk.abs().max() * (1e5 if dtype == torch.float16 else 3.4e38)
    bad[j_zero, 384:448] = 0.0
    assert bool(torch.isfinite(bad).all())
    img_bad = _image(engine, bad, cb)
    wq_bad = engine.w4_dequantize(img_bad, n, k, cb, dtype=dtype).cpu()
    inf_at = ~torch.isfinite(wq_bad)
    assert bool(inf_at[j_inf, 128:192].any()) and int(inf_at.sum()) == int(inf_at[j_inf, 128:192].sum())
    assert bool((wq_bad[j_zero, 384:448] == 0).all())
    keep = torch.ones(n, dtype=torch.bool)
    keep[[j_inf, j_zero]] = False
    assert _same_bits(wq_bad[keep], wq[keep])
    got = _gemm(engine, x, img_bad, n, cb, b)
    assert _same_bits(got[:, keep], clean[:, keep])
    for j in (j_inf, j_zero):
        ref = _column64(x, wq_bad[j], b[j])
        assert torch.equal(torch.isfinite(got[:, j]), torch.isfinite(ref)), j
    assert not bool(torch.isfinite(got[:, j_inf]).any()) and bool(torch.isfinite(got[:, j_zero]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_largest_finite_rows_overflow_where_float64_does(engine, dtype):
    """Two rows of X hold the dtype's largest finite value (one +, one -).  Column j of W has t_j = 1 .. 3 entries -s_j,
    s_j = 1/2, 1, 2, in different K blocks (and different slices): the sum of a largest-value row is t_j s_j times the
    largest value, all terms of one sign, so the float32 partial sums grow monotonically and overflow if and only if the
    total does - the kernel's inf pattern must be that of the float64 answer rounded to the dtype, bit for bit.  The other
    rows keep the bits they have when the two rows hold ordinary values."""
    n, k, m = 80, 448, 33
    kb = k // 64
    w = torch.zeros(n, k)
    for j in range(n):
        for i in range(j % 3 + 1):
            w[j, 64 * ((j + 3 * i) % kb) + (5 * j + 17 * i) % 64] = -(2.0 ** ((j // 3) % 3 - 1))
    assert bool(((w != 0).view(n, kb, 64).sum(-1) <= 1).all())  # one -s per block: the round trip is exact
    img = _image(engine, w, EXACT)
    assert torch.equal(engine.w4_dequantize(img, n, k, EXACT, dtype=dtype).cpu().float(), w)
    x, _, _, _ = R.onehot_w_case(m, n, k, 0, dtype)  # (its X: full-mantissa rows)
    clean = _gemm(engine, x, img, n, EXACT)
    big = torch.finfo(dtype).max
    hot = x.clone()
    hot[5], hot[20] = big, -big
    got = _gemm(engine, hot, img, n, EXACT)
    keep = torch.ones(m, dtype=torch.bool)
    keep[[5, 20]] = False
    assert _same_bits(got[keep], clean[keep])
    want = (hot[[5, 20]].double() @ w.double().T).float().to(dtype)
    assert bool(torch.isinf(want).any()) and bool(torch.isfinite(want).any()) and not bool(torch.isnan(want).any())
    assert _same_bits(got[[5, 20]], want)


# ---- f: W4Linear.forward ----------------------------------------------------------------------------------------------------------
def _linear(engine, img, bias, n, k, quant_type, dtype):
    from genlm_backend_amd.quant import W4Linear, W4Scratch

    scratch = W4Scratch(engine.device)
    scratch.reserve(n * k, dtype)
    return W4Linear(img, None if bias is None else bias.to(DEV), k, n, quant_type, None, engine, scratch)


def _errors(y, ref):
    d = y.double().cpu() - ref
    return d.abs().max().item(), (d.norm() / ref.norm()).item()


@pytest.mark.parametrize("nk,dtype", _cases([(80, 448), (32, 704)]))
def test_w4linear_forward(engine, nk, dtype, monkeypatch):
    n, k = nk
    x, b, img, wq, cb, _ = _gauss_case(engine, n, k, dtype, seed=n + 5 * k)
    lin = _linear(engine, img, b, n, k, "nf4", dtype)
    lin.mode = "fused"
    # a 3-D input: the GEMM's bits
    x3 = x[:10].view(2, 5, k).to(DEV)
    y3 = lin(x3)
    assert y3.shape == (2, 5, n) and _same_bits(y3.cpu().view(10, n), _gemm(engine, x[:10], img, n, cb, b))
    # a sliced view that reshape has to copy: the bits of its contiguous copy
    view = x[:12].view(2, 6, k).to(DEV)[:, :5]
    assert not view.is_contiguous() and view.reshape(-1, k).data_ptr() != view.data_ptr()
    assert _same_bits(lin(view).cpu(), lin(view.contiguous()).cpu())
    # rows that are not 16-byte aligned, and 129 rows: not served by the kernel, W4Linear dequantises without a word - and
    # stays within twice F.linear's errors against float64 (the rule of tests/test_quant4_gpu.py)
    wide = torch.zeros(33, k + 8, dtype=dtype, device=DEV)
    wide[:, 4:4 + k] = x[:33].to(DEV)
    odd = wide[:, 4:4 + k]
    assert odd.data_ptr() % 16 == 8
    g = torch.Generator().manual_seed(k)
    many = torch.randn(R.M_MAX + 1, k, generator=g).to(dtype).to(DEV)
    wqd, bd = wq.to(DEV), b.to(DEV)
    for xin in (odd, many):
        assert engine.w4_gemm(xin, img, n, cb, bd) is None
        y = lin(xin)
        ref = xin.double().cpu() @ wq.double().T + b.double()
        lib = torch.nn.functional.linear(xin.contiguous(), wqd, bd)
        e_max, e_fro = _errors(y, ref)
        l_max, l_fro = _errors(lib, ref)
        print(f"W4Linear {n}x{k} {_id(dtype)} rows {xin.shape[0]}: max {e_max:.3e} (lib {l_max:.3e}) fro {e_fro:.3e} (lib {l_fro:.3e})")
        assert e_max <= 2 * l_max + 1e-30 and e_fro <= 2 * l_fro + 1e-30, (e_max, l_max, e_fro, l_fro)
    # dense integers: the dequantise path and the fused kernel agree exactly, and with the float64 answer
    from genlm_backend_amd import quant

    monkeypatch.setitem(quant.CODEBOOKS, "exact", EXACT)
    for m in (1, 17, R.M_MAX):
        xi, wi, bi, want = R.dense_int_case(m, n, k, dtype)
        assert R.exact_sum_ok(xi, wi, bi)
        li = _linear(engine, _image(engine, wi, EXACT), bi, n, k, "exact", dtype)
        out = {}
        for mode in ("fused", "dequant"):
            li.mode = mode
            out[mode] = li(xi.to(DEV)).cpu()
        assert torch.equal(out["fused"], want) and torch.equal(out["dequant"], want), m
