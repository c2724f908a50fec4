"""glb_gemm_f32_split where its answer is known exactly, at the smallest shapes the library serves (tests/split_gemm_ref.py:
edge_grid): the packed image byte for byte; selections through A and through W, dense integers and power-of-two scalings
compared with torch.equal, each only after exact_sum_ok has shown that no order of additions can round; bit comparisons
of rows, columns, padded and hostile calls with their plain counterparts; the GELU epilogue element by element; and the
guards of HipEngine.gemm_split.  No tolerance appears outside the GELU test."""
import ctypes as C

import pytest
import torch

from tests import split_gemm_ref as R

pytestmark = pytest.mark.gpu

GRID = R.edge_grid()
FLT_MAX = 3.4028234663852886e38


def _ids(v):
    return "m%d-n%d-k%d" % v


def _bits_equal(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def _run(engine, a, w, bias=None, gelu=False):
    img = engine.gemm_split_weights(w.cuda())
    assert img is not None
    y = engine.gemm_split(a.cuda(), img, w.shape[1], None if bias is None else bias.cuda(), gelu=gelu)
    assert y is not None
    return y.cpu()


def _gauss(m, n, k, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(m, k, generator=g), torch.randn(k, n, generator=g), torch.randn(n, generator=g)


# ---- 2a: the device image is the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n", [(64, 128), (192, 384), (768, 256)])
def test_device_image_equals_the_restatement(engine, k, n):
    g = torch.Generator().manual_seed(k + n)
    w = R.full_mantissa((k, n), g, -40, 40)  # full 24-bit mantissas, mixed sign and exponent
    want = R.split_image(w)
    got = engine.gemm_split_weights(w.cuda())
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), want)
    # a column slice of a wider matrix: ldw > n, storage offset 3 floats (12 bytes: no multiple of 16)
    wide = torch.full((k, n + 5), float("nan"))
    wide[:, 3:3 + n] = w
    view = wide.cuda()[:, 3:3 + n]
    assert view.stride(0) == n + 5 and view.data_ptr() % 16 == 12
    assert torch.equal(engine.gemm_split_weights(view).cpu(), want)


# ---- 2b - 2e: exact answers over the edge grid ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", GRID, ids=_ids)
def test_selection_through_a(engine, shape):
    """One-hot rows of A pick rows of a full-mantissa W: every byte of the image, the three B planes, A's staging at every
    K offset."""
    m, n, k = shape
    for phase in range(R.spread_phases(m, k)):
        for with_bias in (False, True):
            a, w, b, want = R.onehot_case(m, n, k, phase, with_bias)
            assert R.exact_sum_ok(a, w, b) and R.dropped_products_zero(a, w)
            assert _bits_equal(_run(engine, a, w, b), want), (phase, with_bias)


@pytest.mark.parametrize("shape", GRID, ids=_ids)
def test_selection_through_w(engine, shape):
    """A 0 / +-1 W picks columns of a full-mantissa A: the in-register split, the three A planes, the C/D lane map of every
    fragment of every wave."""
    m, n, k = shape
    for phase in range(R.spread_phases(n, k)):
        a, w, want = R.selection_case(m, n, k, phase)
        assert R.exact_sum_ok(a, w) and R.dropped_products_zero(a, w)
        assert _bits_equal(_run(engine, a, w), want), phase


@pytest.mark.parametrize("shape", GRID, ids=_ids)
def test_dense_integers(engine, shape):
    """Every K block adds its own integers: a stale, repeated or skipped LDS stage changes the sum; with both operands wide,
    mid.mid is nonzero and a plane that reaches the wrong product changes it too."""
    m, n, k = shape
    for wide in ("a", "w", "both"):
        a, w, b, want = R.dense_int_case(m, n, k, wide)
        assert R.exact_sum_ok(a, w, b) and R.dropped_products_zero(a, w)
        assert torch.equal(_run(engine, a, w, b), want), wide


@pytest.mark.parametrize("shape", GRID, ids=_ids)
def test_power_of_two_scaling_keeps_the_bits(engine, shape):
    """(A 2^s) . (W 2^-s) has the bits of A . W.  These operands round (exact_sum_ok does not hold and is not what makes this
    exact): what does is that every part of every scaled operand stays a normal bf16 number, so the split, the products and
    every addition are those of s = 0 - asserted on the inputs first."""
    m, n, k = shape
    a, w, b = R.scaling_case(m, n, k)
    assert bool((a.abs() >= 2.0 ** -4).all() and (a.abs() < 2.0 ** 4).all() and (w.abs() >= 2.0 ** -4).all())
    base = _run(engine, a, w, b)
    for s in (-60, -30, 30, 60):
        a_s, w_s = a * 2.0 ** s, w * 2.0 ** -s
        assert R.parts_stay_normal(a_s) and R.parts_stay_normal(w_s)
        assert torch.equal((a_s * 2.0 ** -s), a) and torch.equal(w_s * 2.0 ** s, w)
        assert _bits_equal(_run(engine, a_s, w_s, b), base), s


# ---- 3: containment and invariance -------------------------------------------------------------------------------------------
SMALL = [s for s in GRID if s[2] in (64, 768) or R.tiles(s[0], s[1]) in (7, 8, 9)]


@pytest.mark.parametrize("shape", SMALL, ids=_ids)
def test_row_and_column_bits_do_not_depend_on_the_batch(engine, shape):
    m, n, k = shape
    a, w, b = _gauss(m, n, k, seed=m + n + k)
    ad, wd, bd = a.cuda(), w.cuda(), b.cuda()
    img = engine.gemm_split_weights(wd)
    full = engine.gemm_split(ad, img, n, bd)
    for i in sorted({0, m // 2, m - 1}):  # a row computed alone
        assert _bits_equal(engine.gemm_split(ad[i:i + 1], img, n, bd), full[i:i + 1]), i
    for r0 in sorted({min(5, m - 1), min(131, m - 1)}):  # the same rows at another row offset, in another wave and tile
        assert _bits_equal(engine.gemm_split(ad[r0:], img, n, bd), full[r0:]), r0
    img128 = engine.gemm_split_weights(wd[:, :128])  # (a view when n > 128: ldw > n)
    assert _bits_equal(engine.gemm_split(ad, img128, 128, bd[:128].contiguous()), full[:, :128])
    if n > 128:
        img_hi = engine.gemm_split_weights(wd[:, n - 128:].contiguous())
        assert _bits_equal(engine.gemm_split(ad, img_hi, 128, bd[n - 128:].contiguous()), full[:, n - 128:])


@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("shape", [(1, 128, 64), (17, 128, 64), (129, 256, 128), (300, 384, 768), (895, 128, 64)], ids=_ids)
def test_nothing_outside_m_by_n_is_written_and_nothing_outside_m_by_k_is_read(engine, shape, gelu):
    """The C ABI with ldc > n and lda > k: sentinels in C's pitch gap and in 130 rows behind row m-1, NaN in A's padding
    columns and in 130 rows behind row m-1, every buffer one allocation."""
    from genlm_backend_amd import _lib

    m, n, k = shape
    a, w, b = _gauss(m, n, k, seed=3 * m + n + k)
    plain = _run(engine, a, w, b, gelu)
    lda, ldc, extra, mark = k + 12, n + 7, 130, -12345.0
    abuf = torch.full((m + extra, lda), float("nan"))
    abuf[:m, :k] = a
    abuf, bd = abuf.cuda(), b.cuda()
    cbuf = torch.full((m + extra, ldc), mark, device="cuda")
    img = engine.gemm_split_weights(w.cuda())
    g = _lib.GemmArgs()
    g.struct_size = C.sizeof(_lib.GemmArgs)
    g.m, g.n, g.k = m, n, k
    g.a, g.lda, g.w_split, g.bias = abuf.data_ptr(), lda, img.data_ptr(), bd.data_ptr()
    g.c, g.ldc = cbuf.data_ptr(), ldc
    g.epilogue = _lib.GEMM_BIAS_GELU_TANH if gelu else _lib.GEMM_BIAS
    assert engine.lib.glb_gemm_f32_split(C.byref(g), engine._stream()) == _lib.GLB_OK
    torch.cuda.synchronize()
    got = cbuf.cpu()
    assert _bits_equal(got[:m, :n], plain)
    assert bool((got[:m, n:] == mark).all()) and bool((got[m:] == mark).all())


BELOW = float.fromhex("0x1.fefffep127")  # the largest float32 that still rounds to a finite bf16
HOSTILE = [float("nan"), float("inf"), float("-inf"), FLT_MAX, -FLT_MAX, R.BF16_OVER, -R.BF16_OVER]


@pytest.mark.parametrize("shape", [(17, 128, 64), (300, 256, 192), (129, 384, 768)], ids=_ids)
def test_hostile_elements_stay_in_their_row_or_column(engine, shape):
    """The contract of include/glb.h: NaN, +-inf and finite |x| >= 0x1.ffp127 (they round to a bf16 infinity; +-FLT_MAX is
    among them) in A make that row of C non-finite, in W that column; every other row or column keeps the bits of the clean
    call.  The largest |x| below the threshold, and 3.39e38, are served as numbers."""
    m, n, k = shape
    a, w, b = _gauss(m, n, k, seed=m + 7 * n + k)
    w = w * 0.02
    clean = _run(engine, a, w, b)
    assert bool(torch.isfinite(clean).all())
    # rows of A: one hostile value each, the last row (the one that tail rows re-read) among them
    rows = [m - 1 - 2 * i for i in range(len(HOSTILE))]
    cols = [(k - 1 - 37 * i) % k for i in range(len(HOSTILE))]
    bad = a.clone()
    for r, c, v in zip(rows, cols, HOSTILE):
        bad[r, c] = v
    got = _run(engine, bad, w, b)
    keep = torch.ones(m, dtype=torch.bool)
    keep[rows] = False
    assert _bits_equal(got[keep], clean[keep])
    assert not bool(torch.isfinite(got[~keep]).any())  # the contract: the whole row
    ref = (bad.double() @ w.double() + b.double()).float()  # (non-finite also where float32 cannot hold the float64 sum)
    assert not bool(torch.isfinite(got[~torch.isfinite(ref)]).any())
    # columns of W
    wrows = [(k - 1 - 29 * i) % k for i in range(len(HOSTILE))]
    wcols = [(n - 1 - 17 * i) % n for i in range(len(HOSTILE))]
    badw = w.clone()
    for r, c, v in zip(wrows, wcols, HOSTILE):
        badw[r, c] = v
    got = _run(engine, a, badw, b)
    keep = torch.ones(n, dtype=torch.bool)
    keep[wcols] = False
    assert _bits_equal(got[:, keep], clean[:, keep])
    assert not bool(torch.isfinite(got[:, ~keep]).any())
    ref = (a.double() @ badw.double() + b.double()).float()
    assert not bool(torch.isfinite(got[~torch.isfinite(ref)]).any())
    # just below the threshold: numbers like any other (|w| < 0.1 here: the products stay in range)
    one_row = torch.ones(m, dtype=torch.bool)
    one_row[rows[0]] = False
    for v in (3.39e38, -3.39e38, BELOW, -BELOW):
        near = a.clone()
        near[rows[0], cols[0]] = v
        got = _run(engine, near, w, b)
        assert bool(torch.isfinite(got).all()) and _bits_equal(got[one_row], clean[one_row]), v


# ---- 4: the GELU epilogue, element by element -----------------------------------------------------------------------------------
# |gelu_kernel(x) - gelu_float64(x)| <= GELU_C * 2^-24 * |x| for every pre-activation x of R.gelu_case().  The bound is in |x|,
# not in the result: 1 + tanh cancels near x = -5 and a bound relative to the result would mean nothing there.  GELU_C is
# twice the largest such ratio of torch.nn.functional.gelu(approximate="tanh") in float32 on the same grid on an MI355X
# against the same float64 reference (it depends on the device's tanhf and cannot be derived).
# Measured (profiles/r12/split_gemm_exact_tests.log): torch 1.6144, so GELU_C = 3.2288; this kernel 1.6144 as well.
GELU_TORCH_RATIO = 1.6144
GELU_C = 2 * GELU_TORCH_RATIO


def test_gelu_epilogue_element_by_element(engine):
    a, w, b, pre = R.gelu_case()
    assert R.exact_sum_ok(a, w, b)
    want = R.gelu_tanh64(pre)
    got = _run(engine, a, w, b, gelu=True)
    assert _bits_equal(_run(engine, a, w, b), pre)  # the pre-activation is what the host says it is
    lib = torch.nn.functional.gelu(pre.cuda(), approximate="tanh").cpu()
    unit = pre.double().abs() * 2.0 ** -24

    def ratio(y):
        err = (y.double() - want).abs()
        assert bool((err[unit == 0] == 0).all())  # +-0 -> exactly 0
        r = err[unit > 0] / unit[unit > 0]
        return r.max().item()

    k_ratio, t_ratio = ratio(got), ratio(lib)
    print(f"\ngelu epilogue: largest |err| / (2^-24 |x|): kernel {k_ratio:.4f}, torch fp32 {t_ratio:.4f}, C {GELU_C}")
    assert k_ratio <= GELU_C, (k_ratio, t_ratio)
    # separately: large negative finite inputs give +-0, large positive ones x itself; never NaN
    assert not bool(torch.isnan(got).any())
    big = pre.abs() >= 1e4
    assert int(big.sum()) == 6 * R.GELU_M
    assert _bits_equal(got[big & (pre > 0)], pre[big & (pre > 0)])
    assert bool((got[big & (pre < 0)] == 0).all())
    # (a -0 in W or in the bias reaches the epilogue as +0: the accumulator starts at +0)
    assert int((pre == 0).sum()) == 2 * R.GELU_M and _bits_equal(got[pre == 0], torch.zeros(2 * R.GELU_M))


# ---- 5: HipEngine.gemm_split's out= and bias ----------------------------------------------------------------------------------
def test_strided_out_is_written_in_place_and_only_there(engine):
    m, n, k = 129, 256, 128
    a, w, b = _gauss(m, n, k, seed=9)
    ad, bd = a.cuda(), b.cuda()
    img = engine.gemm_split_weights(w.cuda())
    plain = engine.gemm_split(ad, img, n, bd)
    buf = torch.full((m + 2, n + 24), -7.0, device="cuda")
    view = buf[1:m + 1, 8:8 + n]
    ret = engine.gemm_split(ad, img, n, bd, out=view)
    assert ret.data_ptr() == view.data_ptr() and _bits_equal(view, plain)
    assert bool((buf[0] == -7).all() and (buf[m + 1] == -7).all() and (buf[:, :8] == -7).all() and (buf[:, 8 + n:] == -7).all())
    one = torch.full((3, n), -7.0, device="cuda")  # a single row, whatever its stride says
    engine.gemm_split(ad[:1], img, n, bd, out=one[1:2])
    assert _bits_equal(one[1:2], plain[:1]) and bool((one[0] == -7).all() and (one[2] == -7).all())


def test_out_and_bias_are_checked(engine):
    m, n, k = 16, 128, 64
    a, w, b = _gauss(m, n, k, seed=10)
    ad, bd = a.cuda(), b.cuda()
    img = engine.gemm_split_weights(w.cuda())
    for bad_out in (torch.empty(m, n, device="cuda", dtype=torch.float16), torch.empty(m, n),
                    torch.empty(m + 1, n, device="cuda"), torch.empty(m, n + 128, device="cuda"), torch.empty(m * n, device="cuda"),
                    torch.empty(m, 2 * n, device="cuda")[:, ::2], torch.empty(n, m, device="cuda").t()):
        with pytest.raises(ValueError):
            engine.gemm_split(ad, img, n, bd, out=bad_out)
    for bad_bias in (torch.zeros(n - 1, device="cuda"), torch.zeros(n + 1, device="cuda"), torch.zeros(1, n, device="cuda"),
                     torch.zeros(n)):
        with pytest.raises(ValueError):
            engine.gemm_split(ad, img, n, bad_bias)
    # not served: the caller's addmm takes these
    assert engine.gemm_split(ad, img, n, bd.half()) is None and engine.gemm_split(ad, img, n, bd.double()) is None
    assert engine.gemm_split(ad, img, n, torch.zeros(2 * n, device="cuda")[::2]) is None


def test_module_with_a_bias_the_kernel_does_not_take_is_conv1d(engine):
    from transformers.pytorch_utils import Conv1D

    from genlm_backend_amd.fuse import SplitConv1D

    src = Conv1D(128, 64).cuda()
    x = torch.randn(40, 64, device="cuda")
    strided = torch.randn(2 * 128, device="cuda")[::2]
    with torch.no_grad():
        src.bias = torch.nn.Parameter(strided, requires_grad=False)
        assert src.bias.stride(0) == 2
        mod = SplitConv1D(src, engine, min_rows=16)
        assert torch.equal(mod(x), src(x))  # the library's addmm, bit for bit
        src.bias = torch.nn.Parameter(strided.contiguous(), requires_grad=False)
        y = mod(x)  # the kernel again
        assert torch.allclose(y, src(x), rtol=1e-5, atol=1e-5)
        src.bias = torch.nn.Parameter(strided.contiguous().double(), requires_grad=False)
        try:
            want = src(x)
        except RuntimeError:
            want = None
        if want is None:
            with pytest.raises(RuntimeError):
                mod(x)  # as Conv1D itself: torch's error
        else:
            assert torch.equal(mod(x), want)
