"""tests/w4_gemm_ref.py checked on the CPU: the EXACT_CB round trip through the restated quantiser, exact_sum_ok on every
case the builders make (and its rejection of a case made to round), and - for the dense-integer cases - float32 sums in
shuffled orders and slice by slice, all equal to the float64 answer: the expected values of
tests/test_w4_gemm_exact_gpu.py do not depend on the order in which the kernel adds."""
import numpy as np
import pytest
import torch

from tests import quant4_engine as Q
from tests import w4_gemm_ref as R

DTYPES = [torch.bfloat16, torch.float16]
ALL_DTYPES = [torch.float32] + DTYPES


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def test_exact_codebook_is_the_sixteen_eighths_unsorted():
    assert sorted(R.EXACT_CB.tolist()) == [j / 8 for j in range(-8, 8)]
    assert R.EXACT_CB.tolist() != sorted(R.EXACT_CB.tolist()) and R.EXACT_CB[R.CODE_NEG1] == -1.0
    srt, code_of, mid = Q.sorted_table(R.EXACT_CB)
    assert not np.array_equal(code_of, np.arange(16))  # the code is not the sorted index
    assert mid.tolist() == [(2 * i - 15) / 16 for i in range(15)]


@pytest.mark.parametrize("n,k", [(16, 64), (17, 192), (80, 704)])
def test_exact_codebook_round_trip_is_bit_exact(n, k):
    """Blocks of c * 2^e with one -2^e each: absmax is 2^e and dequantize(quantize(W)) is W, bit for bit, in float32,
    bfloat16 and float16, from either layout of the source (the transposed one is how a Conv1D weight is read)."""
    w, e = R.exact_weights(n, k)
    stub = Q.StubW4Engine()
    for e_shift in (0, -9, 11):  # (and with every block scaled by another power of two)
        ws = w * 2.0 ** e_shift
        codes, absmax = Q.quantize(ws.numpy(), R.EXACT_CB)
        assert np.array_equal(absmax, np.ldexp(np.float32(1), e + e_shift))
        assert np.array_equal(R.EXACT_CB[codes], (ws.numpy().reshape(n, -1, 64) / absmax[:, :, None]).reshape(n, k))
        for transposed in (False, True):  # the source as [n, k], and as the [k, n] memory of a Conv1D weight
            img = stub.w4_quantize(ws.T.contiguous() if transposed else ws, R.EXACT_CB, transposed=transposed)
            for dt in ALL_DTYPES:
                for tr in (False, True):
                    back = stub.w4_dequantize(img, n, k, R.EXACT_CB, dtype=dt, transposed=tr)
                    want = (ws.T.contiguous() if tr else ws).to(dt)
                    assert torch.equal(_bits(back), _bits(want)), (e_shift, transposed, dt, tr)
                    assert torch.equal(want.float(), ws.T if tr else ws)  # (the 16-bit value IS the float32 one)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_hot_weights_round_trip(dtype):
    """onehot_w_case's weight: the block of the nonzero holds -s and zeros (exact); every other block is zero and comes
    back as +-0."""
    for n, k in [(16, 64), (80, 704)]:
        for phase in (0, R.spread_phases(n, k) - 1):
            _, w, _, _ = R.onehot_w_case(17, n, k, phase, dtype)
            assert bool(((w != 0).sum(1) == 1).all()) and bool((w <= 0).all())
            back = Q.roundtrip(w, R.EXACT_CB, dtype)
            assert torch.equal(back.float(), w)  # (numerically: a zero block's W' is -0)


def _phases(count, k):
    p = R.spread_phases(count, k)
    return sorted({0, p // 2, p - 1})


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,k", R.edge_grid())
def test_every_built_case_is_exactly_summable(n, k, dtype):
    """exact_sum_ok over the whole grid.  The 128-row case of a shape holds every smaller one: a builder's m-row x is the
    first m rows of its 128-row x (asserted), and the condition is per output element."""
    m = R.M_MAX
    x, w, b, want = R.dense_int_case(m, n, k, dtype, with_bias=True)
    assert R.representable(x, dtype) and R.representable(b, dtype) and bool(x.abs().max() <= 4)
    assert R.exact_sum_ok(x, w, b) and R.exact_sum_ok(x, w, None)
    assert torch.isfinite(want).all()
    for mm in R.m_grid(n, k):
        xs, ws, bs, wants = R.dense_int_case(mm, n, k, dtype, with_bias=True)
        assert torch.equal(xs, x[:mm]) and torch.equal(wants, want[:mm]) and torch.equal(bs, b)
    if (n, k) in R.LARGE_NK:  # (the large-n selections: one phase each is what the GPU test runs)
        phases_x = phases_w = [0]
    else:
        phases_x, phases_w = _phases(m, k), _phases(n, k)
    for phase in phases_x:
        x, w, _, want = R.onehot_x_case(m, n, k, phase, dtype)
        assert R.exact_sum_ok(x, w) and bool(((x != 0).sum(1) == 1).all())
    for phase in phases_w:
        x, w, _, want = R.onehot_w_case(m, n, k, phase, dtype)
        assert R.exact_sum_ok(x, w) and R.full_mantissa(x, dtype)


def test_one_hot_indices_cover_every_k():
    for count, k in [(128, 64), (128, 704), (1, 64), (17, 320), (16, 704), (80, 448)]:
        seen = np.concatenate([R._spread(count, k, p) for p in range(R.spread_phases(count, k))])
        assert set(seen.tolist()) == set(range(k))


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_sum_ok_rejects_sums_that_round(dtype):
    x, w, b = R.rounding_case(dtype)
    assert R.representable(x, dtype) and not R.exact_sum_ok(x, w, b)
    got = (x.float() @ w.float().T)  # ... and it does round: 2^12 + 2^-13 is no float32
    assert not torch.equal(got.double(), x.double() @ w.double().T)
    # a dense-integer case scaled so that the 24 bits no longer hold the sum; a bias that breaks the common 2^q; inf
    xd, wd, bd, _ = R.dense_int_case(16, 16, 704, dtype)
    assert R.exact_sum_ok(xd, wd, bd)
    fine = torch.full((16,), 2.0 ** -20)
    assert not R.exact_sum_ok(xd, wd, fine)  # q = -20, and sum |x w| is beyond 2^4 (checked, not assumed):
    assert float((xd.double().abs() @ wd.double().abs().T).min()) >= 2.0 ** 4
    xi = xd.clone()
    xi[3, 5] = float("inf")
    assert not R.exact_sum_ok(xi, wd, bd)
    huge = xd.float() * 2.0 ** 100
    assert R.exact_sum_ok(huge, wd) and not R.exact_sum_ok(huge, wd * 2.0 ** 20)  # q + 24 > 128


@pytest.mark.parametrize("n,k", R.SMALL_NK + ((256, 704),))
def test_dense_integer_sums_do_not_depend_on_the_order(n, k):
    """float32 sums over k in three shuffled orders, and slice by slice in the library's split with an ascending combine,
    all equal the float64 answer bit for bit."""
    from genlm_backend_amd import _lib

    lib = _lib.load()  # (host functions only: no GPU is touched)
    m = 33
    x, w, b, _ = R.dense_int_case(m, n, k, torch.float16)
    x32, w32, b32 = x.float().numpy(), w.numpy(), b.float().numpy()
    want = x32.astype(np.float64) @ w32.astype(np.float64).T + b32.astype(np.float64)
    prod = x32[:, None, :] * w32[None, :, :]  # float32 products [m, n, k], exact
    assert np.array_equal(prod.astype(np.float64), x32.astype(np.float64)[:, None, :] * w32.astype(np.float64)[None, :, :])
    rng = np.random.default_rng(n + k)
    for _ in range(3):
        acc = np.zeros((m, n), np.float32)
        for kk in rng.permutation(k):
            acc = (acc + prod[:, :, kk]).astype(np.float32)
        assert np.array_equal((acc + b32[None, :]).astype(np.float32).astype(np.float64), want)
    ksplit = R.ksplit_of(lib, m, n, k)
    parts = []
    for kb0, kb1 in R.slice_blocks(k // R.BLOCK, ksplit):
        acc = np.zeros((m, n), np.float32)
        for kk in range(kb0 * R.BLOCK, kb1 * R.BLOCK):
            acc = (acc + prod[:, :, kk]).astype(np.float32)
        parts.append(acc)
    total = parts[0]
    for p in parts[1:]:
        total = (total + p).astype(np.float32)
    assert np.array_equal((total + b32[None, :]).astype(np.float32).astype(np.float64), want)
    assert sum(b - a for a, b in R.slice_blocks(k // R.BLOCK, ksplit)) == k // R.BLOCK


def test_grid_holds_every_split_class():
    """From the library's own workspace sizes (host code): the grid has every class of K split the GPU test relies on."""
    from genlm_backend_amd import _lib

    found = R.ksplit_classes(_lib.load())
    print("\nksplit classes:", {c: v for c, v in found.items()})
    missing = [c for c, v in found.items() if not v]
    assert not missing, f"the edge grid no longer holds: {missing} (have the constants of glb_quant.hip changed?)"
