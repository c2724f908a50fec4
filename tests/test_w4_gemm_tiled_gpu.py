"""glb_w4_gemm_tiled (the many-row 4-bit GEMM) per tile form and dtype at the smallest shapes at which each
of its mechanisms can fail: m at the tile edges of both row sizes and a third partial row tile, n of one column group, a
full 64 plus one group and a full 128 plus one, k of one, two and three blocks (prologue only, each LDS buffer once, first
reuse) and eleven.  Exact answers bit for bit where no float32 addition can round (tests/w4_gemm_ref.py), bits compared
between forms, row counts and the few-row kernel where the sums round, the 2x-of-F.linear rule of tests/test_quant4_gpu.py
against float64, containment, and W4Linear under w4_gemm="tiled".  Every call reads X at a pitch of k + 8 with NaN between
and after the rows and writes Y at a pitch of n + 8 inside guard values that must come back untouched.

Measured on an MI355X (this file's 24 tests): 16 s of wall time, the libraries' set-up included; the slowest case is
the dense-integer grid of one (form, dtype), 2.1 s for its 168 calls."""
import numpy as np
import pytest
import torch

from genlm_backend_amd import _lib, quant
from tests import quant4_engine as Q
from tests import w4_gemm_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
NAN = float("nan")
EXACT = tuple(float(v) for v in R.EXACT_CB)
MS, NS, KS = (1, 63, 64, 65, 128, 129, 257), (16, 80, 144), (64, 128, 192, 704)
FORMS = range(1, _lib.load().glb_w4_gemm_tiled_forms() + 1)
DTYPES = (torch.bfloat16, torch.float16)
form_dtype = pytest.mark.parametrize("form,dtype", [(f, d) for f in FORMS for d in DTYPES])
by_dtype = pytest.mark.parametrize("dtype", DTYPES)


def _tiled(engine, x, img, n, cb, bias=None, form=0):
    """One glb_w4_gemm_tiled call on host operands through guarded, padded buffers; Y on the host."""
    m, k = x.shape
    xbuf = torch.full((m * (k + 8) + GUARD,), NAN, dtype=x.dtype, device=DEV)
    xd = xbuf[:m * (k + 8)].view(m, k + 8)[:, :k]
    xd.copy_(x)
    ld = n + 8
    ybuf = torch.full((GUARD + m * ld + GUARD,), 7.0, dtype=x.dtype, device=DEV)
    yd = ybuf[GUARD:GUARD + m * ld].view(m, ld)[:, :n]
    assert engine.w4_gemm_tiled(xd, img, n, cb, None if bias is None else bias.to(DEV), out=yd, form=form) is not None
    host = ybuf.cpu()
    body = host[GUARD:GUARD + m * ld].view(m, ld)
    assert bool((host[:GUARD] == 7).all() and (host[GUARD + m * ld:] == 7).all() and (body[:, n:] == 7).all()), (m, n, k)
    return body[:, :n].contiguous()


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


def _gauss(engine, n, k, dtype, name, m=257):
    g = torch.Generator().manual_seed(n + k + sum(name.encode()))  # (its own X, W and bias per codebook)
    cb = tuple(Q.codebook(name))
    w = torch.randn(n, k // 64, 64, generator=g) * torch.exp(torch.rand(n, k // 64, 1, generator=g) * 4.0 - 3.0)
    x = torch.randn(m, k, generator=g).to(dtype)
    b = (torch.randn(n, generator=g) * 0.5).to(dtype)
    img = engine.w4_quantize(w.view(n, k).to(DEV), cb)
    return x, b, img, engine.w4_dequantize(img, n, k, cb, dtype=dtype), cb, w.view(n, k)


@form_dtype
def test_dense_integers_exact(engine, form, dtype):
    for n in NS:
        for k in KS:
            rng = np.random.default_rng([n, k])
            x = torch.from_numpy(rng.integers(-4, 5, size=(MS[-1], k)).astype(np.float32))
            b = torch.from_numpy(rng.integers(-255, 256, size=n).astype(np.float32))
            w, _ = R.exact_weights(n, k)
            assert R.exact_sum_ok(x, w, b) and R.exact_sum_ok(x, w)
            img = engine.w4_quantize(w.to(DEV), EXACT)
            prod = x.double() @ w.double().T
            for bias, want in ((b.to(dtype), (prod + b.double()).float().to(dtype)), (None, prod.float().to(dtype))):
                for m in MS:
                    got = _tiled(engine, x[:m].to(dtype), img, n, EXACT, bias, form)
                    assert torch.equal(got, want[:m]), (n, k, m, bias is not None, int((got != want[:m]).sum()))


@form_dtype
def test_selection_through_w_exact(engine, form, dtype):
    g = torch.Generator().manual_seed(5)
    for n in NS:
        for k in KS:
            kj = (np.arange(n) * 37 + 5) % k
            s = np.ldexp(1.0, np.arange(n) % 5 - 2)
            w = torch.zeros(n, k)
            w[torch.arange(n), torch.from_numpy(kj)] = torch.from_numpy(-s).float()
            r = torch.randn(MS[-1], k, generator=g)
            x = (torch.sign(r) * (r.abs() + 0.5)).to(dtype)  # full mantissas, and no product below the normal range
            assert R.exact_sum_ok(x, w)
            want = (x.double()[:, kj] * torch.from_numpy(-s)[None, :]).to(dtype)
            img = engine.w4_quantize(w.to(DEV), EXACT)
            for m in MS:
                assert _same(_tiled(engine, x[:m], img, n, EXACT, None, form), want[:m]), (n, k, m)


@by_dtype
@pytest.mark.parametrize("name", ["nf4", "fp4"])
def test_sums_that_round(engine, dtype, name):
    n, k = 144, 704
    x, b, img, wq, cb, _ = _gauss(engine, n, k, dtype, name)
    full = _tiled(engine, x, img, n, cb, b)
    assert bool(torch.isfinite(full).all())
    for form in FORMS:  # (a) every form, the same bits; (b) the rows of a smaller call are the rows of the large one
        assert _same(_tiled(engine, x, img, n, cb, b, form), full), form
        for m in (1, 65, 129):
            assert _same(_tiled(engine, x[:m], img, n, cb, b, form), full[:m]), (form, m)
    # (d) against float64 on W': within twice F.linear's error on the dequantised weight
    ref = x.double() @ wq.double().cpu().T + b.double()
    lib = torch.nn.functional.linear(x.to(DEV), wq, b.to(DEV)).double().cpu()
    e_max, l_max = (full.double() - ref).abs().max().item(), (lib - ref).abs().max().item()
    e_fro, l_fro = ((full.double() - ref).norm() / ref.norm()).item(), ((lib - ref).norm() / ref.norm()).item()
    print(f"tiled {dtype} {name}: max {e_max:.3e} (lib {l_max:.3e}) fro {e_fro:.3e} (lib {l_fro:.3e})")
    assert e_max <= 2 * l_max + 1e-30 and e_fro <= 2 * l_fro + 1e-30, (e_max, l_max, e_fro, l_fro)
    for k1 in (64, 128):  # (c) a single K slice of the few-row kernel: its bits
        x1, b1, img1, _, _, _ = _gauss(engine, n, k1, dtype, name, m=128)
        for m in (1, 65, 128):
            assert engine.lib.glb_w4_gemm_workspace_bytes(m, n, k1) == 4 * m * n
            few = engine.w4_gemm(x1[:m].to(DEV), img1, n, cb, b1.to(DEV)).cpu()
            for form in FORMS:
                assert _same(_tiled(engine, x1[:m], img1, n, cb, b1, form), few), (k1, m, form)


@form_dtype
def test_containment(engine, form, dtype):
    n, k, m = 144, 192, 129
    x, b, img, wq, cb, w = _gauss(engine, n, k, dtype, "nf4", m)
    clean = _tiled(engine, x, img, n, cb, b, form)
    assert bool(torch.isfinite(clean).all())
    bad = x.clone()
    bad[63, 5], bad[64, 100] = NAN, float("inf")
    got = _tiled(engine, bad, img, n, cb, b, form)
    keep = torch.ones(m, dtype=torch.bool)
    keep[[63, 64]] = False
    assert _same(got[keep], clean[keep]) and not bool(torch.isfinite(got[~keep]).any())
    j_inf, j_zero = 37, 130
    wb = w.clone()
    blk = wb[j_inf, 64:128]
    wb[j_inf, 64:128] = blk / blk.abs().max() * (1e5 if dtype == torch.float16 else 3.4e38)
    wb[j_zero, 128:192] = 0.0
    got = _tiled(engine, x, engine.w4_quantize(wb.to(DEV), cb), n, cb, b, form)
    cols = torch.ones(n, dtype=torch.bool)
    cols[[j_inf, j_zero]] = False
    assert _same(got[:, cols], clean[:, cols])
    assert not bool(torch.isfinite(got[:, j_inf]).any()) and bool(torch.isfinite(got[:, j_zero]).all())


@by_dtype
def test_w4linear_tiled(engine, dtype, monkeypatch):
    n, k = 144, 192
    x, b, img, _, cb, _ = _gauss(engine, n, k, dtype, "nf4", 150)
    scratch = quant.W4Scratch(engine.device)
    scratch.reserve(n * k, dtype)
    scratch.reserve(n * k, torch.float32)
    lin = quant.W4Linear(img, b.to(DEV), k, n, "nf4", None, engine, scratch)
    lin.mode = "tiled"
    monkeypatch.setitem(quant.MIN_ROWS_FUSED, (n, k), 64)
    deq = engine.w4_dequantize

    def no_dequantize(*a, **kw):
        raise AssertionError("w4_dequantize called")

    monkeypatch.setattr(engine, "w4_dequantize", no_dequantize)
    y = lin(x.view(3, 50, k).to(DEV))
    assert y.shape == (3, 50, n) and _same(y.cpu().view(150, n), _tiled(engine, x, img, n, cb, b))
    monkeypatch.setattr(engine, "w4_gemm_tiled", no_dequantize)  # 7 rows: the few-row rule, glb_w4_gemm
    assert _same(lin(x[:7].to(DEV)).cpu(), engine.w4_gemm(x[:7].to(DEV), img, n, cb, b.to(DEV)).cpu())
    with pytest.raises(AssertionError, match="w4_dequantize called"):  # float32 activations still dequantise
        lin(x[:7].float().to(DEV))
    monkeypatch.setattr(engine, "w4_dequantize", deq)
    assert lin(x[:7].float().to(DEV)).dtype == torch.float32
