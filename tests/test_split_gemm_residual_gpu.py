"""The residual epilogue of the split GEMM (glb_gemm_f32_split_residual: C = (acc + bias) + R) against
`gemm_split(x, ...)` followed by torch's add in both operand orders: torch.equal throughout, both tile forms forced, rows
around the 16-row fragment and the 64- / 128-row tiles, padded C and R with canaries, C = R in place, a non-finite element
of R, a row alone against the row in its batch, and the calls the entry point refuses before any launch."""
import ctypes as C

import pytest
import torch

from genlm_backend_amd import _lib

pytestmark = pytest.mark.gpu

LARGE, SMALL = _lib.GEMM_FORM_LARGE, _lib.GEMM_FORM_SMALL
KN = ((64, 128), (128, 384), (512, 128))
MS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 300)
CANARY = -123456.0


def _bits(x):
    return x.contiguous().view(torch.int32)


def _case(engine, k, n):
    g = torch.Generator().manual_seed(1000 * k + n)
    m = max(MS)
    a = (torch.randn((m, k), generator=g).view(torch.int32) | 1).view(torch.float32).cuda()
    w = (torch.randn((k, n), generator=g).view(torch.int32) | 1).view(torch.float32).cuda()
    return a, engine.gemm_split_weights(w), torch.randn(n, generator=g).cuda(), (3 * torch.randn((m, n), generator=g)).cuda()


@pytest.fixture(scope="module", params=KN, ids=lambda kn: f"k{kn[0]}-n{kn[1]}")
def case(request, engine):
    a, img, bias, r = _case(engine, *request.param)
    plain = engine.gemm_split(a, img, request.param[1], bias)  # the reference: computed once, rows independent of the batch
    return request.param + (a, img, bias, r, plain)


@pytest.mark.parametrize("form", (LARGE, SMALL), ids=("large", "small"))
def test_equals_gemm_then_add(engine, case, form):
    k, n, a, img, bias, r, plain = case
    for m in MS:
        y = engine.gemm_split(a[:m], img, n, bias, form=form)
        assert torch.equal(_bits(y), _bits(plain[:m])), m  # (a row's bits do not depend on the batch)
        got = engine.gemm_split(a[:m], img, n, bias, form=form, residual=r[:m])
        assert torch.equal(_bits(got), _bits(y + r[:m])) and torch.equal(_bits(got), _bits(r[:m] + y)), m
    got = engine.gemm_split(a[:65], img, n, None, form=form, residual=r[:65])  # no bias: acc + 0, then R
    assert torch.equal(_bits(got), _bits(engine.gemm_split(a[:65], img, n, None, form=form) + r[:65]))


@pytest.mark.parametrize("form", (LARGE, SMALL), ids=("large", "small"))
def test_padded_rows_and_canaries(engine, case, form):
    k, n, a, img, bias, r, plain = case
    for m in (1, 17, 65, 129, 300):
        cbuf = torch.full((m + 2, n + 24), CANARY, device="cuda")
        rbuf = torch.full((m + 2, n + 8), float("nan"), device="cuda")  # (whatever is read around R's rows poisons C)
        rbuf[1:m + 1, 4:n + 4] = r[:m]
        rbuf_was = rbuf.clone()
        out, res = cbuf[1:m + 1, 8:n + 8], rbuf[1:m + 1, 4:n + 4]
        engine.gemm_split(a[:m], img, n, bias, out=out, form=form, residual=res)
        assert torch.equal(_bits(out), _bits(plain[:m] + r[:m])), m
        ring = torch.ones_like(cbuf, dtype=torch.bool)
        ring[1:m + 1, 8:n + 8] = False
        assert bool((cbuf[ring] == CANARY).all()), m
        assert torch.equal(_bits(rbuf), _bits(rbuf_was)), m


@pytest.mark.parametrize("form", (LARGE, SMALL), ids=("large", "small"))
def test_in_place_on_the_residual(engine, case, form):
    k, n, a, img, bias, r, plain = case
    for m in (1, 63, 64, 129, 300):
        buf = torch.full((m + 2, n + 16), CANARY, device="cuda")
        view = buf[1:m + 1, :n]
        view.copy_(r[:m])
        got = engine.gemm_split(a[:m], img, n, bias, out=view, form=form, residual=view)
        assert got.data_ptr() == view.data_ptr()
        assert torch.equal(_bits(view), _bits(plain[:m] + r[:m])), m
        assert bool((buf[0] == CANARY).all() and (buf[m + 1] == CANARY).all() and (buf[1:m + 1, n:] == CANARY).all()), m


@pytest.mark.parametrize("form", (LARGE, SMALL), ids=("large", "small"))
def test_non_finite_residual_stays_in_its_element(engine, case, form):
    k, n, a, img, bias, r, plain = case
    m = 129
    want = plain[:m] + r[:m]
    for value, (i, j) in ((float("nan"), (0, 0)), (float("inf"), (64, n - 1)), (float("-inf"), (128, 17))):
        bad = r[:m].clone()
        bad[i, j] = value
        got = engine.gemm_split(a[:m], img, n, bias, form=form, residual=bad)
        assert not bool(torch.isfinite(got[i, j]))
        same = torch.ones((m, n), dtype=torch.bool, device="cuda")
        same[i, j] = False
        assert torch.equal(_bits(got)[same], _bits(want)[same])


@pytest.mark.parametrize("form", (LARGE, SMALL), ids=("large", "small"))
def test_a_row_alone_equals_the_row_in_its_batch(engine, case, form):
    k, n, a, img, bias, r, plain = case
    full = engine.gemm_split(a, img, n, bias, form=form, residual=r)
    for i in (0, 15, 16, 63, 64, 127, 128, 299):
        alone = engine.gemm_split(a[i:i + 1], img, n, bias, form=form, residual=r[i:i + 1])
        assert torch.equal(_bits(alone[0]), _bits(full[i])), i


def _args(a, img, n, bias, out, epilogue=_lib.GEMM_BIAS):
    g = _lib.GemmArgs()
    g.struct_size = C.sizeof(_lib.GemmArgs)
    g.m, g.n, g.k = a.shape[0], n, a.shape[1]
    g.a, g.lda, g.w_split, g.bias = a.data_ptr(), a.stride(0), img.data_ptr(), bias.data_ptr()
    g.c, g.ldc, g.epilogue = out.data_ptr(), out.stride(0), epilogue
    return g


def test_refusals_launch_nothing(engine, case):
    k, n, a, img, bias, r, plain = case
    m = 64
    out = torch.full((2 * m, n), CANARY, device="cuda")
    stream = engine._stream()
    call = engine.lib.glb_gemm_f32_split_residual
    with pytest.raises(ValueError):
        engine.gemm_split(a[:m], img, n, bias, gelu=True, residual=r[:m])  # GELU with a residual
    with pytest.raises(ValueError):
        engine.gemm_split(a[:m], img, n, bias, residual=r[:m].cpu())  # the wrong device
    with pytest.raises(ValueError):
        engine.gemm_split(a[:m], img, n, bias, residual=r[:m + 1])  # the wrong shape
    with pytest.raises(_lib.GlbError):
        engine.gemm_split(a[:m], img, n, bias, out=out[:m], residual=out[1:m + 1])  # a partial overlap of C and R
    with pytest.raises(_lib.GlbError):
        engine.gemm_split(a[:m], img, n, bias, out=out[:m], residual=out.view(m, 2 * n)[:, :n])  # same pointer, other pitch
    g = _args(a[:m], img, n, bias, out[:m])
    assert call(C.byref(g), r.data_ptr() + 2, n, 0, stream) == _lib.GLB_EINVAL  # misaligned
    assert call(C.byref(g), r.data_ptr(), n - 1, 0, stream) == _lib.GLB_EINVAL  # pitch below n
    assert call(C.byref(g), None, n, 0, stream) == _lib.GLB_EINVAL
    assert call(C.byref(g), r.data_ptr(), n, 7, stream) == _lib.GLB_EINVAL  # no such form
    host = torch.zeros((m, n))
    assert call(C.byref(g), host.data_ptr(), n, 0, stream) == _lib.GLB_EINVAL  # host memory
    assert "device" in _lib.last_error()
    g = _args(a[:m], img, n, bias, out[:m], _lib.GEMM_BIAS_GELU_TANH)
    assert call(C.byref(g), r.data_ptr(), n, 0, stream) == _lib.GLB_EINVAL
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())  # nothing ran
    assert call(C.byref(_args(a[:m], img, n, bias, out[:m])), r.data_ptr(), n, 0, stream) == _lib.GLB_OK  # the runtime is fine
    torch.cuda.synchronize()
    assert torch.equal(_bits(out[:m]), _bits(plain[:m] + r[:m]))
