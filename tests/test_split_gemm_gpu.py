"""The split-bf16 MFMA GEMM (glb_gemm_f32_split, fuse.SplitConv1D) on the GPU: fp32-accurate against float64 - max |err| and
the relative Frobenius error each within 2x those of torch.addmm in fp32 on the same inputs -, the bias + tanh GELU
epilogue, shapes it does not serve, and a hipGraph replay that gives the eager call's bits."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(2304, 768), (768, 768), (3072, 768), (768, 3072)]  # (N, K) of GPT-2 small's four projections
ROWS = [1, 37, 1024, 11520 + 7]


def _inputs(m, n, k, scaled, seed):
    g = torch.Generator().manual_seed(seed)
    if scaled:  # GPT-2-like: layer-normed activations, weights ~ N(0, 0.02), small biases
        x = torch.randn(m, k, generator=g) * 2.0 + 0.1
        w = torch.randn(k, n, generator=g) * 0.02
        b = torch.randn(n, generator=g) * 0.05
    else:
        x = torch.randn(m, k, generator=g)
        w = torch.randn(k, n, generator=g)
        b = torch.randn(n, generator=g)
    return x, w, b


def _errors(y, ref):
    d = (y.double().cpu() - ref)
    return d.abs().max().item(), (d.norm() / ref.norm()).item()


def _gelu64(t):
    return 0.5 * t * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (t + 0.044715 * t ** 3)))


@pytest.mark.parametrize("n,k", SHAPES)
@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("scaled", [False, True])
def test_split_gemm_is_fp32_accurate(engine, n, k, m, scaled):
    x, w, b = _inputs(m, n, k, scaled, seed=m * 7 + n + k)
    ref = torch.addmm(b.double(), x.double(), w.double())
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    img = engine.gemm_split_weights(wd)
    assert img is not None and img.numel() == 6 * k * n
    y = engine.gemm_split(xd, img, n, bd)
    lib = torch.addmm(bd, xd, wd)
    torch.cuda.synchronize()
    e_max, e_fro = _errors(y, ref)
    l_max, l_fro = _errors(lib, ref)
    assert e_max <= 2 * l_max + 1e-30 and e_fro <= 2 * l_fro + 1e-30, (e_max, l_max, e_fro, l_fro)


@pytest.mark.parametrize("n,k", [(3072, 768), (2304, 768)])
@pytest.mark.parametrize("m", [37, 11520 + 7])
def test_split_gemm_gelu_epilogue(engine, n, k, m):
    x, w, b = _inputs(m, n, k, True, seed=11 + m)
    ref = _gelu64(torch.addmm(b.double(), x.double(), w.double()))
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    y = engine.gemm_split(xd, engine.gemm_split_weights(wd), n, bd, gelu=True)
    lib = torch.nn.functional.gelu(torch.addmm(bd, xd, wd), approximate="tanh")
    torch.cuda.synchronize()
    e_max, e_fro = _errors(y, ref)
    l_max, l_fro = _errors(lib, ref)
    assert e_max <= 2 * l_max and e_fro <= 2 * l_fro, (e_max, l_max, e_fro, l_fro)


def test_split_gemm_strided_rows_and_no_bias(engine):
    n, k, m = 768, 768, 300
    x, w, _ = _inputs(m, n, 2 * k, False, seed=5)
    xs = x.cuda()[:, k:]  # row pitch 2K
    wd = w[:k].contiguous().cuda()
    y = engine.gemm_split(xs, engine.gemm_split_weights(wd), n, None)
    ref = x[:, k:].double() @ w[:k].double()
    lib = xs @ wd
    e_max, _ = _errors(y, ref)
    l_max, _ = _errors(lib, ref)
    assert e_max <= 2 * l_max


def test_unsupported_shapes_fall_back(engine):
    from genlm_backend_amd import _lib

    assert not engine.gemm_split_supports(768, 50257) and not engine.gemm_split_supports(40, 768)
    assert engine.gemm_split_weights(torch.randn(768, 1000, device="cuda")) is None
    img = engine.gemm_split_weights(torch.randn(768, 768, device="cuda"))
    xm = torch.randn(8, 769, device="cuda")[:, 1:]  # rows not 16-byte aligned: unsupported, not an error
    assert engine.gemm_split(xm, img, 768) is None
    a = _lib.GemmArgs()
    a.struct_size = 3
    assert engine.lib.glb_gemm_f32_split(C.byref(a), None) == _lib.GLB_EINVAL
    # the module runs torch.addmm for what the kernel does not take
    from genlm_backend_amd.fuse import SplitConv1D
    from transformers.pytorch_utils import Conv1D

    src = Conv1D(768, 768).cuda()
    mod = SplitConv1D(src, engine, min_rows=16)
    x = torch.randn(4, 5, 768, device="cuda")  # 20 rows: the kernel
    y = mod(x)
    assert y.shape == (4, 5, 768) and torch.allclose(y, src(x), rtol=1e-5, atol=1e-5)
    x = torch.randn(3, 768, device="cuda")
    assert torch.equal(mod(x), src(x))  # 3 rows: library, bit for bit
    x = torch.randn(3, 768, device="cuda", dtype=torch.float64)
    assert mod.weight.dtype == torch.float32
    with pytest.raises(RuntimeError):
        mod(x)  # as Conv1D itself: dtype mismatch is torch's error


def test_graph_replay_gives_the_eager_bits(engine):
    n, k, m = 3072, 768, 1031
    x, w, b = _inputs(m, n, k, True, seed=3)
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    img = engine.gemm_split_weights(wd)
    eager = engine.gemm_split(xd, img, n, bd, gelu=True).clone()
    out = torch.empty(m, n, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        engine.gemm_split(xd, img, n, bd, gelu=True, out=out)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    out.zero_()
    with torch.cuda.graph(g):
        engine.gemm_split(xd, img, n, bd, gelu=True, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
