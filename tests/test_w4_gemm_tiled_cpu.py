"""glb_w4_gemm_tiled on a host without a GPU: the symbols, the argument checks (they return before any GPU work), the
"tiled" mode of quant.bind, and W4Linear under "tiled" on an engine that has no such kernel."""
import ctypes as C

import pytest
import torch

from genlm_backend_amd import _lib, quant
from tests import quant4_engine as Q


def _args(**kw):
    a = _lib.W4TiledArgs()
    buf = (C.c_char * 64)()
    cb = (C.c_float * 16)(*Q.codebook("nf4"))
    a.struct_size, a.dtype, a.form = C.sizeof(_lib.W4TiledArgs), _lib.BF16, 0
    a.m, a.n, a.k, a.ldx, a.ldy = 4, 32, 64, 64, 32
    a.x = a.image = a.y = C.addressof(buf)  # (never dereferenced: every call below is refused)
    a.codebook = cb
    for name, v in kw.items():
        setattr(a, name, v)
    a._keep = (buf, cb)
    return a


def test_symbols_and_argument_errors():
    lib = _lib.load()
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("glb_w4_gemm_tiled_forms", "glb_w4_gemm_tiled"):
        assert name in _lib.SYMBOLS and hasattr(raw, name)
    forms = lib.glb_w4_gemm_tiled_forms()
    assert forms >= 2
    assert lib.glb_w4_gemm_tiled(None, None) == _lib.GLB_EINVAL
    bad = [dict(struct_size=8), dict(dtype=_lib.F32), dict(form=forms + 1), dict(form=-1), dict(ldx=63), dict(x=None),
           dict(image=None), dict(y=None), dict(codebook=None)]
    for kw in bad:
        assert lib.glb_w4_gemm_tiled(C.byref(_args(**kw)), None) == _lib.GLB_EINVAL, kw
    assert lib.glb_w4_gemm_tiled(C.byref(_args(n=24, ldy=24)), None) == _lib.GLB_EUNSUPPORTED
    assert lib.glb_w4_gemm_tiled(C.byref(_args(k=96, ldx=96)), None) == _lib.GLB_EUNSUPPORTED


def test_tiled_mode_on_an_engine_without_the_kernel():
    eng = Q.StubW4Engine()
    assert not hasattr(eng, "w4_gemm_tiled")
    n, k = 32, 128
    g = torch.Generator().manual_seed(0)
    w, x = torch.randn(n, k, generator=g), torch.randn(3, 50, k, generator=g).bfloat16()
    scratch = quant.W4Scratch(eng.device)
    scratch.reserve(n * k, torch.bfloat16)
    lin = quant.W4Linear(eng.w4_quantize(w, quant.NF4), None, k, n, "nf4", None, eng, scratch)
    net = torch.nn.Sequential(lin)
    assert "tiled" in quant.W4_GEMM_MODES and quant.bind(net, eng, "tiled") == 1 and lin.mode == "tiled"
    with pytest.raises(ValueError):
        quant.bind(net, eng, "sometimes")
    y = lin(x)
    lin.mode = "dequant"
    assert y.shape == (3, 50, n) and torch.equal(y, lin(x))
    assert isinstance(quant.ROWS_TILED, dict)
