"""The two tile forms of glb_gemm_f32_split (128 x 128 and 64 x 64: DESIGN.md §12) give the same bits: every call here is
made once with each form forced (glb_gemm_f32_split_form) on the same inputs and compared with torch.equal - plain and
padded, with both epilogues, across the small form's tile edges and the XCD remap's modulus, with hostile elements, and a
row alone against the row in a batch.  No tolerance appears."""
import pytest
import torch

from genlm_backend_amd import _lib

pytestmark = pytest.mark.gpu

LARGE, SMALL = _lib.GEMM_FORM_LARGE, _lib.GEMM_FORM_SMALL
FLT_MAX = 3.4028234663852886e38
MS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200)  # around the 16-row fragment, the 64-row and the 128-row tile
NS = (128, 256, 384)
KS = (64, 128, 768)
# (m, n) whose small-form block counts ceil(m / 64) * (n / 64) are 6, 8, 10, 16 and 18: below, on and above multiples of 8
REMAP = ((192, 128, 6), (256, 128, 8), (320, 128, 10), (512, 128, 16), (513, 128, 18), (129, 256, 12), (65, 384, 12))


def _bits(x):
    return x.contiguous().view(torch.int32)


def _gauss_full(shape, g):
    """Gaussian values with the lowest significand bit set: all three bf16 parts of the split carry bits."""
    return (torch.randn(shape, generator=g).view(torch.int32) | 1).view(torch.float32)


def _operands(m, n, k, seed):
    g = torch.Generator().manual_seed(seed)
    a, w = _gauss_full((m, k), g), _gauss_full((k, n), g)
    return a.cuda(), w.cuda(), torch.randn(n, generator=g).cuda()


def _both(engine, a, img, n, bias, gelu):
    yl = engine.gemm_split(a, img, n, bias, gelu=gelu, form=LARGE)
    ys = engine.gemm_split(a, img, n, bias, gelu=gelu, form=SMALL)
    assert yl is not None and ys is not None
    return yl, ys


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_forms_agree_bit_for_bit(engine, n, k):
    a_all, w, bias = _operands(max(MS), n, k, seed=n + k)
    img = engine.gemm_split_weights(w)
    for m in MS:
        a = a_all[:m]
        for gelu in (False, True):
            yl, ys = _both(engine, a, img, n, bias, gelu)
            assert bool(torch.isfinite(yl).all()) and torch.equal(_bits(yl), _bits(ys)), (m, gelu)
            auto = engine.gemm_split(a, img, n, bias, gelu=gelu)  # whichever form the library picks
            assert torch.equal(_bits(auto), _bits(yl)), (m, gelu)


@pytest.mark.parametrize("m,n,blocks", REMAP)
def test_forms_agree_around_the_xcd_remap(engine, m, n, blocks):
    assert -(-m // 64) * (n // 64) == blocks
    a, w, bias = _operands(m, n, 128, seed=m + n)
    img = engine.gemm_split_weights(w)
    for gelu in (False, True):
        yl, ys = _both(engine, a, img, n, bias, gelu)
        assert torch.equal(_bits(yl), _bits(ys)), gelu
    # every row and column was written by some block: against a one-row-tile call of the same rows
    ys = engine.gemm_split(a, img, n, bias, form=SMALL)
    for r0 in range(0, m, 64):
        assert torch.equal(_bits(engine.gemm_split(a[r0:r0 + 64], img, n, bias, form=SMALL)), _bits(ys[r0:r0 + 64])), r0


@pytest.mark.parametrize("m,n,k", [(1, 128, 64), (17, 256, 128), (65, 128, 768), (129, 384, 64), (200, 256, 768)])
def test_forms_agree_with_padded_rows(engine, m, n, k):
    """lda > k, ldc > n: A's padding is NaN (reading it would poison a row), C's padding holds a canary that must survive."""
    a, w, bias = _operands(m, n, k, seed=m * n + k)
    img = engine.gemm_split_weights(w)
    wide_a = torch.full((m + 1, k + 4), float("nan"), device="cuda")  # (a NaN row behind the last one as well)
    wide_a[:m, :k] = a
    a_view = wide_a[:m, :k]
    assert a_view.stride(0) == k + 4 and a_view.data_ptr() % 16 == 0
    canary = torch.arange((m + 1) * (n + 3), dtype=torch.int32, device="cuda").reshape(m + 1, n + 3) | 0x7FC00000
    for gelu in (False, True):
        plain_l, plain_s = _both(engine, a, img, n, bias, gelu)
        for form, plain in ((LARGE, plain_l), (SMALL, plain_s)):
            buf = canary.clone().view(torch.float32)
            out = buf[:m, :n]
            y = engine.gemm_split(a_view, img, n, bias, gelu=gelu, out=out, form=form)
            assert y.data_ptr() == out.data_ptr()
            assert torch.equal(_bits(out), _bits(plain)), (form, gelu)
            got = buf.view(torch.int32)
            assert torch.equal(got[:m, n:], canary[:m, n:]) and torch.equal(got[m:], canary[m:]), (form, gelu)
        assert torch.equal(_bits(plain_l), _bits(plain_s)), gelu


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), FLT_MAX, -FLT_MAX])
def test_forms_agree_on_hostile_elements(engine, bad):
    m, n, k = 129, 256, 128
    a, w, bias = _operands(m, n, k, seed=11)
    a[70, 37] = bad   # the small form's second row tile, the large form's third wave
    w[45, 200] = bad  # the small form's fourth column tile
    img = engine.gemm_split_weights(w)
    for gelu in (False, True):
        yl, ys = _both(engine, a, img, n, bias, gelu)
        fl, fs = torch.isfinite(yl), torch.isfinite(ys)
        assert torch.equal(fl, fs), gelu
        assert not bool(fl[70].any()) and not bool(fl[:, 200].any())  # the row and the column, as include/glb.h says
        keep = torch.ones(m, n, dtype=torch.bool, device="cuda")
        keep[70], keep[:, 200] = False, False
        assert bool(fl[keep].all())
        assert torch.equal(_bits(yl)[fl], _bits(ys)[fs]), gelu


def test_a_row_alone_in_the_small_form_equals_the_batch_in_the_large(engine):
    m, n, k = 129, 384, 768
    a, w, bias = _operands(m, n, k, seed=5)
    img = engine.gemm_split_weights(w)
    for gelu in (False, True):
        batch = engine.gemm_split(a, img, n, bias, gelu=gelu, form=LARGE)
        for i in (0, 63, 64, 127, 128):
            alone = engine.gemm_split(a[i:i + 1], img, n, bias, gelu=gelu, form=SMALL)
            assert torch.equal(_bits(alone), _bits(batch[i:i + 1])), (i, gelu)


def test_form_argument_and_residency(engine):
    a, w, bias = _operands(16, 128, 64, seed=1)
    img = engine.gemm_split_weights(w)
    out = torch.full((16, 128), 7.0, device="cuda")
    for form in (-1, 3, 99):
        with pytest.raises(_lib.GlbError) as e:
            engine.gemm_split(a, img, 128, bias, out=out, form=form)
        assert e.value.code == _lib.GLB_EINVAL
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing was launched
    for gelu in (False, True):
        # registers and 24 KiB of LDS both admit six blocks of the small form on a CU
        assert engine.gemm_split_blocks_per_cu(gelu, form=SMALL) == 6
        assert engine.gemm_split_blocks_per_cu(gelu, form=LARGE) == engine.gemm_split_blocks_per_cu(gelu)
    with pytest.raises(_lib.GlbError):
        engine.gemm_split_blocks_per_cu(False, form=0)
