"""The arithmetic of the split-bf16 GEMM (genlm-backend_amd/csrc/glb_gemm.hip), restated on the CPU with torch's bf16
rounding (round to nearest even, as v_cvt_pk_bf16_f32): x = hi + mid + lo exactly, and the six-product sum the kernel
accumulates (mid.mid, lo.hi, hi.lo, mid.hi, hi.mid, hi.hi) stays within the bound of the three dropped products."""
import numpy as np
import pytest
import torch


def split3(x):
    """float32 -> (hi, mid, lo) float32 tensors holding bf16 values; each residual an exact float32 subtraction."""
    hi = x.to(torch.bfloat16).float()
    r1 = x - hi
    mid = r1.to(torch.bfloat16).float()
    r2 = r1 - mid
    lo = r2.to(torch.bfloat16).float()
    return hi, mid, lo


def test_three_bf16_parts_reproduce_x_exactly():
    g = torch.Generator().manual_seed(0)
    vals = [torch.randn(100000, generator=g), torch.randn(10000, generator=g) * 1e30, torch.randn(10000, generator=g) * 1e-30,
            torch.rand(10000, generator=g) * 2 - 1]
    special = torch.tensor([0.0, -0.0, 1.0, -1.0, 1e30, -1e30, 1e-30, -1e-30, 3.4e37, -3.4e37, 1.1754944e-38 * 2 ** 20,
                            np.nextafter(np.float32(1), np.float32(2)), np.float32(1) / 3, -np.float32(2) / 3,
                            np.float32(16777215.0), np.float32(0.1)], dtype=torch.float32)
    # every mantissa pattern of the low 16 bits at one exponent (the bits the two smaller parts must carry)
    pattern = (torch.arange(1 << 16, dtype=torch.int32) | (127 << 23) | (0x55 << 16)).view(torch.float32)
    for x in vals + [special, pattern, -pattern]:
        hi, mid, lo = split3(x)
        s = (hi + mid) + lo
        normal = x.abs() >= 2.0 ** -109  # lo (at most 2^-17 |x|) is then a normal number: the split is exact
        assert torch.equal(s[normal], x[normal])
        # below, lo falls among bf16's subnormals (spacing 2^-133): the split is exact to that spacing
        assert bool(((s - x).abs() <= 2.0 ** -134).all())
        assert torch.equal(lo.to(torch.bfloat16).float(), lo)  # lo is exactly a bf16 value
        # magnitudes: |mid| <= 2^-8 |hi|, |lo| <= 2^-8 |mid| (round to nearest: half an ulp of an 8-bit significand)
        assert bool((mid.abs() <= hi.abs() * 2.0 ** -8).all()) and bool((lo.abs() <= mid.abs() * 2.0 ** -8).all())


def six_term_product(a, w):
    """a [M, K] @ w [K, N] as the kernel sums it, in float64 over exact products (the accumulation order is the
    hardware's; what is tested here is the truncation: the three dropped products)."""
    ah, am, al = (t.double() for t in split3(a))
    wh, wm, wl = (t.double() for t in split3(w))
    return am @ wm + al @ wh + ah @ wl + am @ wh + ah @ wm + ah @ wh


@pytest.mark.parametrize("n,k", [(2304, 768), (768, 768), (3072, 768), (768, 3072)])
def test_six_products_are_fp32_accurate(n, k):
    g = torch.Generator().manual_seed(n + k)
    m = 16
    a = torch.randn(m, k, generator=g) * 2.0 + 0.1
    w = torch.randn(k, n, generator=g) * 0.02
    exact = a.double() @ w.double()
    err = (six_term_product(a, w) - exact).abs()
    bound = a.double().abs() @ w.double().abs()  # sum |a||w| over k
    # the dropped mid.lo + lo.mid + lo.lo: at most (2 * 2^-16 * 2^-8 + 2^-32) of each |a||w|, below fp32's unit roundoff
    assert bool((err <= bound * 2.0 ** -23.5).all())
    assert bool((err <= bound * 2.0 ** -24).all())
    # ... and a float32 GEMM on the CPU makes a larger error than the truncation does
    f32 = (a @ w).double()
    assert (err.norm() / exact.norm()) < ((f32 - exact).norm() / exact.norm())
