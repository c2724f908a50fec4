"""The arithmetic of the split-bf16 GEMM (genlm-backend_amd/csrc/glb_gemm.hip), restated on the CPU with torch's bf16
rounding (round to nearest even, as v_cvt_pk_bf16_f32): x = hi + mid + lo exactly, and the six-product sum the kernel
accumulates (mid.mid, lo.hi, hi.lo, mid.hi, hi.mid, hi.hi) stays within the bound of the three dropped products."""
import numpy as np
import pytest
import torch

from tests import split_gemm_ref as R
from tests.split_gemm_ref import split3


def _value_classes():
    g = torch.Generator().manual_seed(0)
    vals = [torch.randn(100000, generator=g), torch.randn(10000, generator=g) * 1e30, torch.randn(10000, generator=g) * 1e-30,
            torch.rand(10000, generator=g) * 2 - 1]
    special = torch.tensor([0.0, -0.0, 1.0, -1.0, 1e30, -1e30, 1e-30, -1e-30, 3.4e37, -3.4e37, 1.1754944e-38 * 2 ** 20,
                            np.nextafter(np.float32(1), np.float32(2)), np.float32(1) / 3, -np.float32(2) / 3,
                            np.float32(16777215.0), np.float32(0.1)], dtype=torch.float32)
    # every mantissa pattern of the low 16 bits at one exponent (the bits the two smaller parts must carry)
    pattern = (torch.arange(1 << 16, dtype=torch.int32) | (127 << 23) | (0x55 << 16)).view(torch.float32)
    return vals + [special, pattern, -pattern]


def test_three_bf16_parts_reproduce_x_exactly():
    for x in _value_classes():
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


# ---- tests/split_gemm_ref.py itself: the packed image and the exact-sum condition -------------------------------------------
def test_planes_gathered_back_from_the_image_reproduce_w():
    """split_image against the layout sentence of glb_gemm.hip's header, read back index by index: piece
    ((nb * K/32 + kb) * 3 + p), byte 16 * l, value j is plane p of W[kb*32 + 8(l>>4) + j][nb*16 + (l&15)]."""
    k, n = 64, 32
    for x in _value_classes():
        reps = -(-k * n // x.numel())
        w = x.repeat(reps)[:k * n].view(k, n).contiguous()
        img = R.split_image(w)
        assert img.dtype == torch.uint8 and img.numel() == 6 * k * n
        vals = img.view(torch.bfloat16).float().view(-1, 512)  # [piece, 64 lanes x 8 values]
        planes = torch.zeros(3, k, n)
        for nb in range(n // 16):
            for kb in range(k // 32):
                for p in range(3):
                    piece = vals[(nb * (k // 32) + kb) * 3 + p]
                    for l in range(64):
                        for j in range(8):
                            planes[p, kb * 32 + 8 * (l >> 4) + j, nb * 16 + (l & 15)] = piece[8 * l + j]
        for got, want in zip(planes, split3(w)):
            assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        s = (planes[0] + planes[1]) + planes[2]
        normal = w.abs() >= 2.0 ** -109
        assert torch.equal(s[normal], w[normal]) and bool(((s - w).abs() <= 2.0 ** -134).all())


CASES = [(1, 128, 64), (17, 128, 64), (129, 256, 128), (300, 256, 192), (300, 384, 768), (129, 768, 768), (1025, 128, 128)]


@pytest.mark.parametrize("m,n,k", CASES)
def test_exact_sum_condition_accepts_the_exact_generators(m, n, k):
    assert (m, n, k) in R.edge_grid()
    for phase in range(R.spread_phases(m, k)):
        for with_bias in (False, True):
            a, w, b, want = R.onehot_case(m, n, k, phase, with_bias)
            assert R.exact_sum_ok(a, w, b) and R.dropped_products_zero(a, w)
            assert torch.equal(want.double(), a.double() @ w.double() + (0 if b is None else b.double()))
    for phase in range(R.spread_phases(n, k)):
        a, w, want = R.selection_case(m, n, k, phase)
        assert R.exact_sum_ok(a, w) and R.dropped_products_zero(a, w)
        assert torch.equal(want.double(), a.double() @ w.double())
    for wide in ("a", "w", "both"):
        a, w, b, want = R.dense_int_case(m, n, k, wide)
        assert R.exact_sum_ok(a, w, b) and R.dropped_products_zero(a, w)
        for x in (a, w) if wide == "both" else (a,) if wide == "a" else (w,):
            hi, mid, _ = split3(x)
            assert bool(((hi != 0) & (mid != 0))[x != 0].all())  # both planes of a wide operand carry data
        assert bool((w.view(k // 32, 32, n) != 0).any(dim=1).all())  # every K block populated
        assert bool((a.view(m, k // 32, 32) != 0).any(dim=2).all())
    a, w, b, pre = R.gelu_case()
    assert R.exact_sum_ok(a, w, b) and torch.equal(pre.double(), a.double() @ w.double() + b.double())


def test_grid_has_the_tile_counts_the_remap_needs():
    grid = R.edge_grid()
    counts = {R.tiles(m, n) for m, n, _ in grid}
    assert {1, 7, 8, 9} <= counts and 55 <= len(grid) <= 65 and len(set(grid)) == len(grid)
    assert {k for _, _, k in grid} == set(R.KS) and {n for _, n, _ in grid} == set(R.NS) and set(R.MS) <= {m for m, _, _ in grid}


def test_exact_sum_condition_rejects_what_rounds():
    g = torch.Generator().manual_seed(1)
    a, w = torch.randn(16, 64, generator=g), torch.randn(64, 128, generator=g)
    assert not R.exact_sum_ok(a, w) and not R.dropped_products_zero(a, w)
    # one element at the top of its binade: hi rounds up into the next one and |hi| + |mid| + |lo| needs a 25th bit
    one = torch.zeros(1, 64)
    one[0, 63] = 1.0
    w = R.full_mantissa((64, 128), g)
    assert R.exact_sum_ok(one, w)
    w[63, 5] = float.fromhex("0x1.fffffep0")
    assert not R.exact_sum_ok(one, w)
    # a bias that is not a multiple of the terms' unit, and one that carries the sum past 24 bits
    a, w, b, _ = R.dense_int_case(16, 128, 64)
    assert not R.exact_sum_ok(a, w, b + 0.5 ** 10) and not R.exact_sum_ok(a, w, b + 2.0 ** 24)
    # operands whose split is not finite
    w[0, 0] = 3.4e38
    assert not R.exact_sum_ok(a, w, b)


def test_scaling_inputs_keep_every_part_normal():
    a, w, b = R.scaling_case(17, 128, 64)
    for s in (-60, -30, 0, 30, 60):
        assert R.parts_stay_normal(a * 2.0 ** s) and R.parts_stay_normal(w * 2.0 ** -s)
    assert bool((a.abs() >= 2.0 ** -4).all() and (a.abs() < 2.0 ** 4).all())
    assert not R.parts_stay_normal(a * 2.0 ** -110)
