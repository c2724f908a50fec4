"""The split-bf16 GEMM with its A operand loaded straight into registers and three blocks per CU: the bits of
the kernel that staged A through LDS (recorded under tests/golden/split_gemm_bits/), the register prefetch at its shortest
K and at ragged M with NaN all round the operand, the kernel's residency as the runtime reports it, and a time that follows
the rows instead of jumping at 512 tiles."""
import hashlib
import json
import os
import re
import statistics

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "split_gemm_bits")
BIT_SHAPES = [(129, 256, 128), (130, 384, 768), (257, 128, 3072)]  # (m, n, k): 4, 24 and 96 K steps, a ragged last row tile


def bit_operands(m, n, k):
    """Seeded Gaussian a [m, k], w [k, n], bias [n] (numpy's generator: the same on every machine) and their SHA-256."""
    rng = np.random.default_rng(1000 * m + n + k)
    a = rng.standard_normal((m, k), dtype=np.float32)
    w = rng.standard_normal((k, n), dtype=np.float32)
    b = rng.standard_normal(n, dtype=np.float32)
    sha = hashlib.sha256(a.tobytes() + w.tobytes() + b.tobytes()).hexdigest()
    return a, w, b, sha


def bit_outputs(engine, a, w, b):
    """(plain, gelu) outputs of the kernel for A as a view of pitch k + 4 (what recorded the fixtures, and what the test runs)."""
    m, k = a.shape
    buf = torch.zeros(m, k + 4, device="cuda")
    buf[:, :k] = torch.from_numpy(a).cuda()
    view = buf[:, :k]
    assert view.stride(0) == k + 4
    img = engine.gemm_split_weights(torch.from_numpy(w).cuda())
    bd = torch.from_numpy(b).cuda()
    return tuple(engine.gemm_split(view, img, w.shape[1], bd, gelu=g).cpu() for g in (False, True))


@pytest.mark.parametrize("m,n,k", BIT_SHAPES)
def test_same_bits_as_the_kernel_that_staged_a_in_lds(engine, m, n, k):
    a, w, b, sha = bit_operands(m, n, k)
    recorded = json.load(open(os.path.join(GOLDEN, "operands_sha256.json")))
    assert recorded[f"{m}x{n}x{k}"] == sha, (
        f"numpy generated other operands for {m}x{n}x{k} here than where the fixtures were recorded: "
        f"the recorded outputs do not apply (sha256 {sha}, recorded {recorded[f'{m}x{n}x{k}']})")
    for name, got in zip(("bias", "gelu"), bit_outputs(engine, a, w, b)):
        want = torch.from_numpy(np.load(os.path.join(GOLDEN, f"{m}x{n}x{k}_{name}.npy")))
        assert got.shape == want.shape
        assert torch.equal(got, want), (name, int((got != want).sum()))
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), name  # (signs of zero too)


class _Conv1D(torch.nn.Module):  # what SplitConv1D takes its parameters from
    def __init__(self, w, b):
        super().__init__()
        self.nx, self.nf = w.shape
        self.weight, self.bias = torch.nn.Parameter(w, requires_grad=False), torch.nn.Parameter(b, requires_grad=False)


@pytest.fixture(scope="module")
def short_k(engine):
    """Per k: the weight, its SplitConv1D (serving from one row) and 129 Gaussian rows, made once."""
    from genlm_backend_amd.fuse import SplitConv1D

    out = {}
    for k in (64, 128):  # (k % 64 == 0 is the shape rule: test_k_96_is_not_served)
        g = torch.Generator().manual_seed(k)
        w, b, a = torch.randn(k, 256, generator=g).cuda(), torch.randn(256, generator=g).cuda(), torch.randn(129, k, generator=g).cuda()
        out[k] = (SplitConv1D(_Conv1D(w, b), engine, 1), engine.gemm_split_weights(w), b, a)
    return out


def test_k_96_is_not_served(engine):
    """Three K steps would be the next-shortest prefetch; the day the shape rule admits k = 96, add it to the cases below."""
    assert not engine.gemm_split_supports(96, 256)


@pytest.mark.parametrize("k", [64, 128])
@pytest.mark.parametrize("m", [1, 15, 16, 17, 127, 128, 129])
def test_short_k_and_ragged_m_read_nothing_outside_the_window(engine, short_k, m, k):
    conv, img, b, a = short_k[k]
    clean = a[:m].contiguous()
    lda = k + 8
    buf = torch.full((m + 3, lda), float("nan"), device="cuda")  # one row of NaN above, two below, four columns each side
    view = buf[1:1 + m, 4:4 + k]
    view.copy_(clean)
    assert view.data_ptr() % 16 == 0 and view.stride(0) == lda and torch.isnan(buf).sum().item() == buf.numel() - m * k
    for gelu in (False, True):
        got = engine.gemm_split(view, img, 256, b, gelu=gelu)
        with torch.no_grad():
            want = conv(clean, act=torch.nn.GELU(approximate="tanh") if gelu else None)
        assert got is not None and torch.isfinite(got).all(), (m, k, gelu)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (m, k, gelu)


@pytest.mark.parametrize("gelu", [False, True])
def test_three_blocks_per_cu(engine, gelu):
    assert "gfx950" in torch.cuda.get_device_properties(0).gcnArchName
    assert engine.gemm_split_blocks_per_cu(gelu) >= 3


def staircase_ratio(engine, rounds=5, iters=10):
    """time(M = 11520: 540 tiles) / time(M = 9216: 432 tiles) of mlp.c_proj (N = 768, K = 3072), the two alternating in one
    process, median of `rounds` x `iters` calls each (as tools/split_gemm_ab.py times)."""
    n, k = 768, 3072
    g = torch.Generator(device="cuda").manual_seed(0)
    w = torch.randn(k, n, device="cuda", generator=g) * 0.02
    bias = torch.randn(n, device="cuda", generator=g) * 0.05
    img = engine.gemm_split_weights(w)
    xs = {m: torch.randn(m, k, device="cuda", generator=g) for m in (9216, 11520)}
    outs = {m: torch.empty(m, n, device="cuda") for m in xs}

    def time(m):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            engine.gemm_split(xs[m], img, n, bias, out=outs[m])
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / iters

    for m in xs:
        time(m)
    t = {m: [] for m in xs}
    for _ in range(rounds):
        for m in xs:
            t[m].append(time(m))
    us = {m: statistics.median(v) for m, v in t.items()}
    return us[11520] / us[9216], us


def test_time_follows_the_rows_across_512_tiles(engine):
    """Proportional to rows is 1.25; the kernel with two blocks per CU paid a second round (its ratio, measured on the same
    machine as this kernel's, is in profiles/r14/staircase.txt).  The bound is the midpoint of the two."""
    text = open(os.path.join(ROOT, "profiles", "r14", "staircase.txt")).read()
    parent = float(re.search(r"^parent_ratio\s+([0-9.]+)", text, re.M).group(1))
    bound = 0.5 * (1.25 + parent)
    ratio, us = staircase_ratio(engine)
    print(f"t(11520) / t(9216) = {ratio:.3f} ({us[11520]:.1f} us / {us[9216]:.1f} us); parent {parent:.3f}, bound {bound:.3f}")
    assert ratio < bound, (ratio, bound, us)
