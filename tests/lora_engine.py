"""The arithmetic contract of glb_lora_merge (include/glb.h) restated bit for bit in numpy, and a test double
of `HipEngine` that merges adapters with it.  TEST INFRASTRUCTURE: lives under tests/, is never imported by the product.

    acc = +0.0f;  for t = 0 .. r-1 ascending: acc = fmaf(f32(B[i, t]), f32(A[t, j]), acc)
    out[i, j] = round_to_w_dtype(fmaf(scale, acc, f32(W[i, j])))

Python 3.10 has no math.fma: `fmaf` below forms the product exactly in float64 (24 + 24 bits), adds c with TwoSum (s + e ==
p + c exactly) and rounds s to float32; rounding s is the correctly rounded result except when s lies exactly on a float32
midpoint and e != 0, where the true value is on e's side of the midpoint.
"""
import numpy as np
import torch

from tests.cpu_engine import CpuOracleEngine


def fmaf(a, b, c):
    """Correctly rounded float32 fma of float32 arrays (finite values; broadcasting)."""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    p = a * b  # exact
    s = p + c
    bp = s - c
    e = (p - bp) + (c - (s - bp))  # TwoSum: s + e == p + c
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    toward = np.where(r64 < s, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
    other = np.nextafter(r, toward)
    mid = (r64 != s) & ((r64 + other.astype(np.float64)) * 0.5 == s)
    # on a midpoint with a nonzero error the true value lies on e's side: take the neighbour there
    up = mid & (e > 0) & (r64 < s)
    down = mid & (e < 0) & (r64 > s)
    r = np.where(up | down, other, r)
    return r.astype(np.float32)


def to_f32(t):
    """float32 numpy copy of a tensor (exact for float32 / bfloat16 / float16)."""
    return t.detach().to("cpu", torch.float32).numpy()


def round_to(x32, dtype):
    """float32 numpy -> tensor of `dtype`, round to nearest even (NaN stays NaN)."""
    if dtype == torch.float32:
        return torch.from_numpy(np.ascontiguousarray(x32, np.float32))
    if dtype == torch.float16:
        return torch.from_numpy(np.ascontiguousarray(x32, np.float32).astype(np.float16))
    u = np.ascontiguousarray(x32, np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    rounded = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    h = np.where(nan, (u >> 16) | 0x40, rounded).astype(np.uint16)
    return torch.from_numpy(h.view(np.int16)).view(torch.bfloat16)


def lora_delta_acc(a32, b32):
    """acc[i, j] of the contract: float32 [n_out, r] x [r, k_in] -> float32 [n_out, k_in]."""
    acc = np.zeros((b32.shape[0], a32.shape[1]), np.float32)
    for t in range(a32.shape[0]):
        acc = fmaf(b32[:, t:t + 1], a32[t:t + 1, :], acc)
    return acc


def lora_merge_ref(w, a, b, scale, transposed=False):
    """The contract's result as a CPU tensor of w's dtype and shape."""
    acc = lora_delta_acc(to_f32(a), to_f32(b))
    if transposed:
        acc = acc.T
    out = fmaf(np.float32(scale), acc, to_f32(w))
    return round_to(out, w.dtype)


class LoraOracleEngine(CpuOracleEngine):
    """CpuOracleEngine with HipEngine.lora_merge restated by the contract (writes every job's `out`)."""

    merges = 0

    def lora_merge(self, jobs):
        for j in jobs:
            got = lora_merge_ref(j["w"], j["a"], j["b"], j["scale"], bool(j.get("transposed", False)))
            j["out"].copy_(got.to(j["out"].device))
        self.merges += 1
