"""float64 reference of glb_importance_step (include/glb.h), written from its formulas:

    y = float32(q * scale) when scale != 1        qt(j) ∝ exp(y_j + m_j)        token ~ qt
    dlogw = (p_tok - lse(p)) - (y_tok - lse(y + m))

Inputs are taken as the exact values of their element type (float32, float16, or uint16 words holding bfloat16) and widened
to float64 before anything is added.  The draw is two inverse CDFs: R1 / 2^64 over the masses of the 4096-index chunks in
chunk order, R2 / 2^64 over the chosen chunk's elements in index order; `Row.chunk_interval` / `Row.elem_interval` give the
interval of [0, 1) that selects a token's chunk, and the token inside it.  R1, R2 come from the library's own Philox block
function (glb_philox4x32_10), counter = (global particle index, offset), key = seed.
"""
import ctypes as C

import numpy as np

CHUNK = 4096


def bf16_bits(x):
    """float32 array -> uint16 words of its bfloat16 rounding (nearest even; -inf and NaN keep their class)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r).astype(np.uint16)


def widen(a):
    """The exact float64 values of an array of float32 / float16 / bfloat16 words (uint16)."""
    a = np.asarray(a)
    if a.dtype == np.uint16:
        return (a.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    assert a.dtype in (np.float32, np.float16), a.dtype
    return a.astype(np.float64)


def proposal_values(q, scale):
    """y of the contract: the element's float32 value times float32(scale), rounded to float32 - when scale != 1."""
    q = np.asarray(q)
    q32 = (q.astype(np.uint32) << 16).view(np.float32) if q.dtype == np.uint16 else q.astype(np.float32)
    if scale != 1:
        with np.errstate(invalid="ignore"):
            q32 = (q32 * np.float32(scale)).astype(np.float32)
    return q32.astype(np.float64)


def mask_values(kind, row, V):
    """The additive log-mask of one mask row: kind 0 none, 1 bit words (uint32 / int32), 2 floats."""
    if kind == 0:
        return np.zeros(V)
    if kind == 1:
        w = np.ascontiguousarray(row).view(np.uint32)
        j = np.arange(V)
        return np.where((w[j >> 5] >> (j & 31).astype(np.uint32)) & 1, 0.0, -np.inf)
    return np.asarray(row[:V], np.float32).astype(np.float64)


def lse(x):
    m = np.max(x) if x.size else -np.inf
    if not np.isfinite(m):
        return -np.inf
    return float(m + np.log(np.sum(np.exp(x - m))))


class Row:
    """One (target row, proposal values, mask values), all float64 [V]."""

    def __init__(self, p, y, m):
        self.p, self.y, self.m = p, y, m
        with np.errstate(invalid="ignore"):
            z = y + m
        z = np.where(np.isnan(z), -np.inf, z)
        self.V = len(p)
        self.lse_p, self.lse_y, self.lse_z = lse(p), lse(y), lse(z)
        self.empty = not np.isfinite(self.lse_z)
        self.qt = np.zeros(self.V) if self.empty else np.exp(z - self.lse_z)
        self.logZ_proposal = -np.inf if self.empty else self.lse_z - self.lse_y
        self._cum = {}
        self.nch = (self.V + CHUNK - 1) // CHUNK
        self.mass = np.array([self.qt[c * CHUNK:(c + 1) * CHUNK].sum() for c in range(self.nch)])

    def dlogw(self, j=None):
        """dlogw of token j (None: every token; -inf where p is -inf, NaN where qt is 0: never drawn)."""
        with np.errstate(invalid="ignore"):
            d = (self.p - self.lse_p) - (self.y - self.lse_z)
        d = np.where(np.isneginf(self.p), -np.inf, d)
        d = np.where(self.qt > 0, d, np.nan)
        return d if j is None else float(d[j])

    def target_mass(self):
        """Z = sum_j softmax(p)_j e^{m_j}."""
        if not np.isfinite(self.lse_p):
            return 0.0
        dead = np.isneginf(self.p) | np.isneginf(self.m)
        return float(np.sum(np.exp(np.where(dead, -np.inf, self.p - self.lse_p + np.where(dead, 0.0, self.m)))))

    def chunk_interval(self, c):
        """[lo, hi) of R1 / 2^64 that selects chunk c."""
        cum = np.concatenate([[0.0], np.cumsum(self.mass)])
        return float(cum[c] / cum[-1]), float(cum[c + 1] / cum[-1])

    def elem_interval(self, j):
        """[lo, hi) of R2 / 2^64 that selects token j inside its chunk."""
        c = j // CHUNK
        if c not in self._cum:
            self._cum[c] = np.concatenate([[0.0], np.cumsum(self.qt[c * CHUNK:(c + 1) * CHUNK])])
        cum, k = self._cum[c], j - c * CHUNK
        return float(cum[k] / cum[-1]), float(cum[k + 1] / cum[-1])


def philox_pair(seed, offset, gidx):
    """(R1, R2) of global particle `gidx`: the library's Philox4x32-10 block, words 0,1 and 2,3, low word first."""
    from genlm_backend_amd import _lib

    lib = _lib.load()
    ctr = (C.c_uint32 * 4)(gidx & 0xFFFFFFFF, (gidx >> 32) & 0xFFFFFFFF, offset & 0xFFFFFFFF, (offset >> 32) & 0xFFFFFFFF)
    key = (C.c_uint32 * 2)(seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    out = (C.c_uint32 * 4)()
    lib.glb_philox4x32_10(ctr, key, out)
    return (out[1] << 32) | out[0], (out[3] << 32) | out[2]


def uniforms(seed, offset, gidx):
    r1, r2 = philox_pair(seed, offset, gidx)
    return r1 / 2.0 ** 64, r2 / 2.0 ** 64
