"""Inputs for glb_w4_gemm (genlm-backend_amd/csrc/glb_quant.hip) whose answer is known exactly, and the condition under
which it is: every float32 addition the kernel can make - inside a K slice, in any order, and in the ascending combine of
the slices - is exact.  CPU only (numpy, torch on the CPU and tests/quant4_engine.py); TEST INFRASTRUCTURE, never imported
by the product package.  tests/test_w4_gemm_ref_cpu.py checks this file itself; tests/test_w4_gemm_exact_gpu.py builds its
inputs and expected values from it.

Orientation: x is [m, k], w is [n, k] (nn.Linear's), y = x . w^T + bias is [m, n].  Builders return torch tensors: x, bias
and the expected y in the 16-bit dtype of the call, w in float32 (the source glb_w4_quantize reads)."""
import functools

import numpy as np
import torch

from tests import quant4_engine as Q

BLOCK = Q.BLOCK
NONE = 1 << 20  # "no nonzero element": larger than any exponent sum
MANT_BITS = {torch.bfloat16: 8, torch.float16: 11}  # significand bits, the implicit one included

# The 16 values j / 8, j = -8 .. 7, in the fixed order j_i = (5 i + 3) % 16 - 8: not sorted, so the code of a value is not
# its sorted index and the quantiser's code_of table matters.  Sorted, the entries are (i - 8) / 8 and the 15 midpoints
# (2 i - 15) / 16: all exact.  For a block of values c * s (c in the table, s a power of two) that holds at least one -s,
# absmax is s (|c| <= 1), midpoint * absmax is exact, the code of c * s is the code of c and codebook[code] * absmax is
# c * s again - four significant bits, so exact in float32, bfloat16 and float16 alike.
EXACT_CB = np.array([((5 * i + 3) % 16 - 8) / 8.0 for i in range(16)], dtype=np.float32)
CODE_NEG1 = int(np.nonzero(EXACT_CB == -1.0)[0][0])

M_GRID = (1, 15, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 127, 128)  # first and last m of every MF = 1 .. 8
M_GRID_LARGE = (1, 17, 128)
M_MAX = 128
SMALL_NK = tuple((n, k) for n in (16, 32, 80) for k in (64, 128, 192, 256, 320, 448, 704))
LARGE_NK = ((24000, 704), (65536, 256))


def edge_grid():
    """The (n, k) of the edge-shape calls: every small n with every small k, and the two shapes whose split is decided by
    n (what splits they get is the library's business: ksplit_of and ksplit_classes ask it)."""
    return list(SMALL_NK) + list(LARGE_NK)


def m_grid(n, k):
    return M_GRID if (n, k) in SMALL_NK else M_GRID_LARGE


def ksplit_of(engine_or_lib, m, n, k):
    """The number of K slices the library uses for (n, k): its own workspace size over the 4 m n bytes of one slice."""
    lib = getattr(engine_or_lib, "lib", engine_or_lib)
    nbytes = int(lib.glb_w4_gemm_workspace_bytes(m, n, k))
    assert nbytes > 0 and nbytes % (4 * m * n) == 0, (m, n, k, nbytes)
    return nbytes // (4 * m * n)


def slice_blocks(kb_count, ksplit):
    """[(kb0, kb1)] of the slices: kb0 = ks * kb_count / ksplit (include/glb.h does not fix it; glb_quant.hip does)."""
    return [(ks * kb_count // ksplit, (ks + 1) * kb_count // ksplit) for ks in range(ksplit)]


CLASSES = ("one block in a single slice", "two blocks in a single slice", "three blocks in a single slice", "an even split",
           "an uneven split bound by k", "an uneven split bound by n", "a single slice of four blocks or more")


def ksplit_classes(engine_or_lib, grid=None):
    """{class: [(n, k, ksplit)]} over the grid, from the library's answers alone.  A split is "bound by k" when the same n
    with twice the k gets more slices, "bound by n" when it does not."""
    found = {c: [] for c in CLASSES}
    for n, k in grid or edge_grid():
        ks, kb = ksplit_of(engine_or_lib, 1, n, k), k // BLOCK
        if ks == 1:
            if kb <= 3:
                found[CLASSES[kb - 1]].append((n, k, ks))
            else:
                found[CLASSES[6]].append((n, k, ks))
        elif kb % ks == 0:
            found[CLASSES[3]].append((n, k, ks))
        elif ksplit_of(engine_or_lib, 1, n, 2 * k) > ks:
            found[CLASSES[4]].append((n, k, ks))
        else:
            found[CLASSES[5]].append((n, k, ks))
    return found


# ---- exactness ----------------------------------------------------------------------------------------------------------------
def _np64(t):
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        t = t.detach().double().cpu().numpy()
    return np.asarray(t, np.float64)


def _unit_exponent(v):
    """Per element of a float64 array of float32 values: the largest e with v an integer multiple of 2^e (NONE where
    v == 0), read from the float32 bit pattern (torch's int32 arithmetic: the large-n weights have 17 M elements)."""
    v64 = torch.from_numpy(np.ascontiguousarray(v))
    v32 = v64.float()
    assert torch.equal(v32.double(), v64), "operands must be float32 values"
    bits = v32.view(torch.int32) & 0x7FFFFFFF
    exp = bits >> 23
    mant = (bits & 0x7FFFFF) | ((exp > 0).to(torch.int32) << 23)  # (subnormals have no implicit bit)
    low = mant & -mant  # its lowest set bit
    tz = (low.float().view(torch.int32) >> 23) - 127  # log2(low)
    e = exp.clamp(min=1) - 150 + tz
    return torch.where(bits == 0, torch.full_like(e, NONE), e).numpy()


def representable(t, dtype):
    """True when every element of the tensor is a value of `dtype`."""
    t = t.detach().double()
    return bool((t.to(dtype).double() == t).all())


def full_mantissa(t, dtype):
    """True when every element uses all significand bits of `dtype`: the lowest one is set (and the value is normal)."""
    v = _np64(t)
    _, exp = np.frexp(v)
    return bool((v != 0).all() and (_unit_exponent(v) == exp - MANT_BITS[dtype]).all()
                and (np.abs(v) >= float(torch.finfo(dtype).tiny)).all())


def exact_sum_ok(x, w, bias=None):
    """True when y = x . w^T + bias cannot depend on the order of the float32 additions: for every output element (i, j)
    there is one 2^q of which every product x[i, k] w[j, k], and bias[j], is an integer multiple, and
    sum_k |x w| + |bias| < 2^(q + 24) - every partial sum, in any order, inside a slice or across slices, is then a multiple
    of 2^q below 2^(q + 24), a float32 value, and no addition rounds.  (The products themselves are exact in float32: two
    operands of at most 11 significant bits.)  q is taken per output element: the product's own unit exponent where a row
    of x or a row of w has a single nonzero, else the lower bound min_k + min_k - the condition stays sufficient.
    Everything must stay a normal float32: q >= -126 and q + 24 <= 128; operands and bias must be finite."""
    x, w, b = _np64(x), _np64(w), _np64(bias)
    if not (np.isfinite(x).all() and np.isfinite(w).all() and (b is None or np.isfinite(b).all())):
        return False
    (m, k), n = x.shape, w.shape[0]
    assert w.shape == (n, k) and (b is None or b.shape == (n,))
    ex, ew = _unit_exponent(x), _unit_exponent(w)
    if ((x != 0).sum(1) <= 1).all():
        ki = (x != 0).argmax(1)  # (a row of zeros: ex is NONE there)
        q = ex[np.arange(m), ki][:, None] + ew[:, ki].T
    elif ((w != 0).sum(1) <= 1).all():
        kj = (w != 0).argmax(1)
        q = ex[:, kj] + ew[np.arange(n), kj][None, :]
    else:
        q = ex.min(1)[:, None] + ew.min(1)[None, :]
    total = np.abs(x) @ np.abs(w).T  # float64: exact while below 2^(q + 53), and far out of bound beyond
    if b is not None:
        q = np.minimum(q, _unit_exponent(b)[None, :])
        total = total + np.abs(b)[None, :]
    live = q < NONE // 2  # (an output with no nonzero term at all is exactly zero)
    if not live.any():
        return True
    q, total = q[live], total[live]
    if int(q.min()) < -126 or int(q.max()) + 24 > 128:
        return False
    return bool((total < np.ldexp(1.0, q + 24)).all())


# ---- builders -------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([int(v) for v in key])


@functools.lru_cache(maxsize=3)
def _exact_weights(n, k):
    """float32 [n, k] of values c * 2^e, c drawn from EXACT_CB, every block with one -2^e at a drawn place; e = (row +
    2 * block) % 4 differs from that of the rows above and below, of the blocks before and after and of the four diagonal
    neighbours: a block multiplied by a neighbour's absmax gives another sum.  Vectorised (the large n take 17 M elements)."""
    rng = _rng(1, n, k)
    kb = k // BLOCK
    idx = rng.integers(0, 16, size=(n, kb, BLOCK), dtype=np.uint8)
    np.put_along_axis(idx, rng.integers(0, BLOCK, size=(n, kb, 1)), np.uint8(CODE_NEG1), axis=2)
    e = (np.arange(n)[:, None] + 2 * np.arange(kb)[None, :]) % 4
    w = EXACT_CB[idx] * np.ldexp(np.float32(1), e)[:, :, None].astype(np.float32)
    w = w.reshape(n, k)
    w.setflags(write=False)
    return w


def exact_weights(n, k):
    """(w float32 [n, k] tensor, e int [n, k / 64]): absmax of block (row, kb) is 2^e."""
    e = (np.arange(n)[:, None] + 2 * np.arange(k // BLOCK)[None, :]) % 4
    return torch.from_numpy(_exact_weights(n, k).copy()), e


def _spread(count, k, phase):
    """count indices into 0 .. k - 1, spread over all of K (every slice is hit in one call once count >= its slices); over
    the phases 0 .. spread_phases(count, k) - 1 they are every index."""
    return (phase + np.arange(count) * spread_phases(count, k)) % k


def spread_phases(count, k):
    return -(-k // count)


def onehot_x(m, k, phase, dtype, unit=False):
    """(x [m, k] of `dtype`, kidx [m], value [m]): x[i, kidx[i]] = value[i] = 2^(i % 3 - 1) (1 with `unit`), zeros elsewhere."""
    kidx = _spread(m, k, phase)
    val = np.ones(m) if unit else np.ldexp(1.0, np.arange(m) % 3 - 1)
    x = np.zeros((m, k), np.float32)
    x[np.arange(m), kidx] = val
    return torch.from_numpy(x).to(dtype), kidx, val


def onehot_x_case(m, n, k, phase, dtype):
    """Rows of x are unit vectors times 2^(i % 3 - 1); w = exact_weights.  y[i, :] = value[i] * w[:, kidx[i]]: a column of
    W'.  Returns x, w, None, expected."""
    x, kidx, val = onehot_x(m, k, phase, dtype)
    w = _exact_weights(n, k)
    want = torch.from_numpy(w[:, kidx].T.astype(np.float64) * val[:, None])
    assert representable(want, dtype)
    return x, torch.from_numpy(w.copy()), None, want.to(dtype)


@functools.lru_cache(maxsize=4)
def _full_mantissa_rows(k, dtype):
    """[M_MAX, k] float64 values of `dtype` with every significand bit in use (the lowest one set), random sign, binary
    exponent -2 .. 2."""
    rng = _rng(2, k, MANT_BITS[dtype])
    p = MANT_BITS[dtype]
    frac = rng.integers(0, 1 << (p - 2), size=(M_MAX, k)) * 2 + 1  # odd, below 2^(p - 1)
    v = ((1 << (p - 1)) + frac).astype(np.float64) * 2.0 ** -(p - 1)  # 1.f with the last bit of f set
    v = v * rng.choice([-1.0, 1.0], size=(M_MAX, k)) * np.ldexp(1.0, rng.integers(-2, 3, size=(M_MAX, k)))
    v.setflags(write=False)
    return v


def onehot_w_case(m, n, k, phase, dtype):
    """Row j of w (column j of y) has the single nonzero w[j, k_j] = -s_j, s_j = 2^(j % 5 - 2): its block holds -s_j and
    zeros (absmax s_j, codes exact), every other block of the row is zero (absmax 0: W' = +-0).  x: the first m of 128 rows
    of full-mantissa values.  y[:, j] = -s_j x[:, k_j], exact: a power-of-two scaling well inside the dtype's range.
    Returns x, w, None, expected."""
    kj = _spread(n, k, phase)
    s = np.ldexp(1.0, np.arange(n) % 5 - 2)
    w = np.zeros((n, k), np.float32)
    w[np.arange(n), kj] = -s
    xv = _full_mantissa_rows(k, dtype)[:m]
    x = torch.from_numpy(xv.copy())
    assert representable(x, dtype) and full_mantissa(x, dtype)
    want = torch.from_numpy(xv[:, kj] * -s[None, :])
    assert representable(want, dtype) and bool((want.abs() >= float(torch.finfo(dtype).tiny)).all())
    return x.to(dtype), torch.from_numpy(w), None, want.to(dtype)


@functools.lru_cache(maxsize=2)
def _dense_full(n, k):
    rng = _rng(3, n, k)
    x = rng.integers(-4, 5, size=(M_MAX, k)).astype(np.float32)
    bias = rng.integers(-255, 256, size=n).astype(np.float32)  # (integers up to 255: values of bfloat16 and float16)
    w = _exact_weights(n, k)
    prod = x.astype(np.float64) @ w.astype(np.float64).T  # sums of multiples of 1/8 below 2^15: exact in float64
    for a in (x, bias, prod):
        a.setflags(write=False)
    return x, w, bias, prod


def dense_int_case(m, n, k, dtype, with_bias=True):
    """x: the first m of 128 rows of integers, |x| <= 4; w = exact_weights (multiples of 1/8 with a per-block power of two
    up to 8); bias: integers, |b| <= 255.  Every product is a multiple of 1/8 and sum |x w| + |b| <= 704 * 32 + 255 < 2^21:
    exact_sum_ok holds by a factor of 64.  Expected: the float64 result - itself exact - rounded ONCE to the dtype.
    Returns x, w, bias, expected."""
    x, w, bias, prod = _dense_full(n, k)
    want = prod[:m] + (bias.astype(np.float64)[None, :] if with_bias else 0.0)
    want = torch.from_numpy(want)
    assert bool((want.float().double() == want).all())  # a float32 value: .to(dtype) below is the one rounding
    b = torch.from_numpy(bias.copy()).to(dtype) if with_bias else None
    return torch.from_numpy(x[:m].copy()).to(dtype), torch.from_numpy(w.copy()), b, want.float().to(dtype)


def rounding_case(dtype):
    """A case made to round, which exact_sum_ok must reject: 2^12 + 2^-12 + ... spans more than 24 bits in one output."""
    k = BLOCK
    x = torch.zeros(1, k)
    x[0, 0], x[0, 1] = 2.0 ** 12, 2.0 ** -6
    w = torch.zeros(16, k)
    w[:, 0], w[:, 1] = 1.0, 2.0 ** -7  # products 2^12 and 2^-13: 26 bits apart
    return x.to(dtype), w, None
