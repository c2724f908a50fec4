"""The split-bf16 GEMM (genlm-backend_amd/csrc/glb_gemm.hip) restated on the CPU in plain torch: the three-way bf16 split,
the packed weight image byte for byte, and the condition under which the kernel's answer is known exactly - every
addition it can make, in any order and at any internal width of at least 24 bits, is exact.  The GPU tests build their
inputs and expected values from this file; tests/test_split_gemm_cpu.py checks the file itself."""
import torch

KEPT = ((1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0))  # (plane of a, plane of w) of the six products, 0 = hi, 1 = mid, 2 = lo
DROPPED = ((1, 2), (2, 1), (2, 2))
BF16_MAX = float.fromhex("0x1.fep127")  # largest bf16 value
BF16_OVER = float.fromhex("0x1.ffp127")  # the smallest |x| that rounds to a bf16 infinity (a tie, to the even 2^128)
NONE = 1 << 20  # "no nonzero element": larger than any exponent sum


def split3(x):
    """float32 -> (hi, mid, lo) float32 tensors holding bf16 values; each residual an exact float32 subtraction."""
    hi = x.to(torch.bfloat16).float()
    r1 = x - hi
    mid = r1.to(torch.bfloat16).float()
    r2 = r1 - mid
    lo = r2.to(torch.bfloat16).float()
    return hi, mid, lo


def split_image(w):
    """The packed image of w [K, N] (K % 32 == 0, N % 16 == 0) as a uint8 tensor of 6 * K * N bytes: piece
    ((nb * K/32 + kb) * 3 + p) is 1 KiB and holds at byte 16 * l the eight plane-p bf16 values
    W[kb*32 + 8(l>>4) + j][nb*16 + (l&15)], j = 0..7."""
    k, n = w.shape
    assert k % 32 == 0 and n % 16 == 0
    planes = torch.stack([p.to(torch.bfloat16) for p in split3(w.float())])  # [p, K, N]; exact: the parts are bf16 values
    # K = (kb, l >> 4, j), N = (nb, l & 15)  ->  [nb, kb, p, l >> 4, l & 15, j]
    img = planes.view(3, k // 32, 4, 8, n // 16, 16).permute(4, 1, 0, 2, 5, 3).contiguous()
    return img.view(torch.uint8).reshape(-1)


def _unit_exponent(x):
    """Per element of a float64 tensor of float32-representable values: the largest e with x an integer multiple of 2^e
    (NONE where x == 0)."""
    mant, exp = torch.frexp(x)  # x = mant * 2^exp, 0.5 <= |mant| < 1, at most 24 significant bits
    m = (mant.abs() * 2.0 ** 24).to(torch.int64)  # an integer below 2^24
    low = m & -m  # its lowest set bit
    tz = torch.frexp(low.double())[1] - 1  # log2(low)
    e = exp.to(torch.int64) - 24 + tz.to(torch.int64)
    return torch.where(x == 0, torch.full_like(e, NONE), e)


def _min_plus(ea, ew, budget=1 << 25):
    """min over k of ea[i, k] + ew[k, j] (entries >= NONE // 2 mean "no term"): exact when one operand is sparse enough to
    enumerate its nonzeros, else the lower bound min_k ea[i, k] + min_k ew[k, j]."""
    (m, _), n = ea.shape, ew.shape[1]
    q = torch.full((m, n), 2 * NONE, dtype=torch.int64)
    ia, ka = torch.nonzero(ea < NONE, as_tuple=True)
    kw, jw = torch.nonzero(ew < NONE, as_tuple=True)
    if ia.numel() * n <= budget:
        return q.scatter_reduce_(0, ia[:, None].expand(-1, n), ea[ia, ka][:, None] + ew[ka, :], "amin")
    if jw.numel() * m <= budget:
        return q.scatter_reduce_(1, jw[None, :].expand(m, -1), ea[:, kw] + ew[kw, jw][None, :], "amin")
    return ea.amin(dim=1)[:, None] + ew.amin(dim=0)[None, :]


def exact_sum_ok(a, w, bias=None):
    """True when a [M, K] . w [K, N] + bias, summed as the kernel's six part-products, cannot depend on the order of the
    additions or on how the MFMA rounds inside: for every output element (i, j) there is one 2^q of which every kept
    part-product of every k, and bias[j], is an integer multiple, and sum |terms| + |bias| < 2^(q + 24) - so every partial
    sum, in any order, is a multiple of 2^q below 2^(q + 24) and therefore a float32 value.  q is found per output element
    from the unit exponents of the parts (_min_plus: the largest such q where an operand is sparse, a smaller one where
    both are dense - the condition stays sufficient).  Everything must also stay a normal float32 (q >= -126,
    q + 24 <= 128), and the bf16 parts themselves must be finite."""
    pa = [p.double() for p in split3(a.float())]
    pw = [p.double() for p in split3(w.float())]
    if not all(bool(torch.isfinite(p).all()) for p in pa + pw):
        return False
    ea, ew = [_unit_exponent(p) for p in pa], [_unit_exponent(p) for p in pw]
    q = torch.full((a.shape[0], w.shape[1]), 2 * NONE, dtype=torch.int64)
    for i, j in KEPT:
        q = torch.minimum(q, _min_plus(ea[i], ew[j]))
    aa = [p.abs() for p in pa]
    ww = [p.abs() for p in pw]
    # sum over the six kept pairs of |a_p| . |w_p'| (float64: exact while below 2^(q + 53), and far out of bound beyond)
    total = aa[0] @ (ww[0] + ww[1] + ww[2]) + aa[1] @ (ww[0] + ww[1]) + aa[2] @ ww[0]
    if bias is not None:
        b = bias.double()
        if not bool(torch.isfinite(b).all()):
            return False
        q = torch.minimum(q, _unit_exponent(b)[None, :])
        total = total + b.abs()[None, :]
    live = q < NONE // 2  # (an output with no nonzero term at all is exactly zero)
    if not bool(live.any()):
        return True
    q, total = q[live], total[live]
    if int(q.min()) < -126 or int(q.max()) + 24 > 128:
        return False
    return bool((total < torch.ldexp(torch.ones_like(total), q + 24)).all())


def dropped_products_zero(a, w):
    """True when the three products the kernel drops (mid.lo, lo.mid, lo.lo) vanish for every (i, k, j): the six kept ones
    then sum to a . w itself."""
    pa, pw = split3(a.float()), split3(w.float())
    for i, j in DROPPED:
        if bool(((pa[i] != 0).any(dim=0) & (pw[j] != 0).any(dim=1)).any()):
            return False
    return True


def parts_stay_normal(x):
    """True when every nonzero bf16 part of every element is a normal number (the split is then exact and scales with x)."""
    return all(bool(((p == 0) | ((p.abs() >= 2.0 ** -126) & torch.isfinite(p))).all()) for p in split3(x.float()))


def below_binade_top(x):
    """x with every element in the top 1/64 of its binade moved down by 1/32: |hi| + |mid| + |lo| then stays below the next
    power of two, so the three parts of one element add up exactly in any order."""
    mant, _ = torch.frexp(x)
    return torch.where(mant.abs() >= 1.0 - 1.0 / 64, x * (1.0 - 1.0 / 32), x).float()


def full_mantissa(shape, gen, exp_lo=0, exp_hi=0, per="element"):
    """Float32 values of random sign with all 24 significand bits in use (the lowest one set), outside the top 1/64 of
    their binade; binary exponents drawn from exp_lo .. exp_hi per element, per row or per column."""
    frac = torch.randint(0, 1 << 22, shape, generator=gen, dtype=torch.int64) * 2 + 1  # odd, below 2^23
    x = (1.0 + frac.double() * 2.0 ** -23).float()
    x = below_binade_top(x)
    x = (x.view(torch.int32) | 1).view(torch.float32)  # (the move may have cleared the last bit)
    sign = torch.randint(0, 2, shape, generator=gen, dtype=torch.int64) * 2 - 1
    eshape = {"element": shape, "row": (shape[0], 1), "column": (1, shape[1])}[per]
    e = torch.randint(exp_lo, exp_hi + 1, eshape, generator=gen, dtype=torch.int64)
    return (x.double() * sign.double() * torch.ldexp(torch.ones(eshape, dtype=torch.float64), e)).float()


# ---- inputs whose answer is known exactly (tests/test_split_gemm_exact_gpu.py; accepted by exact_sum_ok) -------------------
def _gen(*key):
    seed = 0
    for v in key:
        seed = seed * 1009 + int(v) + 1
    return torch.Generator().manual_seed(seed)


def _spread(count, k, phase):
    """count indices into 0 .. k-1, the first one k-1 (the last element of the last K block), spread over all of K; with
    phases 0 .. spread_phases(count, k) - 1 together they are every index when count >= k / 3."""
    stride = -(-k // count)
    return (k - 1 - phase - stride * torch.arange(count)) % k


def spread_phases(count, k):
    return min(3, -(-k // count))


def onehot_case(m, n, k, phase=0, with_bias=False):
    """A one-hot: A[i, k_i] = 2^s_i; W full 24-bit mantissas, one binary exponent per column.  C[i, :] = 2^s_i W[k_i, :]
    (+ bias).  Returns a, w, bias, expected."""
    g = _gen(1, m, n, k, phase, with_bias)
    kidx = _spread(m, k, phase)
    s = (torch.arange(m) * 3) % 5 - 2 if with_bias else (torch.arange(m) * 5) % 13 - 6
    a = torch.zeros(m, k)
    a[torch.arange(m), kidx] = torch.ldexp(torch.ones(m), s)
    e = torch.randint(-3, 4, (1, n), generator=g, dtype=torch.int64)
    w = full_mantissa((k, n), g) * torch.ldexp(torch.ones(1, n), e)
    bias = None
    want = a[torch.arange(m), kidx].double()[:, None] * w[kidx].double()
    if with_bias:  # multiples of 2^(max s + e_j - 23) below 2^(e_j - 9): exact_sum_ok decides that this is summable
        r = torch.randint(-(1 << 12), 1 << 12, (n,), generator=g, dtype=torch.int64)
        bias = (r.double() * torch.ldexp(torch.ones(n, dtype=torch.float64), e[0] - 21)).float()
        want = want + bias.double()[None, :]
    assert bool((want.float().double() == want).all())
    return a, w, bias, want.float()


def selection_case(m, n, k, phase=0):
    """W selects: column j has the one nonzero W[k_j, j] = +-1; A full 24-bit mantissas, one binary exponent per row.
    C[:, j] = +-A[:, k_j].  Returns a, w, expected."""
    g = _gen(2, m, n, k, phase)
    kidx = _spread(n, k, phase)
    sign = ((torch.arange(n) * 7) % 3 != 0).float() * 2 - 1
    w = torch.zeros(k, n)
    w[kidx, torch.arange(n)] = sign
    a = full_mantissa((m, k), g, -3, 3, per="row")
    return a, w, a[:, kidx] * sign[None, :]


def dense_int_case(m, n, k, wide="a"):
    """Integer operands and an integer bias; every K block's contribution its own.  wide = "a": A odd 10-bit integers (hi
    and mid both nonzero), W 6-bit integers times 2^(K block % 3); "w": the roles exchanged; "both": odd 9-bit integers in
    both, so that mid.mid is nonzero while every dropped product is zero - a plane that reaches the wrong product changes
    the sum.  Elements are thinned (every block keeps some) so that every sum stays below 2^24: K = 768 keeps 8 of every
    32-deep block at offsets that move with the block; "both" keeps 64 in all.  Returns a, w, bias, expected."""
    g = _gen(3, m, n, k, ("a", "w", "both").index(wide))

    def ints(shape, lo, hi, odd):
        v = torch.randint(lo, hi, shape, generator=g, dtype=torch.int64)
        v = v | 1 if odd else v
        return (v * (torch.randint(0, 2, shape, generator=g, dtype=torch.int64) * 2 - 1)).float()

    kk = torch.arange(k)
    if wide == "both":
        a, w = ints((m, k), 256, 512, True), ints((k, n), 256, 512, True)
        keep = (kk % (k // 64) == 0).float()
    else:
        a = ints((m, k), 1, 64, False) if wide == "w" else ints((m, k), 256, 1024, True)
        w = ints((k, n), 256, 1024, True) if wide == "w" else ints((k, n), 1, 64, False)
        w = w * torch.ldexp(torch.ones(k), (kk // 32) % 3)[:, None]
        keep = ((kk % 32 - 5 * (kk // 32)) % 4 == 0).float() if k > 192 else torch.ones(k)
    a, w = a * keep[None, :], w * keep[:, None]
    bias = torch.randint(-1023, 1024, (n,), generator=g, dtype=torch.int64).float()
    return a, w, bias, (a.double() @ w.double() + bias.double()).float()


def scaling_case(m, n, k):
    """Full-mantissa operands with magnitudes in [2^-4, 2^4)."""
    g = _gen(4, m, n, k)
    return full_mantissa((m, k), g, -4, 3), full_mantissa((k, n), g, -4, 3), full_mantissa((1, n), g, -4, 3)[0]


GELU_SPECIALS = (0.0, -0.0, 1e-30, -1e-30, 1e4, -1e4, 1e20, -1e20, 3.4028234663852886e38, -3.4028234663852886e38)
GELU_M, GELU_N, GELU_K = 64, 256, 64


def gelu_case():
    """One-hot A (ones) over K = 64, so the pre-activation of C[i, j] is exactly W[i, j] + bias[j]: columns 0 .. 191 carry
    12 288 values dense over [-12, 12] through W (bias 0), columns 192 .. 255 a zero W and the value in the bias: another
    64 over [-12, 12] and GELU_SPECIALS (+-FLT_MAX can only come through the bias: W's split does not take it).  Returns
    a, w, bias, pre-activation [64, 256] float32."""
    m, n, k = GELU_M, GELU_N, GELU_K
    a = torch.eye(m, k)
    w = torch.zeros(k, n)
    dense = below_binade_top(torch.linspace(-12.0, 12.0, m * 192, dtype=torch.float64).float())
    w[:, :192] = dense[torch.randperm(m * 192, generator=_gen(5))].view(m, 192)
    bias = torch.zeros(n)
    bias[192:256] = torch.linspace(-12.0, 12.0, 64, dtype=torch.float64).float()
    bias[192:192 + len(GELU_SPECIALS)] = torch.tensor(GELU_SPECIALS, dtype=torch.float64).float()
    return a, w, bias, w + bias[None, :]


def gelu_tanh64(x):
    """torch.nn.GELU(approximate="tanh") of a float32 tensor, evaluated in float64."""
    t = x.double()
    return 0.5 * t * (1.0 + torch.tanh(0.7978845608028654 * (t + 0.044715 * t ** 3)))


# ---- the shapes: K x N x M of the smallest the library serves up to one GPT-2 projection --------------------------------
KS, NS, MS = (64, 128, 192, 768), (128, 256, 384, 768), (1, 15, 16, 17, 127, 128, 129, 257, 300)


def edge_grid():
    """(m, n, k) of the edge-shape calls.  Pruning rule: of the 144 products keep those whose indices into KS, NS and MS
    satisfy (ik + 2 * in + im) % 3 == 0 - 48 calls in which every pair (K, N), (K, M) and (N, M) still occurs - plus every M
    at the smallest shape (K = 64: two K steps; N = 128: one column tile, so M <= 128 is a grid of ONE tile), and three
    calls whose tile counts straddle the XCD remap's modulus: 7 tiles (M = 895), 8 (M = 1024) and 9 (M = 1025) at N = 128.
    (No product of the three sets has 7 or 8 tiles; 9 = 3 x 3 also occurs inside, at M = 257, N = 384.)"""
    grid = []
    for ik, k in enumerate(KS):
        for i_n, n in enumerate(NS):
            for im, m in enumerate(MS):
                if (ik + 2 * i_n + im) % 3 == 0 or (k == 64 and n == 128):
                    grid.append((m, n, k))
    grid += [(895, 128, 64), (1024, 128, 64), (1025, 128, 128)]
    return grid


def tiles(m, n):
    return ((m + 127) // 128) * (n // 128)
