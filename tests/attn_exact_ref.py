"""Exact-answer inputs for the attention kernels (the wave kernels of glb_kv.hip, the MFMA tile kernels of glb_attn_tile.hip,
glb_attn_batch.hip and glb_attn_packed_tile.hip), made and answered on the CPU.  tests/test_attn_exact_cpu.py pins what the
generators promise; tests/test_attn_exact_gpu.py runs the kernels on them.

Every operand is a small integer or a power of two - exact in float32, bfloat16 and float16 - and the kernels run with
scale = 1.0, so every score is an exact integer in float32.  Three families:

  selector   two dims (e0, e1) of a head carry a key's rank: K[s][e0] = rank & 255, K[s][e1] = rank >> 8, every query holds
             Q[e0] = B = 128 and Q[e1] = 256 B.  Scores are B * rank: the runner-up is at least 128 below the winner,
             exp(-128) = 2.6e-56 is far below float32's smallest denormal (1.4e-45), so p is exactly 1 for the visible key of
             largest rank and exactly 0 for every other: l == 1 and the output IS V[winner], bit for bit.  (e0, e1) move with
             (row, KV head) through every 16-byte vector of a head row.  The other dims hold noise from {+-1, +-2, +-3} in K
             with Q zero there (noise "k") or in Q with K zero there (noise "q"): exactly 0 in every score unless a kernel
             mixes dims, heads or rows.  Ranks: "last" (rank = position: any key seen past a causal or mask boundary wins
             instead), "first" (the first visible key wins: the earlier tile's o must survive every later tile untouched),
             "perm" (a seeded permutation: winners mid-tile, the running maximum rises and falls across tiles).
  uniform    Q = 0: every score is 0, every visible p exactly 1 (also as a 16-bit MFMA operand), l the number of visible keys
             and the sums of V exact integers.  The output is the mean of V over the visible keys up to the rounding of 1 / l,
             one multiply and the final conversion: |out - mean| <= |mean| (2^-21 + u), u the unit roundoff of the output
             type (pack16v converts with a C cast: round to nearest, so u and not 2 u).
  poison     what a query must not see.  Slab kernels: NaN in every slab position >= pos and every k_new / v_new position
             t >= n_new - neither is ever read.  Batch and packed kernels multiply hidden keys by p = 0, so their poison is
             finite: a key hidden from every query of its row (a packed row no segment names) has the top rank 511 and
             V = 255 everywhere - seen once, it wins the selector and shifts the mean by ~255 / n.

A case is built once in float32 (`lru_cache`) and shared by the dtypes and kernels that run it; nothing mutates it.
"""
import functools
from types import SimpleNamespace as NS

import numpy as np
import torch

B = 128                # a rank step in score units: exp(-B) underflows float32
POISON_RANK = 511      # 255 + 256: still two 8-bit digits
POISON_V = 255.0
CANARY = 12345.0
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
UNIT_ROUNDOFF = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
KT = 32                # keys of a tile of the MFMA kernels (glb_attn_mfma.hpp)

HEADS = ((4, 2), (3, 3))           # (H, Hkv)
TILE_DIMS, WAVE_DIMS = (64, 128), (16, 32, 64, 128)  # the head sizes the MFMA tile kernels / the wave kernels are built for
TILE_T, CHUNK_T = (17, 33, 64, 128), (1, 5, 16)      # new tokens a row: slab_attention_tile / slab_attention_chunk (1: slab_attention too)
ROWS_SHAPES = ((7, 16), (13, 32))  # (Lq, Lk) of short_attention's form for up to 16 / 32 keys, on top of BATCH_SHAPES

# (family, rank variant, noise) of every launch of a case
FAMILIES = (("selector", "last", "k"), ("selector", "first", "q"), ("selector", "perm", "k"), ("selector", "perm", "q"),
            ("uniform", "last", "k"))


def uniform_bound(mean, dtype):
    """|out - mean| may be at most this (float64 tensor like `mean`)."""
    return mean.abs() * (2.0 ** -21 + UNIT_ROUNDOFF[dtype])


def rank_dims(salt, r, hk, Hkv, Dh):
    """The two dims of (row r, KV head hk) that carry the rank."""
    e0 = (17 * ((salt + r) * Hkv + hk) + 5) % Dh
    return e0, (e0 + 7) % Dh


def ranks(variant, position, seed):
    """position: int array, a key's place in its context, -1 for poison.  Distinct places get distinct ranks."""
    P = int(position.max()) + 1
    assert 1 <= P < POISON_RANK
    at = np.maximum(position, 0)
    if variant == "last":
        rank = at.copy()
    elif variant == "first":
        rank = P - 1 - at
    else:
        rank = np.random.default_rng(seed).permutation(P)[at]
    rank[position < 0] = POISON_RANK
    return rank.astype(np.int64)


def fill(family, variant, noise, salt, seed, H, Hkv, Dh, position, Lq):
    """float32 torch tensors q [R, H, Lq, Dh], k / v [R, Hkv, L, Dh] and rank [R, L] for keys at `position` [R, L]."""
    rng = np.random.default_rng(seed)
    R, L = position.shape
    G = H // Hkv
    rank = ranks(variant, position, seed + 1)
    vals = np.array([-3, -2, -1, 1, 2, 3], np.float32)
    k, q = np.zeros((R, Hkv, L, Dh), np.float32), np.zeros((R, H, Lq, Dh), np.float32)
    if noise == "k":
        k = rng.choice(vals, size=k.shape)
    else:
        q = rng.choice(vals, size=q.shape)
    for r in range(R):
        for hk in range(Hkv):
            e0, e1 = rank_dims(salt, r, hk, Hkv, Dh)
            k[r, hk, :, e0], k[r, hk, :, e1] = rank[r] & 255, rank[r] >> 8
            q[r, hk * G:(hk + 1) * G, :, e0], q[r, hk * G:(hk + 1) * G, :, e1] = B, 256 * B
    if family == "uniform":
        q[:] = 0.0
    v = (rng.integers(1, 32, size=k.shape) * rng.choice([-1, 1], size=k.shape)).astype(np.float32)
    v[np.broadcast_to((position < 0)[:, None, :], v.shape[:3])] = POISON_V
    return torch.from_numpy(q), torch.from_numpy(k), torch.from_numpy(v), torch.from_numpy(rank)


# ---- the flat form every signature reduces to: q [R, H, Lq, Dh], k / v [R, Hkv, L, Dh], see [R, Lq, L], valid [R, Lq] -------
def attention_f64(flat):
    """Plain attention in float64: (out [R, Lq, H, Dh], scores [R, H, Lq, L]); a query that sees nothing gives zeros."""
    G = flat.q.shape[1] // flat.k.shape[1]
    kf, vf = (x.double().nan_to_num(0.0).repeat_interleave(G, dim=1) for x in (flat.k, flat.v))  # (NaN is never visible)
    sc = torch.einsum("rhtd,rhsd->rhts", flat.q.double(), kf)
    w = torch.softmax(sc.masked_fill(~flat.see[:, None], float("-inf")), -1).nan_to_num(0.0)
    return torch.einsum("rhts,rhsd->rthd", w, vf), sc


def expected_flat(flat):
    """The answer from the construction alone, float64 [R, Lq, H, Dh]: V of the visible key of largest rank / the mean of V
    over the visible keys; zeros for a query that sees nothing."""
    G = flat.q.shape[1] // flat.k.shape[1]
    vf = flat.v.double().nan_to_num(0.0).repeat_interleave(G, dim=1)  # [R, H, L, Dh]
    seen = flat.see.any(-1)
    if flat.family == "selector":
        win = torch.where(flat.see, flat.rank[:, None, :], torch.full((), -1, dtype=torch.int64)).argmax(-1)  # [R, Lq]
        R, H, _, Dh = vf.shape
        out = torch.gather(vf, 2, win[:, None, :, None].expand(R, H, win.shape[1], Dh)).transpose(1, 2)
    else:
        count = flat.see.sum(-1).clamp(min=1).double()  # (the sum is an exact integer: a sum of 0 gives a mean of exactly 0)
        out = torch.einsum("rts,rhsd->rthd", flat.see.double(), vf) / count[:, :, None, None]
    return out * seen[:, :, None, None]


def round_to(x, dtype):
    return x.to(dtype).float()


def compare(out, expected, family, dtype, where=None):
    """`out` (tensor of `dtype`) against `expected` (float64) at the elements `where` (bool over the leading dims; None: all):
    (ok, largest |out - mean| / |mean|, its bound).  Selector: the same bits, no tolerance.  Uniform: `uniform_bound` alone."""
    if where is not None:
        out, expected = out[where], expected[where]
    if family == "selector":
        return torch.equal(out, expected.to(dtype)), 0.0, 0.0
    err, bound = (out.double() - expected).abs(), uniform_bound(expected, dtype)
    nz = expected != 0
    rel = (err[nz] / expected[nz].abs()).max().item() if nz.any() else 0.0
    return bool((err <= bound).all()), rel, 2.0 ** -21 + UNIT_ROUNDOFF[dtype]


def emulate_tiles(flat, dtype, swap_v=None, see_one_more=False, rescale=True):
    """The kernels' online softmax over tiles of KT keys in float32 (m2 = max(m, tm), c = exp(m - m2), l = l c + ps,
    o = o c + P V with P rounded to `dtype`; a maximum still at -inf takes its exponentials against 0), the output rounded to
    `dtype`: float32 [R, Lq, H, Dh].  The three keywords break it on purpose: swap_v = (a, b) exchanges two key slots of every
    tile's V operand, see_one_more shows every query the key behind each key it sees (`> lim + 1` for `> lim`),
    rescale = False drops o *= c."""
    q, k, v = (round_to(x.nan_to_num(0.0), dtype) for x in (flat.q, flat.k, flat.v))
    R, H, Lq, Dh = q.shape
    G, L = H // k.shape[1], k.shape[2]
    k, v = k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1)
    see = flat.see.clone()
    if see_one_more:
        see[:, :, 1:] |= flat.see[:, :, :-1]
    ninf = torch.tensor(float("-inf"))
    m, l = torch.full((R, H, Lq), float("-inf")), torch.zeros((R, H, Lq))
    o = torch.zeros((R, H, Lq, Dh))
    for t0 in range(0, L, KT):
        kt, vt, st = k[:, :, t0:t0 + KT], v[:, :, t0:t0 + KT], see[:, None, :, t0:t0 + KT]
        if swap_v is not None and max(swap_v) < vt.shape[2]:
            order = list(range(vt.shape[2]))
            order[swap_v[0]], order[swap_v[1]] = swap_v[1], swap_v[0]
            vt = vt[:, :, order]
        s = torch.where(st, torch.einsum("rhtd,rhsd->rhts", q, kt), ninf)
        m2 = torch.maximum(m, s.amax(-1))
        mref = torch.where(torch.isinf(m2), torch.zeros(()), m2)
        c, p = torch.exp(m - mref), torch.exp(s - mref[..., None])
        l = l * c + p.sum(-1)
        if rescale:
            o = o * c[..., None]
        o = o + torch.einsum("rhts,rhsd->rhtd", round_to(p, dtype), vt)
        m = m2
    inv = torch.where(l > 0, 1.0 / l, torch.zeros(()))
    return round_to(o * inv[..., None], dtype).transpose(1, 2)


# ---- slab signature: slab_attention_tile, slab_attention_chunk, slab_attention --------------------------------------------------
CAP = 160


def slab_rows(T, cap=CAP):
    """(pos, n_new) of every row: the first new key on, before and after a tile boundary; pos + n_new == cap; one token
    inside a wide forward."""
    half = max(1, T // 2)
    rows = [(0, T), (31, 1), (32, half)] + ([(33, T)] if 33 + T <= cap else []) + [(cap - T, T), (45, 1)]
    return np.asarray(rows, np.int32)


@functools.lru_cache(maxsize=512)
def slab_case(family, variant, noise, T, H, Hkv, Dh, cap=CAP):
    """flat: the rows AFTER the append (keys 0 .. pos + n_new - 1, NaN behind them).  k_slab / v_slab: the slab before the
    call, NaN at every position >= pos; k_new / v_new [R, Hkv, T, Dh]: NaN at t >= n_new; k_after / v_after: the slab the call
    must leave; expected [R, T, H, Dh] float64, zeros at padded queries."""
    rows = slab_rows(T, cap)
    R = len(rows)
    pos, nn = rows[:, 0].astype(np.int64), rows[:, 1].astype(np.int64)
    s, t = np.arange(cap)[None, :], np.arange(T)[None, :]
    held = s < (pos + nn)[:, None]  # [R, cap]
    position = np.where(held, s, -1)
    q, k, v, rank = fill(family, variant, noise, T, 1000 * T + 10 * H + Dh, H, Hkv, Dh, position, T)
    nan = torch.tensor(float("nan"))
    held_t = torch.from_numpy(held)[:, None, :, None]
    k_after, v_after = torch.where(held_t, k, nan), torch.where(held_t, v, nan)
    old = torch.from_numpy(s < pos[:, None])[:, None, :, None]
    k_slab, v_slab = torch.where(old, k, nan), torch.where(old, v, nan)
    idx = torch.from_numpy(np.minimum(pos[:, None] + t, cap - 1))  # [R, T]
    gat = idx[:, None, :, None].expand(R, Hkv, T, Dh)
    fresh = torch.from_numpy(t < nn[:, None])[:, None, :, None]
    k_new, v_new = torch.where(fresh, torch.gather(k, 2, gat), nan), torch.where(fresh, torch.gather(v, 2, gat), nan)
    valid = torch.from_numpy(t < nn[:, None])
    see = torch.from_numpy(s[:, None, :] <= (pos[:, None] + t)[:, :, None]) & valid[:, :, None]
    flat = NS(family=family, q=q, k=k_after, v=v_after, rank=rank, see=see, valid=valid, blind=torch.zeros_like(valid))
    return NS(flat=flat, q=q, k_new=k_new, v_new=v_new, k_slab=k_slab, v_slab=v_slab, k_after=k_after, v_after=v_after,
              pos=torch.from_numpy(rows[:, 0].copy()), n_new=torch.from_numpy(rows[:, 1].copy()), valid=valid,
              expected=expected_flat(flat))


# ---- batch signature: batch_attention_tile, short_attention ------------------------------------------------------------------------
U = 4
BATCH_SHAPES = ((1, 70), (65, 65), (33, 160), (96, 257))
MASKS = ("null", "right", "left", "hole", "random", "broadcast")


def batch_mask(name, Lq, Lk, seed):
    """(see bool [U, Lq, Lk], blind bool [U, Lq]: the queries MEANT to see nothing, from the construction)."""
    P = Lk - Lq
    s, t = np.arange(Lk)[None, None, :], np.arange(Lq)[None, :, None]
    causal = np.broadcast_to(s <= t + P, (U, Lq, Lk))
    col = lambda lens: np.asarray(lens)[:, None, None]
    n_tok, n_pre = col([Lq, max(1, Lq // 2), max(1, Lq - 5), 1]), col([P, P // 2, 0, max(0, P - 3)])
    blind = np.zeros((U, Lq), bool)
    if name in ("null", "broadcast"):
        see = causal & (s != 3) if name == "broadcast" else causal  # (key 0 stays: every query sees something)
    elif name == "right":
        see, blind = causal & (s < P + n_tok) & (t < n_tok), np.broadcast_to(t[..., 0] >= n_tok[..., 0], (U, Lq))
    elif name == "left":
        see, blind = causal & (s >= P + Lq - n_tok) & (t >= Lq - n_tok), np.broadcast_to(t[..., 0] < Lq - n_tok[..., 0], (U, Lq))
    elif name == "hole":
        see = causal & ((s < n_pre) | ((s >= P) & (s < P + n_tok))) & (t < n_tok)
        blind = np.broadcast_to(t[..., 0] >= n_tok[..., 0], (U, Lq))
    else:
        see = np.random.default_rng(seed).random((U, Lq, Lk)) < 0.6
        see[0, Lq // 3] = False
        see[0, Lq // 3, Lk - 1] = True  # its only key is the last one: m stays -inf through every earlier tile
        see[1, Lq // 2] = False  # a query that sees nothing
        see[2, :64, min(64, Lk - 1):128] = False  # a 64-key stretch hidden from every query of the first block
        see[3, :, :min(40, Lk // 2)] = False  # the first tiles hidden from every query of a row (40 keys at the tile kernels' shapes)
        blind = np.zeros((U, Lq), bool)
        blind[1, Lq // 2] = True
    return torch.from_numpy(np.array(see)), torch.from_numpy(np.array(blind))  # (copies: the broadcasts are read-only)


@functools.lru_cache(maxsize=512)
def batch_case(family, variant, noise, mask, Lq, Lk, H, Hkv, Dh):
    """q [U, H, Lq, Dh], k / v [U, Hkv, Lk, Dh]; mask: None (causal) or bool [U or 1, 1, Lq, Lk] - "broadcast" is one row for
    all U; expected [U, Lq, H, Dh] float64.  A key no query of its row sees is poison."""
    see, blind = batch_mask(mask, Lq, Lk, Lq + Lk)
    position = np.where(see.any(1).numpy(), np.arange(Lk)[None, :], -1)
    q, k, v, rank = fill(family, variant, noise, Lq, 1000 * Lk + 10 * H + Dh + MASKS.index(mask), H, Hkv, Dh, position, Lq)
    flat = NS(family=family, q=q, k=k, v=v, rank=rank, see=see, valid=torch.ones((U, Lq), dtype=torch.bool), blind=blind)
    m_arg = None if mask == "null" else (see[:1] if mask == "broadcast" else see)[:, None].contiguous()
    return NS(flat=flat, q=q, k=k, v=v, mask=m_arg, blind=blind, expected=expected_flat(flat))


# ---- packed signature: packed_row_map + packed_attention_tile, short_attention_packed -------------------------------------------
def plan(prompts, tails, gap=0, reverse=False):
    """(segments int32 [S, 4] = (pre_start, pre_len, tail_start, tail_len), M): the prompts' rows, `gap` rows nobody names,
    then the tails (group, length) in order - tests/test_attn_packed_tile_gpu.py's `_plan`."""
    starts = np.concatenate([[0], np.cumsum(prompts)]).astype(int)
    seg, at = [(0, 0, int(starts[g]), n) for g, n in enumerate(prompts)], int(starts[-1]) + gap
    for g, t in tails:
        seg.append((int(starts[g]), prompts[g], at, t))
        at += t
    return np.asarray(seg[::-1] if reverse else seg, np.int32), at


_MIXED = ([40, 70], [(i % 2, 3) for i in range(9)])
_MIXED_SHORT = ([10, 20], [(i % 2, 3) for i in range(9)])
PLANS = {"mixed": plan(*_MIXED), "ragged": plan([33], [(0, 1), (0, 17), (0, 64), (0, 65)]),
         "long-prompt": plan([130], [(0, 5), (0, 5)]), "alone": plan([1, 31, 32, 33, 97], []),
         "gap": plan(*_MIXED, gap=5, reverse=True)}
# the same forms within short_attention_packed's 32 keys a context: both of its key counts (<= 16 in registers, <= 32 in LDS)
SHORT_PLANS = {"mixed": plan(*_MIXED_SHORT), "ragged": plan([9], [(0, 1), (0, 7), (0, 23)]), "long-prompt": plan([27], [(0, 5), (0, 5)]),
               "alone": plan([1, 15, 16, 17, 31, 32], []), "gap": plan(*_MIXED_SHORT, gap=5, reverse=True),
               "few-keys": plan([4, 9], [(i % 2, 3) for i in range(5)])}


@functools.lru_cache(maxsize=512)
def packed_case(family, variant, noise, plan_name, H, Hkv, Dh, short=False):
    """q [M, H, Dh], k / v [M, Hkv, Dh], seg int32 [S, 4], max_keys; expected [M, H, Dh] float64 with CANARY in the rows no
    segment names, named bool [M].  A key's rank goes by its place in its context: the prompt's keys, then the context's own
    tail - a sibling's tail, the other prompt and one's own future token all hold ranks a query must not meet.  flat: one row
    per segment, its keys gathered in context order."""
    seg, M = (SHORT_PLANS if short else PLANS)[plan_name]
    position = np.full((1, M), -1)
    for a, n, b, t in seg.tolist():
        position[0, b:b + t] = n + np.arange(t)
    salt = list(PLANS).index(plan_name) if plan_name in PLANS else len(PLANS)
    q, k, v, rank = fill(family, variant, noise, salt, 1000 * M + 10 * H + Dh, H, Hkv, Dh, position, M)
    q, k, v, rank = q[0].transpose(0, 1).contiguous(), k[0].transpose(0, 1).contiguous(), v[0].transpose(0, 1).contiguous(), rank[0]
    S, L, Lq = len(seg), int((seg[:, 1] + seg[:, 3]).max()), int(seg[:, 3].max())
    key_row, q_row = np.zeros((S, L), np.int64), np.zeros((S, Lq), np.int64)
    valid, see = np.zeros((S, Lq), bool), np.zeros((S, Lq, L), bool)
    for i, (a, n, b, t) in enumerate(seg.tolist()):
        key_row[i, :n + t] = list(range(a, a + n)) + list(range(b, b + t))
        q_row[i, :t], valid[i, :t] = np.arange(b, b + t), True
        see[i, :t] = np.arange(L)[None, :] <= n + np.arange(t)[:, None]
    key_row, q_row = torch.from_numpy(key_row), torch.from_numpy(q_row)
    flat = NS(family=family, q=q[q_row].permute(0, 2, 1, 3), k=k[key_row].permute(0, 2, 1, 3), v=v[key_row].permute(0, 2, 1, 3),
              rank=rank[key_row], see=torch.from_numpy(see), valid=torch.from_numpy(valid), blind=torch.zeros((S, Lq), dtype=torch.bool))
    expected = torch.full((M, H, Dh), CANARY, dtype=torch.float64)
    expected[q_row[flat.valid]] = expected_flat(flat)[flat.valid]
    named = torch.zeros(M, dtype=torch.bool)
    named[q_row[flat.valid]] = True
    return NS(flat=flat, q=q, k=k, v=v, seg=seg, M=M, max_keys=L, named=named, expected=expected, q_row=q_row)


def packed_flat_expected(case):
    """`case.expected` in the layout of `case.flat`: [S, Lq, H, Dh], zeros at the queries a segment does not have."""
    return case.expected[case.q_row] * case.flat.valid[:, :, None, None]
