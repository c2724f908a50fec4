"""NumPy reference of glb_truncate_rows (include/glb.h), written from its contract:

    y = float32(x * scale) when scale != 1      key = float32(y + m), -0 folded into +0     (float32: tests/topk_ref.keys_of)
    tau_k   the top_k-th largest key with multiplicity; -inf when top_k is 0 or the row has no more than top_k finite keys
    tau_m   float32(key_max + float32(log(float32(min_p))))
    tau_p   with w = exp(key - key_max) in float64 and Z_k its sum over key >= tau_k: the largest key t of the row with
            sum over key >= t of w >= top_p * Z_k; top_p = 1: off (-inf)
    keep    {key > -inf and key >= max(tau_k, tau_p, tau_m)}

The device's tau_p is held to the exact answer for some p' within EPS = 1e-4 of top_p (clipped to (0, 1]): `tau_p_lo` and
`tau_p_hi` bound those answers.  `margin` is the distance, in shares of Z_k, from top_p to the nearest cumulative mass on either
side of the boundary token: a row whose margin exceeds the device's mass error has one right answer."""
import numpy as np

from tests.score_ref import mask_values
from tests.topk_ref import keys_of

NEG = -np.inf
EPS = 1e-4


def log_min_p(min_p):
    with np.errstate(divide="ignore"):
        return np.float32(np.log(np.float32(min_p)))


def _nucleus(tvals, C, p):
    """The largest distinct key whose cumulative share reaches p (tvals descending, C their cumulative shares, C[-1] == 1)."""
    return int(min(np.searchsorted(C, p, side="left"), len(C) - 1))


def truncate_row(x, top_k=0, top_p=1.0, min_p=0.0, scale=1.0, m=None):
    """One row: dict of key (float32 [V], -0 folded), keep (bool [V]), tau, tau_k, tau_m, tau_p, tau_p_lo, tau_p_hi, margin, kept,
    logmass (float64).  A row without a finite key: keep all False, tau +inf, logmass -inf."""
    _, key = keys_of(x, scale, m)
    key = (key + np.float32(0.0)).astype(np.float32)
    fin = key > np.float32(NEG)
    V = len(key)
    if not fin.any():
        return dict(key=key, keep=np.zeros(V, bool), tau=np.float32(np.inf), tau_k=np.float32(NEG), tau_m=np.float32(NEG),
                    tau_p=np.float32(NEG), tau_p_lo=np.float32(NEG), tau_p_hi=np.float32(NEG), margin=np.inf, kept=0, logmass=NEG)
    ks = np.sort(key[fin])[::-1]
    kmax = ks[0]
    tau_k = ks[top_k - 1] if 0 < top_k < len(ks) else np.float32(NEG)
    with np.errstate(invalid="ignore"):
        tau_m = np.float32(kmax + log_min_p(min_p))
    tau_p = tau_p_lo = tau_p_hi = np.float32(NEG)
    margin = np.inf
    if top_p < 1.0:
        ksk = ks[ks >= tau_k]
        cum = np.cumsum(np.exp(ksk.astype(np.float64) - float(kmax)))
        last = np.r_[np.nonzero(ksk[1:] != ksk[:-1])[0], len(ksk) - 1]  # the last member of every group of equal keys
        tvals, C = ksk[last], cum[last] / cum[-1]
        i = _nucleus(tvals, C, top_p)
        tau_p = tvals[i]
        margin = float(min(C[i] - top_p, top_p - (C[i - 1] if i else 0.0)))
        tau_p_hi = tvals[_nucleus(tvals, C, max(top_p - EPS, 1e-300))]
        tau_p_lo = tvals[_nucleus(tvals, C, min(top_p + EPS, 1.0))]
    tau = np.float32(max(tau_k, tau_p, tau_m))
    keep = fin & (key >= tau)
    w = np.exp(key[fin].astype(np.float64) - float(kmax))
    logmass = float(np.log(w[keep[fin]].sum() / w.sum()))
    return dict(key=key, keep=keep, tau=tau, tau_k=np.float32(tau_k), tau_m=tau_m, tau_p=np.float32(tau_p), tau_p_lo=np.float32(tau_p_lo),
                tau_p_hi=np.float32(tau_p_hi), margin=margin, kept=int(keep.sum()), logmass=logmass)


def row_mask(kind, table, row_mask_id, r, V):
    """The additive mask values of row r (None without a mask): topk_ref.topk_rows's rules."""
    if not kind:
        return None
    mid = int(row_mask_id[r]) if row_mask_id is not None else (0 if len(table) == 1 else r)
    return mask_values(kind, table[mid], V) if 0 <= mid < len(table) else np.full(V, NEG)


def truncate_rows(x, top_k=0, top_p=1.0, min_p=0.0, scale=1.0, kind=0, table=None, row_mask_id=None):
    """A list of `truncate_row` results, one per row of x."""
    return [truncate_row(x[r], top_k, top_p, min_p, scale, row_mask(kind, table, row_mask_id, r, x.shape[1])) for r in range(len(x))]


def pack_bits(keep):
    """bool [..., V] as uint32 words [..., ceil(V / 32)]: bit j % 32 of word j / 32, pad bits 0."""
    keep = np.asarray(keep, bool)
    V = keep.shape[-1]
    words = (V + 31) // 32
    full = np.zeros(keep.shape[:-1] + (words * 32,), bool)
    full[..., :V] = keep
    return np.packbits(full.reshape(keep.shape[:-1] + (words, 32)), axis=-1, bitorder="little").view(np.uint32).reshape(keep.shape[:-1] + (words,))


def unpack_bits(words):
    """uint32 / int32 words [..., W] as bool [..., 32 W] (all the bits, the pad bits too)."""
    w = np.ascontiguousarray(np.asarray(words)).view(np.uint32)
    return np.unpackbits(w.view(np.uint8).reshape(w.shape + (4,)), axis=-1, bitorder="little").reshape(w.shape[:-1] + (-1,)).astype(bool)
