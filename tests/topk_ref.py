"""NumPy reference of glb_topk_rows and glb_beam_select (include/glb.h), written from their contracts:

    y = float32(x * scale) when scale != 1      key = float32(y + m)       (float32 arithmetic: the ids are exact)
    token: a stable sort on (-key, index) after folding -0 into +0; keys of -inf (and NaN) are never selected
    logp = key - lse(y)     logp_masked = key - lse(y + m)     lse = lse(y)     logZ = lse(y + m) - lse(y)

The log-sum-exps are float64 over the widened inputs (tests/score_ref.py's helpers)."""
import numpy as np

from tests.score_ref import lse, mask_values, proposal_values

NEG = -np.inf


def keys_of(x, scale=1.0, m=None):
    """(y float64 [V], key float32 [V]) of one row: x as stored (float32 / float16 / uint16 bfloat16 words), m the additive
    mask values (float64 [V] of float32 values; None: no mask)."""
    y = proposal_values(x, scale)
    y32 = y.astype(np.float32)
    if m is None:
        return y, y32
    with np.errstate(invalid="ignore"):
        key = (y32 + np.asarray(m, np.float64).astype(np.float32)).astype(np.float32)
    return y, np.where(np.isnan(key), np.float32(NEG), key).astype(np.float32)


def select(key, k):
    """Indices of the k largest keys, largest first, equal keys (-0 == +0) by lower index; -inf never; -1 beyond."""
    key = np.asarray(key, np.float32) + np.float32(0.0)  # (-0 + +0 = +0)
    order = np.argsort(-key.astype(np.float64), kind="stable")
    order = order[np.isfinite(key[order]) | (key[order] == np.inf)][:k]
    out = np.full(k, -1, np.int32)
    out[:len(order)] = order
    return out


def topk_row(x, k, scale=1.0, m=None):
    """(token int32 [k], logp float64 [k], logp_masked float64 [k], lse, logZ) of one row."""
    y, key = keys_of(x, scale, m)
    tok = select(key, k)
    ly, lz = lse(y), lse(key.astype(np.float64))
    logp, logpm = np.full(k, NEG), np.full(k, NEG)
    got = tok >= 0
    kk = key[tok[got]].astype(np.float64)
    logp[got] = kk - ly
    logpm[got] = kk - lz
    return tok, logp, logpm, ly, (lz - ly if np.isfinite(lz) else NEG)


def topk_rows(x, k, scale=1.0, kind=0, table=None, row_mask_id=None):
    """dict of token int32 [n, k], logp / logp_masked float64 [n, k], lse / logZ float64 [n].  table: the mask table (kind 1:
    uint32 / int32 bit rows, 2: float rows); row_mask_id None: one mask for all rows if the table has one row, else row r's is
    table[r].  An id out of range: a mask that allows nothing."""
    n, V = x.shape
    out = dict(token=np.empty((n, k), np.int32), logp=np.empty((n, k)), logp_masked=np.empty((n, k)), lse=np.empty(n), logZ=np.empty(n))
    for r in range(n):
        m = None
        if kind:
            mid = int(row_mask_id[r]) if row_mask_id is not None else (0 if len(table) == 1 else r)
            m = mask_values(kind, table[mid], V) if 0 <= mid < len(table) else np.full(V, NEG)
        t = topk_row(x[r], k, scale, m)
        for name, v in zip(("token", "logp", "logp_masked", "lse", "logZ"), t):
            out[name][r] = v
    return out


def beam_select(score, alive, cand_token, cand_logp, width):
    """(parent int32, token int32, score float32), each [G * width]: glb_beam_select's contract, a stable sort on
    (-value, b, j) over each group's candidates."""
    score = np.asarray(score, np.float32)
    alive = np.asarray(alive)
    cand_token, cand_logp = np.asarray(cand_token), np.asarray(cand_logp, np.float32)
    n, k = cand_token.shape
    B = width
    parent, token = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    out = np.full(n, NEG, np.float32)
    for g in range(n // B):
        cands = []  # (value, b, j, token) in (b, j) order
        for b in range(B):
            s = score[g * B + b]
            if not np.isfinite(s):
                continue
            if alive[g * B + b]:
                for j in range(k):
                    with np.errstate(invalid="ignore"):
                        v = np.float32(s + cand_logp[g * B + b, j])
                    if cand_token[g * B + b, j] >= 0 and np.isfinite(v):
                        cands.append((v + np.float32(0.0), b, j, int(cand_token[g * B + b, j])))
            else:
                cands.append((s + np.float32(0.0), b, 0, -1))
        order = sorted(range(len(cands)), key=lambda i: -float(cands[i][0]))[:B]  # (sorted is stable: ties keep (b, j) order)
        for pos, i in enumerate(order):
            parent[g * B + pos], token[g * B + pos], out[g * B + pos] = cands[i][1], cands[i][3], cands[i][0]
    return parent, token, out
