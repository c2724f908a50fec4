"""float64 reference of glb_score_rows (include/glb.h), written from its formulas:

    y = float32(x * scale) when scale != 1      lse = lse(y)      logp = y_t - lse(y)
    logZ = lse(y + m) - lse(y)                  logp_masked = y_t + m_t - lse(y + m)

Inputs are the exact values of their element type, widened to float64 before anything is added (tests/importance_ref.py:
`widen`, `proposal_values`, `mask_values`, `lse`).  Sequence sums are exact sums (math.fsum) rounded to float32 once."""
import math

import numpy as np

from tests.importance_ref import bf16_bits, lse, mask_values, proposal_values, widen  # noqa: F401 (re-exported)

NEG = -np.inf


def score_row(x, t, scale=1.0, m=None):
    """(logp, lse, logZ, logp_masked) of one row: x the logits as stored (float32 / float16 / uint16 bfloat16 words), t
    the token, m the additive mask values (float64 [V]; None: no mask)."""
    y = proposal_values(x, scale)
    V = len(y)
    m = np.zeros(V) if m is None else np.asarray(m, np.float64)
    with np.errstate(invalid="ignore"):
        z = y + m
    z = np.where(np.isnan(z), NEG, z)
    ly, lz = lse(y), lse(z)
    ok = 0 <= t < V
    logp = y[t] - ly if ok and np.isfinite(y[t]) and np.isfinite(ly) else NEG
    logZ = lz - ly if np.isfinite(lz) else NEG
    logpm = z[t] - lz if ok and np.isfinite(z[t]) and np.isfinite(lz) else NEG
    return logp, ly, logZ, logpm


def score_rows(x, tokens, scale=1.0, kind=0, table=None, row_mask_id=None):
    """float64 [n_rows, 4] in the order (logp, lse, logZ, logp_masked).  table: the mask table (kind 1: uint32 / int32 bit
    rows, 2: float rows); row_mask_id None: one mask for all rows if the table has one row, else row r's is table[r].  An id
    out of range: a mask that allows nothing."""
    n, V = x.shape
    out = np.empty((n, 4))
    for r in range(n):
        m = None
        if kind:
            mid = int(row_mask_id[r]) if row_mask_id is not None else (0 if len(table) == 1 else r)
            m = mask_values(kind, table[mid], V) if 0 <= mid < len(table) else np.full(V, NEG)
        out[r] = score_row(x[r], int(tokens[r]), scale, m)
    return out


def seq_sums(values, seq_start):
    """float32 [n_seq]: the exact sum of each sequence's values (float32), rounded once; -inf if any term is; 0 if none."""
    out = np.zeros(len(seq_start) - 1, np.float32)
    for s in range(len(out)):
        v = [float(a) for a in values[seq_start[s]:seq_start[s + 1]]]
        out[s] = NEG if any(a == NEG for a in v) else np.float32(math.fsum(v))
    return out
