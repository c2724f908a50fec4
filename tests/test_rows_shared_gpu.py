"""score_rows, topk_rows and truncate_rows read a logits row through one chunk reader, one pair of chunk sums and one fold
(csrc/glb_rowlse.hpp), so on the same inputs their common outputs are the same bits - compared here as int32 patterns, so that
-inf and NaN compare exactly:
  - lse and logZ of score_rows equal those of topk_rows(k=1);
  - with t the top-1 token of a row (where there is one), score_rows(tokens=t) gives the logp and logp_masked of top-k's first
    column;
  - truncate_rows(top_k=1) keeps exactly the keys equal to the row's largest: bit t alone, or the tied set (of which t is the
    lowest index).
Three rows a case; vocab 33 (a partial chunk), 4097 (one element past a chunk boundary) and 8200 (three chunks: every wave but
one is busy); every element type with no mask, bit masks and float masks.  The mask table's four rows: all allowed, nothing
allowed, per chunk only the elements at least 4.0 below the chunk's largest (made for logits row 0, which reads it: the allowed
sum then has a binary scale of its own), and a random third disallowed; one id of every call is out of range (-1 or n_masks):
a row that allows nothing.  The float masks are 0 / -inf: top-k's logp is key - lse(y) with key = y + m, score's is y_t - lse(y),
which are the same number only where m_t = 0.  logit_scale is 1, so a key is the element's value itself."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 4096
N_ROWS = 3
ID_SETS = ((2, 3, -1), (0, 4, 1))  # (mask ids of the three rows; the table has 4 rows)


def _inputs(V, dtype, dev):
    """logits [3, V] on the device (3 N(0, 1), a few -inf), the float32 values they hold, and bool [4, V] allowed."""
    rs = np.random.default_rng(33 * V + 7)
    x = (3 * rs.standard_normal((N_ROWS, V))).astype(np.float32)
    for r in range(N_ROWS):
        x[r, rs.choice(V, size=3, replace=False)] = -np.inf
    x_d = torch.from_numpy(x).to(dev).to(dtype)
    held = x_d.float().cpu().numpy()
    ok = np.ones((4, V), bool)
    ok[1] = False
    for c0 in range(0, V, CHUNK):
        part = held[0, c0:c0 + CHUNK]
        ok[2, c0:c0 + CHUNK] = part <= part.max() - 4.0
    assert ok[2].any()
    ok[3] = rs.random(V) >= 1 / 3
    return x_d, held, ok


def _bit_rows(ok):
    n, V = ok.shape
    words = (V + 31) // 32
    full = np.zeros((n, words * 32), bool)
    full[:, :V] = ok
    return np.packbits(full.reshape(n, words, 32), axis=-1, bitorder="little").view(np.uint32).reshape(n, words).view(np.int32)


def _pattern(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def _check(engine, x_d, held, ok_rows, what, **kw):
    """ok_rows: bool [3, V], what each logits row's mask allows."""
    V = held.shape[1]
    top = engine.topk_rows(x_d, 1, want=("logp", "logp_masked", "lse", "logZ"), **kw)
    t = top["token"][:, 0]
    has = (t >= 0).cpu().numpy()
    sc = engine.score_rows(x_d, torch.where(t >= 0, t, torch.zeros_like(t)), want=("logp", "lse", "logZ", "logp_masked"), **kw)
    for name in ("lse", "logZ"):
        assert np.array_equal(_pattern(sc[name]), _pattern(top[name])), f"{what}: {name}"
    for name in ("logp", "logp_masked"):
        assert np.array_equal(_pattern(sc[name])[has], _pattern(top[name][:, 0])[has]), f"{what}: {name}"
    keys = np.where(ok_rows, held, -np.inf)
    assert np.array_equal(has, np.isfinite(keys.max(axis=1))), f"{what}: rows with a finite key"
    bits = engine.truncate_rows(x_d, top_k=1, **kw)["bits"].cpu().numpy()
    kept = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :V].astype(bool)
    tn = t.cpu().numpy()
    for r in range(N_ROWS):
        tied = (keys[r] == keys[r].max()) & np.isfinite(keys[r])
        assert np.array_equal(kept[r], tied), f"{what}: kept set of row {r}"
        assert tn[r] == (int(np.flatnonzero(tied)[0]) if has[r] else -1), f"{what}: token of row {r}"


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16, torch.float16), ids=str)
@pytest.mark.parametrize("V", (33, 4097, 8200))
def test_score_topk_truncate_share_their_bits(engine, V, dtype):
    dev = engine.device
    x_d, held, ok = _inputs(V, dtype, dev)
    _check(engine, x_d, held, np.ones((N_ROWS, V), bool), f"V={V} {dtype} no mask")
    tables = {1: torch.from_numpy(_bit_rows(ok)).to(dev),
              2: torch.from_numpy(np.where(ok, 0.0, -np.inf).astype(np.float32)).to(dev)}
    for kind, table in tables.items():
        for ids in ID_SETS:
            ok_rows = np.stack([ok[i] if 0 <= i < 4 else np.zeros(V, bool) for i in ids])
            _check(engine, x_d, held, ok_rows, f"V={V} {dtype} mask_kind={kind} ids={ids}", mask_kind=kind, mask=table,
                   row_mask_id=torch.tensor(ids, dtype=torch.int32, device=dev))
