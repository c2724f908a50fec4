"""The packing plan of the row-packed encoding (kv.packed_plan, the NumPy restatement of what kv.encode_packed computes on
the device): the G prompts once, then every context's tail, in context order."""
import numpy as np
import pytest

from genlm_backend_amd.kv import packed_plan


def _by_hand(prompts, grp, tails):
    """Row by row, from the definition: (segments, positions, tokens, last rows) of the packed batch."""
    rows, g_start = [], []
    for p in prompts:
        g_start.append(len(rows))
        rows += [(j, tok) for j, tok in enumerate(p)]
    seg = [(0, 0, g_start[g], len(p)) for g, p in enumerate(prompts)]
    last = []
    for g, tail in zip(grp, tails):
        P = len(prompts[g])
        seg.append((g_start[g], P, len(rows), len(tail)))
        rows += [(P + i, tok) for i, tok in enumerate(tail)]
        last.append(len(rows) - 1)
    return np.array(seg, np.int32), np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array(last)


CASES = {
    "one prompt, equal tails": ([[5, 6, 7]], [0, 0, 0], [[1, 2], [3, 4], [8, 9]]),
    "one prompt, tails of one": ([list(range(100, 108))], [0, 0], [[1], [2]]),
    "one prompt, one context": ([[9]], [0], [[4]]),
    "one prompt, unequal tails": ([list(range(8))], [0] * 4, [[1], [2, 3, 4], [5, 6], list(range(20, 30))]),
    "three prompts, unequal tails": ([[1, 2, 3], [4], [5, 6, 7, 8, 9]], [2, 0, 1, 1, 0, 2],
                                     [[10], [11, 12], [13], [14, 15, 16], [17], [18, 19, 20, 21]]),
    "three prompts, one unused": ([[1, 2], [3, 4, 5], [6]], [2, 2, 0], [[7, 8], [9], [10]]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_packed_plan(name):
    prompts, grp, tails = CASES[name]
    contexts = [prompts[g] + t for g, t in zip(grp, tails)]
    seg, pos, src, last = packed_plan([len(p) for p in prompts], grp, [len(c) for c in contexts])
    want_seg, want_pos, want_tok, want_last = _by_hand(prompts, grp, tails)
    M = sum(len(p) for p in prompts) + sum(len(t) for t in tails)
    assert seg.dtype == np.int32 and seg.shape == (len(prompts) + len(grp), 4) and pos.shape == (M,) and src.shape == (M, 2)
    assert np.array_equal(seg, want_seg)
    assert np.array_equal(pos, want_pos)
    assert np.array_equal(last, want_last)
    # every row's token, read where the plan says it lies: prompt g (context -1 - g) or context u, at the row's position
    tok = [prompts[-1 - c][o] if c < 0 else contexts[c][o] for c, o in src]
    assert np.array_equal(tok, want_tok)
    # the tails tile [sum P, M) in context order without a gap, and no segment leaves the batch or holds more keys than it has
    t0 = seg[len(prompts):, 2]
    assert t0[0] == sum(len(p) for p in prompts) and np.array_equal(t0[1:], t0[:-1] + seg[len(prompts):-1, 3])
    assert (seg[:, 0] + seg[:, 1] <= M).all() and (seg[:, 2] + seg[:, 3] <= M).all() and (seg >= 0).all()


def test_packed_plan_refuses_a_context_without_tail():
    with pytest.raises(ValueError):
        packed_plan([3], [0, 0], [4, 3])
