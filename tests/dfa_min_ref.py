"""The contract of glb_dfa_refine / glb_dfa_quotient (include/glb.h), restated in NumPy: reachability, Moore's
refinement with `np.unique(axis=0)` over the states' signatures, canonical class ids (a class's smallest member), the quotient,
and an isomorphism check by a simultaneous walk from both starts.  Test infrastructure: the product never imports it."""
import numpy as np


def reachable(delta, start):
    """bool [S] by a plain search, one state at a time."""
    delta = np.asarray(delta)
    seen, todo = {int(start)}, [int(start)]
    while todo:
        for v in set(int(x) for x in delta[todo.pop()] if x >= 0):
            if v not in seen:
                seen.add(v)
                todo.append(v)
    out = np.zeros(delta.shape[0], np.bool_)
    out[list(seen)] = True
    return out


def _canonical(labels, keep):
    """int64 [S]: every kept state's class named by its smallest member, -1 elsewhere (labels: any per-state integers)."""
    S = len(labels)
    idx = np.nonzero(keep)[0]
    _, inv = np.unique(labels[idx], return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    smallest = np.full(inv.max() + 1 if len(idx) else 0, S, np.int64)
    np.minimum.at(smallest, inv, idx)
    out = np.full(S, -1, np.int64)
    out[idx] = smallest[inv]
    return out


def present(delta, keep):
    """bool [S, 256]: the arcs that exist and lead to a kept state."""
    delta = np.asarray(delta, np.int64)
    S = delta.shape[0]
    return (delta >= 0) & (delta < S) & keep[np.clip(delta, 0, S - 1)]


def refine(delta, keep, final_bits, arc_bits=None, max_rounds=None):
    """(cls int32 [S], rounds): the coarsest partition of the kept states in which the states of one class have equal
    final_bits, agree on which arcs are present, lead into one class over every present arc and (arc_bits given) carry equal
    bits on the present arcs; -1 where !keep.  `rounds` counts as the device does: every round performed, the one that left
    the number of classes as it was included."""
    delta = np.asarray(delta, np.int64)
    keep = np.asarray(keep, np.bool_)
    S = delta.shape[0]
    pres = present(delta, keep)
    to = np.clip(delta, 0, S - 1)
    bits = np.where(pres, np.asarray(arc_bits).astype(np.int64), 0) if arc_bits is not None else None
    cls = _canonical(np.asarray(final_bits).astype(np.int64), keep)
    count = len(np.unique(cls[keep]))
    rounds = 0
    idx = np.nonzero(keep)[0]
    while max_rounds is None or rounds < max_rounds:
        succ = np.where(pres, cls[to], -1)
        sig = np.concatenate([cls[:, None], succ] + ([bits] if bits is not None else []), axis=1)[idx]
        _, inv = np.unique(sig, axis=0, return_inverse=True)
        labels = np.zeros(S, np.int64)
        labels[idx] = np.asarray(inv).reshape(-1)
        cls = _canonical(labels, keep)
        rounds += 1
        now = len(np.unique(cls[keep]))
        if now == count:
            break
        count = now
    return cls.astype(np.int32), rounds


def new_ids(cls):
    """(new_id int32 [S], rep int32 [S']): quotient states numbered in the order of their classes' smallest members."""
    cls = np.asarray(cls)
    rep = np.unique(cls[cls >= 0]).astype(np.int32)
    return np.where(cls >= 0, np.searchsorted(rep, cls), -1).astype(np.int32), rep


def quotient(delta, keep, new_id, rep, arc_logw=None, final_logw=None, accepting=None):
    """(delta_out, arc_out, final_out, accepting_out) as glb_dfa_quotient writes them (None where the input is None)."""
    delta = np.asarray(delta, np.int64)
    pres = present(delta, np.asarray(keep, np.bool_))[rep]
    to = np.where(pres, new_id[np.clip(delta[rep], 0, delta.shape[0] - 1)], -1).astype(np.int32)
    arc = None if arc_logw is None else np.where(to >= 0, np.asarray(arc_logw, np.float32)[rep], -np.inf).astype(np.float32)
    fin = None if final_logw is None else np.asarray(final_logw, np.float32)[rep]
    acc = None if accepting is None else np.asarray(accepting)[rep]
    return to, arc, fin, acc


def keep_of(delta, accepting, start):
    """live & reachable with the start state kept whatever it is (what the host passes as `keep`)."""
    from tests import dfa_ref

    k = dfa_ref.live(np.asarray(delta, np.int64), np.asarray(accepting, np.bool_)) & reachable(delta, start)
    k[start] = True
    return k


def minimize(delta, accepting, start):
    """(delta', accepting', start', state_map, rounds) of an unweighted automaton."""
    keep = keep_of(delta, accepting, start)
    cls, rounds = refine(delta, keep, np.asarray(accepting).astype(np.int64))
    new_id, rep = new_ids(cls)
    d, _, _, acc = quotient(delta, keep, new_id, rep, accepting=np.asarray(accepting, np.bool_))
    return d, acc, int(new_id[start]), new_id, rounds


def isomorphic(a, b):
    """Whether two (delta, accepting, start) are one automaton up to the names of the states reachable from the starts
    (a simultaneous walk that builds the bijection)."""
    (da, aa, sa), (db, ab, sb) = a, b
    fwd, back, todo = {int(sa): int(sb)}, {int(sb): int(sa)}, [(int(sa), int(sb))]
    while todo:
        u, v = todo.pop()
        if bool(aa[u]) != bool(ab[v]):
            return False
        for x, y in zip(np.asarray(da[u]).tolist(), np.asarray(db[v]).tolist()):
            if (x < 0) != (y < 0):
                return False
            if x < 0:
                continue
            if x in fwd or y in back:
                if fwd.get(x) != y or back.get(y) != x:
                    return False
            else:
                fwd[x], back[y] = y, x
                todo.append((x, y))
    return True


def lexicon_trie(n=1000, seed=1, letters=b"abcd", max_len=8):
    """The strings of the seeded trie: `n` draws of 1 .. max_len letters (duplicates and all)."""
    rng = np.random.default_rng(seed)
    chars = np.frombuffer(letters, np.uint8)
    return [bytes(rng.choice(chars, int(rng.integers(1, max_len + 1)))) for _ in range(n)]


def doubled(delta, accepting, start, extra=10, seed=5):
    """Two disjoint copies of an automaton, some of the start's arcs redirected into the second copy, and `extra` states
    nothing reaches (arcs of their own into both copies): 2 S + extra states with the language of one copy."""
    delta, accepting = np.asarray(delta, np.int32), np.asarray(accepting, np.bool_)
    S = delta.shape[0]
    rng = np.random.default_rng(seed)
    d = np.full((2 * S + extra, 256), -1, np.int32)
    d[:S] = delta
    d[S:2 * S] = np.where(delta >= 0, delta + S, -1)
    swap = (rng.random(256) < 0.5) & (delta[start] >= 0)
    d[start, swap] += S
    d[2 * S:] = rng.integers(0, 2 * S, (extra, 256))
    acc = np.concatenate([accepting, accepting, rng.random(extra) < 0.5])
    return d, acc, start
