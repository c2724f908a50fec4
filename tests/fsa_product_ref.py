"""The contract of `constraints.product` (include/glb.h glb_fsa_product_round / glb_fsa_live), restated in NumPy:
the queue search over the pairs of states, the normalisation of a pair, accepting, the float32 weight additions, joint
liveness and the trim.  Test infrastructure: the product never imports it.

An operand is `side(automaton)`: (delta, accepting, live, start, arc_logw or None, final_logw or None).
  - A component of a pair is OUT (-1) when it is -1 or not live in its own automaton.  "and": a pair with a side out does
    not exist; "sub": a pair with the a side out; "or": a pair with both sides out.  A start pair that does not exist is
    the pair (-1, -1): one state without arcs that does not accept.
  - State 0 is the start pair; the queue takes the states in id order and the bytes 0 .. 255 in ascending order, and a
    pair gets the next id when it is first met.
  - Accepting: both sides ("and"), either ("or"), a's and not b's ("sub"); a side that is out never accepts.
  - Weights: an arc weighs np.float32(wa + wb) where both sides have weights - ONE rounded addition, a's first - else the
    weight of the side that has them; likewise the final weight, -inf where the state does not accept.  So `path_logw` of the
    result adds, left to right, the arcs' np.float32(wa + wb) and then the final np.float32(fa + fb): that order, not the sum
    of the two operands' path weights.
  - Trim: live[s] = accepting[s] or some arc of s leads to a live state (the least fixed point); the states that are not
    live are dropped, state 0 excepted, the others keep their order; an arc into a dropped state becomes -1 / -inf."""
import numpy as np


def side(automaton):
    return (automaton.delta, automaton.accepting, automaton.live, automaton.start, getattr(automaton, "arc_logw", None),
            getattr(automaton, "final_logw", None))


def _exists(op, a, b):
    return (a >= 0) & (b >= 0) if op == "and" else a >= 0 if op == "sub" else (a >= 0) | (b >= 0)


def _targets(delta, live, s):
    """int64 [256]: where the bytes lead from state s of one operand, normalised (s = -1: nowhere)."""
    if s < 0:
        return np.full(256, -1, np.int64)
    t = delta[s].astype(np.int64)
    return np.where((t >= 0) & live[np.maximum(t, 0)], t, -1)


def search(A, B, op, max_states=None):
    """The untrimmed product: dict(delta int32 [S, 256], accepting bool [S], pairs int32 [S, 2], arc_logw / final_logw float32
    or None).  ValueError as soon as more than `max_states` states are numbered."""
    (da, acca, livea, sa, arca, fina), (db, accb, liveb, sb, arcb, finb) = A, B
    assert op in ("and", "or", "sub") and not (op == "or" and (arca is not None or arcb is not None)) and not (op == "sub" and arcb is not None)
    weighted = arca is not None or arcb is not None
    a0, b0 = (sa if livea[sa] else -1), (sb if liveb[sb] else -1)
    if not _exists(op, np.int64(a0), np.int64(b0)):
        a0 = b0 = -1
    states, index = [(a0, b0)], {(a0, b0): 0}
    rows, arcs, acc, fin = [], [], [], []
    i = 0
    while i < len(states):
        a, b = states[i]
        ta, tb = _targets(da, livea, a), _targets(db, liveb, b)
        ex = _exists(op, ta, tb)
        row = np.full(256, -1, np.int32)
        for byte in np.nonzero(ex)[0]:
            key = (int(ta[byte]), int(tb[byte]))
            if key not in index:
                index[key] = len(states)
                states.append(key)
                if max_states is not None and len(states) > max_states:
                    raise ValueError(f"max_states={max_states} passed")
            row[byte] = index[key]
        rows.append(row)
        fa, fb = a >= 0 and bool(acca[a]), b >= 0 and bool(accb[b])
        ok = (fa and fb) if op == "and" else (fa and not fb) if op == "sub" else (fa or fb)
        acc.append(ok)
        if weighted:
            if arca is not None and arcb is not None:
                w = (arca[a] + arcb[b]).astype(np.float32) if a >= 0 and b >= 0 else np.zeros(256, np.float32)  # float32 + float32: one rounding
                f = np.float32(fina[a] + finb[b]) if ok else np.float32(-np.inf)
            elif arca is not None:
                w = arca[a] if a >= 0 else np.zeros(256, np.float32)
                f = fina[a] if ok else np.float32(-np.inf)
            else:
                w = arcb[b] if b >= 0 else np.zeros(256, np.float32)
                f = finb[b] if ok else np.float32(-np.inf)
            arcs.append(np.where(ex, w, -np.inf).astype(np.float32))
            fin.append(np.float32(f))
        i += 1
    return dict(delta=np.stack(rows), accepting=np.array(acc, np.bool_), pairs=np.array(states, np.int32).reshape(-1, 2),
                arc_logw=np.stack(arcs) if weighted else None, final_logw=np.array(fin, np.float32) if weighted else None)


def liveness(delta, accepting):
    """bool [S]: the least fixed point of live[s] = accepting[s] | any live[delta[s][.]]."""
    live = np.asarray(accepting, np.bool_).copy()
    pres, to = delta >= 0, np.maximum(delta, 0)
    while True:
        nxt = live | (pres & live[to]).any(axis=1)
        if np.array_equal(nxt, live):
            return live
        live = nxt


def trim(p):
    """The product with the states that are not live dropped (state 0 kept); adds `live`, `untrimmed`."""
    live = liveness(p["delta"], p["accepting"])
    keep = live.copy()
    keep[0] = True
    new_id = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    d = p["delta"][keep]
    to = np.where((d >= 0) & keep[np.maximum(d, 0)], new_id[np.maximum(d, 0)], -1).astype(np.int32)
    out = dict(delta=to, accepting=p["accepting"][keep], pairs=p["pairs"][keep], arc_logw=None, final_logw=None, live=live[keep],
               untrimmed=len(live), start=0)
    if p["arc_logw"] is not None:
        out["arc_logw"] = np.where(to >= 0, p["arc_logw"][keep], -np.inf).astype(np.float32)
        out["final_logw"] = p["final_logw"][keep]
    return out


def product(a, b, op, max_states=None):
    """The restated `constraints.product` of two host automata, as a dict (see `trim`)."""
    return trim(search(side(a), side(b), op, max_states))


def accepts(p, data):
    s = 0
    for byte in bytes(data):
        s = int(p["delta"][s, byte])
        if s < 0:
            return False
    return bool(p["accepting"][s])


def path_logw(p, data):
    """float32: the arcs' weights summed left to right, then the final weight; -inf where `data` is not accepted."""
    s, w = 0, np.float32(0.0)
    for byte in bytes(data):
        w = np.float32(w + p["arc_logw"][s, byte])
        s = int(p["delta"][s, byte])
        if s < 0:
            return np.float32(-np.inf)
    return np.float32(w + p["final_logw"][s])
