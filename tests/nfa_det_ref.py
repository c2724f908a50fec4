"""The contract of `constraints.determinize` (include/glb.h glb_nfa_closure / glb_nfa_subset_round), restated in
plain Python and NumPy.  Test infrastructure: the package never imports it.

  - A state of the NFA is IMPORTANT when it has at least one byte arc or is accepting; bit i of a set is the i-th important
    state in increasing order of their ids (`states`).
  - A state of the result is the set of important states inside the empty-arc closure of what was reached, a bitset of
    W = max(1, ceil(n_important / 64)) uint64 words (bit i: word i // 64, bit i % 64).
  - State 0 is the closure of the start, whatever it is.  The empty set is no other state: an arc into it is -1.
  - A state accepts where its set holds an accepting state.
  - A queue takes the states in id order and the bytes 0 .. 255 in ascending order; a set gets the next id when it is first
    met.  (Bytes that no arc tells apart lead to one set: taking each group of them once, the groups in the order of their
    lowest bytes, meets the sets in the same order.)
  - live[s]: some accepting state is reachable from s.  Nothing is trimmed or merged."""
import numpy as np


def important(nfa):
    imp = np.asarray(nfa.accepting, np.bool_).copy()
    imp[nfa.arc_src] = True
    return imp


def determinize(nfa, max_states=None):
    """dict(delta int32 [S, 256], accepting bool [S], sets uint64 [S, W], states int32 [n_important], live bool [S], start 0).
    ValueError as soon as more than `max_states` states are numbered."""
    n = nfa.n_states
    imp = important(nfa)
    states = np.nonzero(imp)[0].astype(np.int32)
    bit_of = {int(v): i for i, v in enumerate(states)}
    W = max(1, -(-len(states) // 64))
    eps = [[] for _ in range(n)]
    for u, v in zip(nfa.eps_src.tolist(), nfa.eps_dst.tolist()):
        eps[u].append(v)
    memo = {}

    def closure(v):
        """The important states behind empty arcs from v, v included, as an int of bits."""
        if v not in memo:
            seen, todo, bits = {v}, [v], 0
            while todo:
                u = todo.pop()
                if u in bit_of:
                    bits |= 1 << bit_of[u]
                for t in eps[u]:
                    if t not in seen:
                        seen.add(t)
                        todo.append(t)
            memo[v] = bits
        return memo[v]

    # the byte groups, in the order of their lowest bytes
    columns = {}
    for b in range(256):
        columns.setdefault(nfa.arc_set[:, b].tobytes(), []).append(b)
    groups = sorted(columns.values())
    # arcs of every important state: (the groups it reads, the closure of its target)
    arcs = [[] for _ in states]
    for a, (u, v) in enumerate(zip(nfa.arc_src.tolist(), nfa.arc_dst.tolist())):
        reads = [g for g, members in enumerate(groups) if nfa.arc_set[a, members[0]]]
        if reads:
            arcs[bit_of[u]].append((reads, closure(v)))
    accepting_bits = sum(1 << i for i, v in enumerate(states) if nfa.accepting[v])
    order, ids, rows = [closure(nfa.start)], {closure(nfa.start): 0}, []
    k = 0
    while k < len(order):
        cur, k = order[k], k + 1
        nxt = [0] * len(groups)
        while cur:
            low = cur & -cur
            cur ^= low
            for reads, target in arcs[low.bit_length() - 1]:
                for g in reads:
                    nxt[g] |= target
        row = np.full(256, -1, np.int32)
        for members, t in zip(groups, nxt):
            if not t:
                continue
            if t not in ids:
                ids[t] = len(order)
                order.append(t)
                if max_states is not None and len(order) > max_states:
                    raise ValueError(f"max_states={max_states} passed")
            row[members] = ids[t]
        rows.append(row)
    delta = np.stack(rows)
    accepting = np.array([bool(t & accepting_bits) for t in order], np.bool_)
    sets = np.array([[(t >> (64 * w)) & 0xffffffffffffffff for w in range(W)] for t in order], np.uint64).reshape(len(order), W)
    return dict(delta=delta, accepting=accepting, sets=sets, states=states, live=liveness(delta, accepting), start=0)


def liveness(delta, accepting):
    """bool [S]: the least fixed point of live[s] = accepting[s] | any live[delta[s][.]]."""
    live = np.asarray(accepting, np.bool_).copy()
    pres, to = delta >= 0, np.maximum(delta, 0)
    while True:
        nxt = live | (pres & live[to]).any(axis=1)
        if np.array_equal(nxt, live):
            return live
        live = nxt


def renumber(delta, accepting, start):
    """(delta, accepting, old): the part of a deterministic automaton that `start` reaches, its states numbered by a queue
    search in byte order (state 0 the start), and every new state's old id."""
    old, new = [int(start)], {int(start): 0}
    k = 0
    while k < len(old):
        for t in delta[old[k]].tolist():
            if t >= 0 and t not in new:
                new[t] = len(old)
                old.append(t)
        k += 1
    old = np.asarray(old, np.int64)
    to = np.full(len(delta), -1, np.int32)
    to[old] = np.arange(len(old), dtype=np.int32)
    d = delta[old]
    return np.where(d >= 0, to[np.maximum(d, 0)], -1).astype(np.int32), np.asarray(accepting, np.bool_)[old], old.astype(np.int32)


def accepts(p, data):
    s = 0
    for byte in bytes(data):
        s = int(p["delta"][s, byte])
        if s < 0:
            return False
    return bool(p["accepting"][s])
