"""The contract of `constraints.LazyConstraint` (include/glb.h glb_lazy_*), restated in NumPy.  Test
infrastructure: the package never imports it.

  - A state of the NFA is IMPORTANT when it has a byte arc or accepts; bit i of a set is the i-th important state (`states`).
  - A state is a set of important states closed under empty arcs and ANDed with `useful` - the important states from which
    an accepting state can be reached - W = max(1, ceil(n_important / 64)) uint64 words.  A set is live exactly when it is
    not empty.  Id 0 is the start's closure; the empty set is -1; a state accepts where its set meets `accepting`.
  - `advance` walks tokens[i, frm[i] .. to[i]) byte by byte from states[i]'s set (None: id 0).  A skipped or empty token, a
    token outside the vocabulary, a range outside [0, ld] or a state that was not numbered before the call give -1; frm == to
    gives the state back.  Only the set a particle ends in is numbered.
  - The new sets of a call get consecutive ids in the order of the smallest particle index that reached them; a set that
    finds every id below max_states taken gets none: its particles are -1 and `overflow` is set.
  - Row of a state: bit t where the walk of token t from its set ends not empty; the EOS bit where the state accepts."""
import numpy as np

ONE = np.uint64(1)


def important(nfa):
    imp = np.asarray(nfa.accepting, np.bool_).copy()
    imp[nfa.arc_src] = True
    return imp


def useful(nfa):
    """bool [n_states]: an accepting state can be reached (a backward search from the accepting states, state by state)."""
    back = [[] for _ in range(nfa.n_states)]
    for u, v in zip(nfa.eps_src.tolist(), nfa.eps_dst.tolist()):
        back[v].append(u)
    reads = nfa.arc_set.any(axis=1)
    for k, (u, v) in enumerate(zip(nfa.arc_src.tolist(), nfa.arc_dst.tolist())):
        if reads[k]:
            back[v].append(u)
    out = np.asarray(nfa.accepting, np.bool_).copy()
    todo = np.nonzero(out)[0].tolist()
    while todo:
        for u in back[todo.pop()]:
            if not out[u]:
                out[u] = True
                todo.append(u)
    return out


def pack(bits, W):
    """bool [<= 64 W] -> uint64 [W]."""
    full = np.zeros(64 * W, np.bool_)
    full[:len(bits)] = bits
    return np.packbits(full, bitorder="little").view("<u8").astype(np.uint64)


def members(row):
    return np.nonzero(np.unpackbits(np.ascontiguousarray(row).view(np.uint8), bitorder="little"))[0]


class Ref:
    def __init__(self, nfa, vocab, eos_id, skip_ids=(), max_states=65536):
        self.nfa, self.max_states, self.overflow = nfa, int(max_states), False
        n = nfa.n_states
        imp = important(nfa)
        self.states = np.nonzero(imp)[0].astype(np.int32)
        n_imp = len(self.states)
        self.W = W = max(1, -(-n_imp // 64))
        self.bit_of = np.full(n, -1, np.int64)
        self.bit_of[self.states] = np.arange(n_imp)
        ec = np.zeros((n, W), np.uint64)
        bits = np.arange(n_imp)
        ec[self.states, bits // 64] = ONE << (bits % 64).astype(np.uint64)
        while True:  # the empty-arc closure: a fixed point that only adds
            new = ec.copy()
            np.bitwise_or.at(new, nfa.eps_src, ec[nfa.eps_dst])
            if np.array_equal(new, ec):
                break
            ec = new
        self.useful = pack(useful(nfa)[self.states], W)
        self.eclose = ec & self.useful
        self.accepting_mask = pack(np.asarray(nfa.accepting, np.bool_)[self.states], W)
        self._table, self._steps = {}, {}
        columns = {}
        self._group = np.array([columns.setdefault(nfa.arc_set[:, b].tobytes(), len(columns)) for b in range(256)])
        self._group_byte = {int(g): b for b, g in reversed(list(enumerate(self._group)))}
        start = self.eclose[nfa.start].copy()
        self.order = [start]
        self.ids = {start.tobytes(): 0} if start.any() else {}
        self.vocab = [bytes(t) for t in vocab]
        self.V, self.eos_id = len(self.vocab), int(eos_id)
        self.skip = np.zeros(self.V, np.bool_)
        self.skip[list(skip_ids)] = True

    # ---- sets ----------------------------------------------------------------------------------------------------------
    def _targets(self, group):
        """uint64 [n_important, W]: for every important state the union of the closures behind its arcs that read the bytes
        of `group` (bytes that no arc's set tells apart share one table)."""
        if group not in self._table:
            nfa = self.nfa
            at = np.nonzero(nfa.arc_set[:, self._group_byte[group]])[0]
            t = np.zeros((len(self.states), self.W), np.uint64)
            np.bitwise_or.at(t, self.bit_of[nfa.arc_src[at]], self.eclose[nfa.arc_dst[at]])
            self._table[group] = t
        return self._table[group]

    def step(self, row, byte):
        key = (row.tobytes(), int(self._group[byte]))
        if key not in self._steps:
            m = members(row)
            self._steps[key] = np.bitwise_or.reduce(self._targets(key[1])[m], axis=0) if len(m) else np.zeros(self.W, np.uint64)
        return self._steps[key]

    def token(self, row, t):
        """The set after token t from `row`; empty for a token that is skipped, empty or outside the vocabulary."""
        if t < 0 or t >= self.V or self.skip[t] or not self.vocab[t]:
            return np.zeros(self.W, np.uint64)
        for b in self.vocab[t]:
            row = self.step(row, b)
            if not row.any():
                break
        return row

    n_states = property(lambda self: len(self.order))

    def sets(self):
        return np.stack(self.order).astype(np.uint64).reshape(len(self.order), self.W)

    def accepting(self):
        return (self.sets() & self.accepting_mask).any(axis=1)

    # ---- advance: the numbering rule of one call ---------------------------------------------------------------------------
    def advance(self, states, tokens, frm, to):
        tokens = np.asarray(tokens).reshape(len(frm), -1)
        n, ld = tokens.shape
        known = len(self.order)
        out = np.full(n, -1, np.int32)
        for i in range(n):
            s = 0 if states is None else int(states[i])
            f, t = int(frm[i]), int(to[i])
            if not (0 <= s < known and 0 <= f <= t <= ld):
                continue
            if f == t:
                out[i] = s
                continue
            row = self.order[s]
            for j in range(f, t):
                row = self.token(row, int(tokens[i, j]))
                if not row.any():
                    break
            if not row.any():
                continue
            key = row.tobytes()
            if key not in self.ids:
                if len(self.order) >= self.max_states:
                    self.overflow = True
                    continue
                self.ids[key] = len(self.order)
                self.order.append(row.copy())
            out[i] = self.ids[key]
        return out

    # ---- rows ------------------------------------------------------------------------------------------------------------
    def _pack_row(self, allowed):
        bits = np.zeros((self.V + 31) // 32 * 32, np.uint8)
        bits[:self.V] = allowed
        return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).astype(np.uint32)

    def allowed(self, row, accepts):
        out = np.array([bool(self.token(row, t).any()) for t in range(self.V)], np.bool_)
        if 0 <= self.eos_id < self.V:
            out[self.eos_id] = accepts
        return out

    def mask(self, s):
        """uint32 [ceil(V / 32)]: the bank row of state s."""
        row = self.order[s]
        return self._pack_row(self.allowed(row, bool((row & self.accepting_mask).any())))

    def row_dead(self):
        return self._pack_row(np.zeros(self.V, np.bool_))

    def row_eos(self):
        allowed = np.zeros(self.V, np.bool_)
        allowed[self.eos_id] = True
        return self._pack_row(allowed)
