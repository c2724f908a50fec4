"""The contract of `constraints.ConstraintProduct` (include/glb.h glb_conj_*), restated in NumPy and plain Python
on top of the parts' own restatements (tests/dfa_ref.py, wfsa_ref.py, lazy_ref.py, pda_ref.py): the tuple of part states, its
numbering within and across calls, the overflow cut, the packed words, and the row of a tuple - the AND of bit rows, or the
ordered float32 sum of the weighted parts' rows with -inf under a cleared bit.  Test infrastructure: the product never
imports it.

A part is an object with `start`, `weighted`, `start_logw`, `advance(states, tokens, frm, to)` (int32 [n]; `states` an array,
never None) and `row(s)` - uint32 [ceil(V / 32)], or float32 [V] when weighted.  `Product` is one itself: products nest."""
import numpy as np

from tests import dfa_ref as R
from tests import wfsa_ref as WR

NINF = np.float32(-np.inf)


class DfaPart:
    """A `ByteDFA` (or, weighted, a `ByteWFSA`) as `DeviceConstraint` serves it without push or minimisation."""

    def __init__(self, dfa, vocab, eos_id, skip_ids=()):
        self.weighted = hasattr(dfa, "arc_logw")
        if self.weighted:
            self.ref = WR.WRef(dfa.delta, dfa.arc_logw, dfa.final_logw, dfa.start, vocab, eos_id, skip_ids)
        else:
            self.ref = R.Ref(dfa.delta, dfa.accepting, dfa.start, vocab, eos_id, skip_ids)
        self.start, self.start_logw, self.S = int(dfa.start), 0.0, len(self.ref.delta)
        self._rows = {}

    def advance(self, states, tokens, frm, to):
        tokens = np.asarray(tokens).reshape(len(frm), -1)
        ld = tokens.shape[1]
        out = np.full(len(frm), -1, np.int32)
        for i, s in enumerate(states):
            f, t = int(frm[i]), int(to[i])
            if 0 <= s < self.S and 0 <= f <= t <= ld:
                out[i] = self.ref.advance(int(s), tokens[i, f:t])
        return out

    def row(self, s):
        if s not in self._rows:
            self._rows[s] = self.ref.row(s) if self.weighted else self.ref.mask(s)
        return self._rows[s]

    def final_logw(self, s):
        return self.ref.final[s]


class NumberedPart:
    """A `lazy_ref.Ref` or `pda_ref.Ref`: a restatement that numbers its own states, start 0, bit rows."""

    weighted, start, start_logw = False, 0, 0.0

    def __init__(self, ref):
        self.ref, self._rows = ref, {}

    def advance(self, states, tokens, frm, to):
        return self.ref.advance(np.asarray(states, np.int32), tokens, frm, to)

    def row(self, s):
        if s not in self._rows:
            self._rows[s] = self.ref.mask(s)
        return self._rows[s]


def bits_of(words, V):
    return np.unpackbits(np.ascontiguousarray(words, "<u4").view(np.uint8), bitorder="little")[:V].astype(np.bool_)


class Product:
    def __init__(self, parts, V, eos_id, max_states=65536):
        assert 2 <= len(parts) <= 8
        self.parts, self.K, self.W, self.V, self.eos_id, self.max_states = list(parts), len(parts), (len(parts) + 1) // 2, V, eos_id, max_states
        self.weighted = any(p.weighted for p in parts)
        self.start, self.start_logw = 0, float(sum(p.start_logw for p in parts))
        first = tuple(int(p.start) for p in parts)
        self.order, self.ids, self.overflow = [first], {first: 0}, False
        self._rows = {}

    n_states = property(lambda self: len(self.order))

    def tuples(self):
        return list(self.order)

    def words(self):
        """uint64 [n_states, W]: two part states a word, part 2 j the low half of word j; odd K: the last high half zero."""
        out = np.zeros((len(self.order), 2 * self.W), np.uint32)
        out[:, :self.K] = np.array(self.order, np.int64).reshape(len(self.order), self.K).astype(np.uint32)
        return np.ascontiguousarray(out).view("<u8")

    def unpack(self, states, n):
        """int32 [K, n]: -1 in every part for a state that is dead or not numbered yet (None: state 0)."""
        known = len(self.order)
        out = np.full((self.K, n), -1, np.int32)
        for i in range(n):
            s = 0 if states is None else int(states[i])
            if 0 <= s < known:
                out[:, i] = self.order[s]
        return out

    def advance(self, states, tokens, frm, to):
        n = len(frm)
        ps = self.unpack(states, n)
        nxt = np.stack([p.advance(ps[k], tokens, frm, to) for k, p in enumerate(self.parts)])
        out = np.full(n, -1, np.int32)
        for i in range(n):  # (particle order: a new tuple gets the next id when the smallest particle that reached it is met)
            if (nxt[:, i] < 0).any():
                continue
            key = tuple(int(v) for v in nxt[:, i])
            if key not in self.ids:
                if len(self.order) >= self.max_states:
                    self.overflow = True
                    continue
                self.ids[key] = len(self.order)
                self.order.append(key)
            out[i] = self.ids[key]
        return out

    def row(self, s):
        """The bank row of state s from the parts' rows: uint32 words, or float32 [V] when a part is weighted."""
        if s in self._rows:
            return self._rows[s]
        rows = [p.row(int(v)) for p, v in zip(self.parts, self.order[s])]
        if not self.weighted:
            out = rows[0].copy()
            for r in rows[1:]:
                out &= r
        else:
            out = np.zeros(self.V, np.float32)
            for p, r in zip(self.parts, rows):  # part order, float32, one rounded addition a part
                if p.weighted:
                    out = (out + r).astype(np.float32)
            for p, r in zip(self.parts, rows):
                if not p.weighted:
                    out[~bits_of(r, self.V)] = NINF
        self._rows[s] = out
        return out

    def accepts(self, s):
        """Whether row 1 is served under `done`: every part accepts."""
        r = self.row(s)
        return bool(r[self.eos_id] > NINF) if self.weighted else bool(bits_of(r, self.V)[self.eos_id])

    def row_dead(self):
        return np.full(self.V, NINF, np.float32) if self.weighted else np.zeros((self.V + 31) // 32, np.uint32)

    def row_eos(self):
        out = self.row_dead()
        if self.weighted:
            out[self.eos_id] = 0.0
        else:
            out[self.eos_id >> 5] = np.uint32(1 << (self.eos_id & 31))
        return out

    def final_logw(self, s):
        """The sum, in part order, of the weighted parts' final weights (float32 additions from 0.0)."""
        w = np.float32(0.0)
        for p, v in zip(self.parts, self.order[s]):
            if p.weighted:
                w = np.float32(w + p.final_logw(int(v)))
        return w
