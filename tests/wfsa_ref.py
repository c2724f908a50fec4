"""The contract of a weighted byte automaton's rows (include/glb.h glb_dfa_weight_*), restated in NumPy by brute force on top
of tests/dfa_ref.py: every state against every token, byte by byte, the weights one float32 addition per byte in byte
order.  Test infrastructure: the product never imports it."""
import numpy as np

from tests import dfa_ref as R

NINF = np.float32(-np.inf)


class WRef(R.Ref):
    """`dfa_ref.Ref` of the automaton with accepting = final_logw > -inf and the arcs of weight -inf removed, plus the
    weights."""

    def __init__(self, delta, arc_logw, final_logw, start, vocab, eos_id, skip_ids=()):
        self.arc = np.asarray(arc_logw, np.float32).copy()
        self.final = np.asarray(final_logw, np.float32).copy()
        delta = np.array(delta, np.int64)
        delta[np.isneginf(self.arc)] = -1
        self.arc[delta < 0] = NINF
        super().__init__(delta, self.final > NINF, start, vocab, eos_id, skip_ids)

    def weight(self, s, t):
        """The column of token t in the row of state s, one token byte by byte (eos_id is the caller's business)."""
        if self.next(s, t) < 0:
            return NINF
        w = np.float32(0.0)
        for b in self.vocab[t]:
            w = np.float32(w + self.arc[s, b])
            s = int(self.delta[s, b])
        return w

    def weights_all(self, s):
        """float32 [V]: every token's column, all tokens walked side by side, one byte position at a time."""
        if s < 0:
            return np.full(self.V, NINF, np.float32)
        cur = np.full(self.V, s, np.int64)
        w = np.zeros(self.V, np.float32)
        for j in range(self.padded.shape[1]):
            on = (j < self.lens) & (cur >= 0)
            at = np.maximum(cur, 0)
            w = np.where(on, w + self.arc[at, self.padded[:, j]], w).astype(np.float32)
            cur = np.where(on, self.delta[at, self.padded[:, j]], cur)
        return np.where(self.next_all(s) >= 0, w, NINF).astype(np.float32)

    def row(self, s):
        """float32 [V]: the bank row of state s."""
        out = self.weights_all(s)
        if 0 <= self.eos_id < self.V:
            out[self.eos_id] = self.final[s] if s >= 0 else NINF
        return out

    def wrow_dead(self):
        return np.full(self.V, NINF, np.float32)

    def wrow_eos(self):
        out = self.wrow_dead()
        out[self.eos_id] = 0.0
        return out

    def path_logw(self, data):
        s, w = self.start, np.float32(0.0)
        for b in bytes(data):
            w = np.float32(w + self.arc[s, b])
            s = int(self.delta[s, b])
            if s < 0:
                return NINF
        return np.float32(w + self.final[s])


def random_weights(delta, accepting, seed):
    """(arc_logw, final_logw): seeded arc weights in [-4, 0] on the arcs of delta, final weights in [-2, 0] on the accepting
    states, -inf elsewhere."""
    rng = np.random.default_rng(seed)
    delta, accepting = np.asarray(delta), np.asarray(accepting, np.bool_)
    arc = np.where(delta >= 0, -4.0 * rng.random(delta.shape), -np.inf).astype(np.float32)
    fin = np.where(accepting, -2.0 * rng.random(accepting.shape), -np.inf).astype(np.float32)
    return arc, fin


def zero_weights(delta, accepting):
    delta, accepting = np.asarray(delta), np.asarray(accepting, np.bool_)
    return (np.where(delta >= 0, 0.0, -np.inf).astype(np.float32), np.where(accepting, 0.0, -np.inf).astype(np.float32))


def bits_to_weights(words, V):
    """where(bit, 0, -inf) of a GLB_MASK_BITS row (uint32 words)."""
    bits = np.unpackbits(np.ascontiguousarray(words, "<u4").view(np.uint8), bitorder="little")[:V]
    return np.where(bits > 0, np.float32(0.0), NINF).astype(np.float32)
