"""float64 restatement of a byte beam under a byte automaton (glb_bytelm_step, `ByteBeam(constraint=...)`, `ByteSIS`; DESIGN.md
§33), written from the contract in include/glb.h on top of tests/bytelm_ref.py.

An automaton is anything with `delta` [S, 256], `accepting` [S], `live` [S] and, both or neither, `arc_logw` [S, 256] and
`final_logw` [S]: a host `ByteDFA` / `ByteWFSA`, or a namespace of arrays (the kernel tests hand over tables no constructor
would make, such as an arc of weight -inf that delta still has)."""
import math

import numpy as np

from tests import bytelm_ref as R

EOS = 256
NINF = float("-inf")


def lc_row(row, automaton, state):
    """float64 [257]: the unconstrained row plus the automaton's weights at `state`, -inf where it forbids."""
    delta, S = automaton.delta, automaton.delta.shape[0]
    arc, fin = getattr(automaton, "arc_logw", None), getattr(automaton, "final_logw", None)
    lc = np.full(257, NINF)
    if not 0 <= state < S:
        return lc
    for b in range(256):
        t = int(delta[state, b])
        if 0 <= t < S and automaton.live[t]:
            v = float(row[b]) + (float(arc[state, b]) if arc is not None else 0.0)
            if math.isfinite(v):
                lc[b] = v
    if automaton.accepting[state]:
        v = float(row[EOS]) + (float(fin[state]) if fin is not None else 0.0)
        if math.isfinite(v):
            lc[EOS] = v
    return lc


def constrained_row(row, automaton, state):
    """(lc - logZc, logZc): float64 [257] and a float; all -inf and -inf where nothing allowed has mass."""
    lc = lc_row(row, automaton, state)
    m = lc.max()
    if m == NINF:
        return lc, NINF
    logZc = m + math.log(np.exp(lc - m).sum())
    return lc - logZc, logZc


def cdf(row):
    """float64 [257]: the cumulative probabilities of exp(row) in column order."""
    with np.errstate(under="ignore"):
        return np.cumsum(np.where(row > NINF, np.exp(row), 0.0))


def pick(row, uniform):
    """The first column with a finite entry whose cumulative probability exceeds `uniform`; the last finite column where
    none does; -1 for a row of -inf."""
    cum = cdf(row)
    last = -1
    for c in range(257):
        if row[c] > NINF:
            if cum[c] > uniform:
                return c
            last = c
    return last


class RefConstrainedBeam:
    """One group of `ByteBeam(constraint=automaton)` on the host: a `RefBeam` with a state, an ended flag and a log-weight."""

    def __init__(self, lm, vocab, eos_ids, width, automaton, ignore_ids=()):
        self.beam, self.a = R.RefBeam(lm, vocab, eos_ids, width, ignore_ids), automaton
        self.state, self.ended, self.log_weight = int(automaton.start), False, 0.0

    pruned = property(lambda self: self.beam.pruned)
    logp = property(lambda self: self.beam.logp)

    def _rows(self):
        if self.ended:
            return np.full(257, NINF), np.full(257, NINF), NINF
        lc = lc_row(self.beam.next_byte_logprobs(), self.a, self.state)
        return (lc,) + constrained_row(self.beam.next_byte_logprobs(), self.a, self.state)

    def next_byte_logprobs(self):
        return self._rows()[1]

    def next_byte_logZ(self):
        return self._rows()[2]

    def _move(self, byte, dead, weight):
        if dead:
            self.beam.next_byte_logprobs()
            if byte >= 0:
                self.beam.logp += self.beam.next_byte_logprobs()[byte]
            self.beam.cands = [None] * len(self.beam.cands)
            self.beam.fresh, self.beam._row = True, None
            self.state, self.log_weight = -1, NINF
            return
        self.beam.advance(byte)
        self.log_weight += weight
        if byte == EOS:
            self.state, self.ended = -1, True
        else:
            self.state = int(self.a.delta[self.state, byte])

    def advance(self, byte):
        """A given byte: the weight is the automaton's own for it (0 without weights); a forbidden one, or one without mass,
        kills the group."""
        if self.ended or byte < 0:
            return
        lc, _, logZc = self._rows()
        arc, fin = getattr(self.a, "arc_logw", None), getattr(self.a, "final_logw", None)
        own = 0.0 if arc is None else float(fin[self.state]) if byte == EOS else float(arc[self.state, byte])
        self._move(byte, logZc == NINF or lc[byte] == NINF, own)

    def step(self, uniform):
        """A drawn byte (`pick`): the weight is logZc.  Returns the byte, -1 for a group that had ended or dies."""
        if self.ended:
            return -1
        _, row, logZc = self._rows()
        byte = pick(row, uniform)
        self._move(byte, logZc == NINF, logZc)
        return byte if logZc > NINF else -1
