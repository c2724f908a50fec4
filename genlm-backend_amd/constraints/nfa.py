"""`ByteNFA`: a byte automaton with empty arcs, the operand of `determinize`.  NumPy only.  Union,
concatenation and closure are array concatenation with offsets here; none of them exists on [S, 256] tables."""
import numpy as np

from .automata import ByteDFA, ByteWFSA


def _ints(name, a, n):
    a = np.asarray(a)
    if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
        raise ValueError(f"{name} must be a vector of integers, got dtype {a.dtype} and shape {a.shape}")
    if a.size and (a.min() < 0 or a.max() >= n):
        raise ValueError(f"{name} entries must be states in [0, {n})")
    return np.ascontiguousarray(a, dtype=np.int32)


class ByteNFA:
    """n_states states, `start` in [0, n), accepting bool [n]; byte arcs arc_src, arc_dst int32 [A] with arc_set bool [A, 256]
    (the bytes arc i reads); empty arcs eps_src, eps_dst int32 [E].  A state is `important` when it has a byte arc or
    accepts: `determinize` keeps sets of those."""

    def __init__(self, n_states, start, accepting, arc_src, arc_dst, arc_set, eps_src=(), eps_dst=()):
        if isinstance(n_states, bool) or not isinstance(n_states, (int, np.integer)) or not 1 <= int(n_states) <= 0x7fffff00:
            raise ValueError(f"n_states must be an int in [1, 2^31 - 256], got {n_states!r}")
        n = int(n_states)
        if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or not 0 <= int(start) < n:
            raise ValueError(f"start must be an int in [0, {n})")
        accepting = np.asarray(accepting)
        if accepting.shape != (n,):
            raise ValueError(f"accepting must be [{n}], got {accepting.shape}")
        if accepting.dtype != np.bool_ and not np.isin(accepting, (0, 1)).all():
            raise ValueError("accepting must be boolean")
        self.arc_src, self.arc_dst = _ints("arc_src", arc_src, n), _ints("arc_dst", arc_dst, n)
        self.eps_src, self.eps_dst = _ints("eps_src", eps_src, n), _ints("eps_dst", eps_dst, n)
        arc_set = np.asarray(arc_set)
        if arc_set.size == 0:
            arc_set = np.zeros((0, 256), np.bool_)
        if arc_set.shape != (len(self.arc_src), 256) or self.arc_dst.shape != self.arc_src.shape:
            raise ValueError(f"arc_src, arc_dst and arc_set must be [A], [A] and [A, 256], got {self.arc_src.shape}, {self.arc_dst.shape}, {arc_set.shape}")
        if arc_set.dtype != np.bool_ and not np.isin(arc_set, (0, 1)).all():
            raise ValueError("arc_set must be boolean")
        if self.eps_src.shape != self.eps_dst.shape:
            raise ValueError(f"eps_src and eps_dst must have one shape, got {self.eps_src.shape} and {self.eps_dst.shape}")
        self.n_states, self.start = n, int(start)
        self.accepting = np.ascontiguousarray(accepting.astype(np.bool_))
        self.arc_set = np.ascontiguousarray(arc_set.astype(np.bool_))

    @property
    def important(self):
        """bool [n]: the states with a byte arc, and the accepting ones."""
        imp = self.accepting.copy()
        imp[self.arc_src] = True
        return imp

    def _closed(self, cur):
        while True:
            more = np.zeros_like(cur)
            more[self.eps_dst[cur[self.eps_src]]] = True
            more &= ~cur
            if not more.any():
                return cur
            cur |= more

    def accepts(self, data):
        """Whether some path of `data`'s bytes and any empty arcs leads from `start` to an accepting state: the set of
        states reached, byte by byte."""
        cur = np.zeros(self.n_states, np.bool_)
        cur[self.start] = True
        cur = self._closed(cur)
        for b in bytes(data):
            nxt = np.zeros(self.n_states, np.bool_)
            nxt[self.arc_dst[cur[self.arc_src] & self.arc_set[:, b]]] = True
            cur = self._closed(nxt)
            if not cur.any():
                return False
        return bool((cur & self.accepting).any())

    # ---- constructors: array concatenation with offsets --------------------------------------------------------------------------
    @classmethod
    def from_dfa(cls, dfa):
        """`dfa` as it is: its states, one byte arc for every (state, target) pair that some byte joins, no empty arcs."""
        if isinstance(dfa, ByteWFSA):
            raise ValueError("ByteNFA takes unweighted automata: a ByteWFSA's weights would be lost, and weighted "
                             "determinisation need not terminate")
        if not isinstance(dfa, ByteDFA):
            raise ValueError(f"from_dfa needs a ByteDFA, got {type(dfa).__name__}")
        S = dfa.n_states
        flat = dfa.delta.reshape(-1).astype(np.int64)
        at = np.nonzero(flat >= 0)[0]
        pair, arc_of = np.unique((at // 256) * S + flat[at], return_inverse=True)
        arc_set = np.zeros((len(pair), 256), np.bool_)
        arc_set[np.asarray(arc_of).reshape(-1), at % 256] = True
        return cls(S, dfa.start, dfa.accepting, pair // S, pair % S, arc_set)

    @classmethod
    def from_regex(cls, pattern, max_states=65536):
        """The Thompson automaton of `pattern`, the one `ByteDFA.from_regex` determinises on the host: the same parser, the
        same constructs refused by name.  `max_states` bounds the automaton alone, at 8 * max_states + 4096 states."""
        from .regex import _thompson

        if isinstance(pattern, str):
            pattern = pattern.encode("utf-8")
        if isinstance(max_states, bool) or not isinstance(max_states, (int, np.integer)) or max_states < 1:
            raise ValueError(f"max_states must be an int >= 1, got {max_states!r}")
        nfa, first, last = _thompson(bytes(pattern), int(max_states))
        n = len(nfa.eps)
        src = [i for i in range(n) if nfa.arc[i] is not None]
        eps_n = np.fromiter((len(e) for e in nfa.eps), np.int64, n)
        accepting = np.zeros(n, np.bool_)
        accepting[last] = True
        return cls(n, first, accepting, np.asarray(src, np.int32), np.asarray([nfa.arc[i][1] for i in src], np.int32),
                   np.stack([nfa.arc[i][0] for i in src]) if src else np.zeros((0, 256), np.bool_),
                   np.repeat(np.arange(n, dtype=np.int32), eps_n), np.asarray([v for e in nfa.eps for v in e], np.int32))

    @staticmethod
    def _operands(items, what):
        items = list(items)
        if not items:
            raise ValueError(f"{what} needs at least one automaton")
        out = []
        for x in items:
            if isinstance(x, ByteDFA):
                x = ByteNFA.from_dfa(x)
            if not isinstance(x, ByteNFA):
                raise ValueError(f"{what} needs ByteNFA or ByteDFA operands, got {type(x).__name__}")
            out.append(x)
        return out

    @classmethod
    def _joined(cls, items, extra, start, accepting, eps_src, eps_dst):
        """The disjoint union of `items` behind `extra` new states (ids 0 .. extra - 1), with further empty arcs."""
        off = extra + np.concatenate([[0], np.cumsum([x.n_states for x in items])]).astype(np.int64)
        cat = lambda name: np.concatenate([getattr(x, name) + o for x, o in zip(items, off)]).astype(np.int32)
        return cls(int(off[-1]), start, accepting, cat("arc_src"), cat("arc_dst"), np.concatenate([x.arc_set for x in items]),
                   np.concatenate([cat("eps_src"), np.asarray(eps_src, np.int64)]).astype(np.int32),
                   np.concatenate([cat("eps_dst"), np.asarray(eps_dst, np.int64)]).astype(np.int32)), off

    @classmethod
    def union(cls, items):
        """The strings that any of `items` accepts (each a `ByteNFA` or a `ByteDFA`): a new start with an empty arc to every
        item's start."""
        items = cls._operands(items, "union")
        off = 1 + np.concatenate([[0], np.cumsum([x.n_states for x in items])])
        acc = np.concatenate([[False]] + [x.accepting for x in items])
        starts = [x.start + o for x, o in zip(items, off)]
        return cls._joined(items, 1, 0, acc, np.zeros(len(items), np.int64), starts)[0]

    @classmethod
    def concat(cls, items):
        """The strings that are one string of every item in turn: an empty arc from every accepting state of an item to the
        start of the next; the last item's accepting states accept."""
        items = cls._operands(items, "concat")
        off = np.concatenate([[0], np.cumsum([x.n_states for x in items])])
        acc = np.concatenate([np.zeros(x.n_states, np.bool_) for x in items[:-1]] + [items[-1].accepting])
        src = [np.nonzero(x.accepting)[0] + o for x, o in zip(items[:-1], off)]
        dst = [np.full(len(s), nxt.start + o, np.int64) for s, nxt, o in zip(src, items[1:], off[1:])]
        return cls._joined(items, 0, items[0].start, acc, np.concatenate(src + [np.zeros(0, np.int64)]),
                           np.concatenate(dst + [np.zeros(0, np.int64)]))[0]

    def _looped(self, new_start, new_accepts, back):
        """This automaton behind `new_start` new start states (0 or 1), with an empty arc from every accepting state back to
        the start where `back`."""
        fin = np.nonzero(self.accepting)[0] + new_start
        first = 0 if new_start else self.start
        src = np.concatenate([[0] if new_start else [], fin if back else []]).astype(np.int64)
        dst = np.concatenate([[self.start + 1] if new_start else [], np.full(len(fin) if back else 0, first)]).astype(np.int64)
        acc = np.concatenate([[new_accepts] if new_start else [], self.accepting]).astype(np.bool_)
        return ByteNFA._joined([self], new_start, first, acc, src, dst)[0]

    def star(self):
        """Zero or more strings of this automaton in a row."""
        return self._looped(1, True, True)

    def plus(self):
        """One or more strings of this automaton in a row."""
        return self._looped(0, False, True)

    def optional(self):
        """The empty string, or a string of this automaton."""
        return self._looped(1, True, False)
