"""The host automata: `ByteDFA` and `ByteWFSA`, its twin in the log semiring.  NumPy only."""
import numpy as np


class ByteDFA:
    """delta int32 [S, 256] (-1: no transition), accepting bool [S], start in [0, S).  `live[s]`: some accepting state is
    reachable from s (s included)."""

    def __init__(self, delta, accepting, start):
        delta = np.asarray(delta)
        accepting = np.asarray(accepting)
        if delta.ndim != 2 or delta.shape[1] != 256 or delta.shape[0] == 0:
            raise ValueError(f"delta must be [S, 256] with S >= 1, got {delta.shape}")
        if not np.issubdtype(delta.dtype, np.integer):
            raise ValueError("delta must hold integers")
        S = delta.shape[0]
        if S > 0x7fffff00:
            raise ValueError("too many states")
        if delta.min() < -1 or delta.max() >= S:
            raise ValueError(f"delta entries must be -1 or a state in [0, {S})")
        if accepting.shape != (S,):
            raise ValueError(f"accepting must be [{S}], got {accepting.shape}")
        if accepting.dtype != np.bool_ and not np.isin(accepting, (0, 1)).all():
            raise ValueError("accepting must be boolean")
        if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or not 0 <= int(start) < S:
            raise ValueError(f"start must be an int in [0, {S})")
        self.delta = np.ascontiguousarray(delta, dtype=np.int32)
        self.accepting = np.ascontiguousarray(accepting.astype(np.bool_))
        self.start = int(start)
        self.n_states = S
        self.live = self._live()

    @classmethod
    def _from_device(cls, delta, accepting, start, live, arc_logw=None, final_logw=None):
        """The automaton of tables that the device made and checked (`product`): `live` is the device's, nothing is searched
        again.  With weights (`cls` a `ByteWFSA`) `accepting` is final_logw > -inf, as the constructor has it."""
        self = cls.__new__(cls)
        self.delta = np.ascontiguousarray(delta, dtype=np.int32)
        self.accepting = np.ascontiguousarray(accepting, dtype=np.bool_)
        self.start, self.n_states = int(start), self.delta.shape[0]
        self.live = np.ascontiguousarray(live, dtype=np.bool_)
        if arc_logw is not None:
            self.arc_logw = np.ascontiguousarray(arc_logw, dtype=np.float32)
            self.final_logw = np.ascontiguousarray(final_logw, dtype=np.float32)
        return self

    def _live(self):
        """Backwards reachability from the accepting states over the reversed transition graph."""
        S = self.n_states
        src = np.repeat(np.arange(S, dtype=np.int64), 256)
        dst = self.delta.reshape(-1).astype(np.int64)
        keep = dst >= 0
        src, dst = src[keep], dst[keep]
        order = np.argsort(dst, kind="stable")
        src, dst = src[order], dst[order]
        first = np.searchsorted(dst, np.arange(S + 1))
        live = self.accepting.copy()
        todo = list(np.nonzero(live)[0])
        while todo:
            s = todo.pop()
            for p in src[first[s]:first[s + 1]]:
                if not live[p]:
                    live[p] = True
                    todo.append(int(p))
        return live

    @classmethod
    def from_strings(cls, strings):
        """The trie automaton of a finite language: accepts exactly the given byte strings."""
        strings = [bytes(s) for s in strings]
        if not strings:
            raise ValueError("from_strings needs at least one string")
        rows, acc = [np.full(256, -1, np.int32)], [False]
        for s in strings:
            cur = 0
            for b in s:
                if rows[cur][b] < 0:
                    rows[cur][b] = len(rows)
                    rows.append(np.full(256, -1, np.int32))
                    acc.append(False)
                cur = int(rows[cur][b])
            acc[cur] = True
        return cls(np.stack(rows), np.array(acc, np.bool_), 0)

    @classmethod
    def from_regex(cls, pattern, max_states=65536, device=None):
        """The automaton of a regular expression over bytes: accepts exactly the byte strings `d` for which
        `re.compile(pattern).fullmatch(d)` matches, `pattern` read as Python's `re` reads a BYTES pattern without flags (a
        `str` is encoded as UTF-8 first: a non-ASCII character is the sequence of its bytes, and a quantifier behind it
        repeats the last byte).  Supported: literals, the escapes \\\\ \\n \\t \\r \\xHH and escaped punctuation, `.` (any byte
        but 0x0A), classes [...] with ranges and negation, \\d \\D \\w \\W \\s \\S (ASCII) inside and outside classes, groups
        (...) and (?:...), alternation, and the quantifiers * + ? {m} {m,} {m,n} {,n} with bounds up to 1000.  Everything
        else - anchors, backreferences, lookaround, lazy and possessive quantifiers, inline flags, named groups, \\b \\B \\A
        \\Z - raises ValueError naming the construct and its position, and so does a subset construction that passes
        `max_states`.  Start state 0; the result is not minimised (`minimize`, `DeviceConstraint(minimize=True)`).  Host
        only: a Thompson automaton and its subset construction - unless `device` is an `llm` or an engine: then the subset
        construction runs there (`determinize(device, ByteNFA.from_regex(pattern), max_states)[0]`), the same
        automaton with its states numbered in byte order instead of byte-group order."""
        if isinstance(pattern, str):
            pattern = pattern.encode("utf-8")
        if isinstance(max_states, bool) or not isinstance(max_states, (int, np.integer)) or max_states < 1:
            raise ValueError(f"max_states must be an int >= 1, got {max_states!r}")
        if device is not None:
            from .nfa import ByteNFA
            from .tables import determinize

            return determinize(device, ByteNFA.from_regex(pattern, int(max_states)), int(max_states))[0]
        from .regex import _regex_dfa

        delta, accepting = _regex_dfa(bytes(pattern), int(max_states))
        return cls(delta, accepting, 0)

    @property
    def reachable(self):
        """bool [S]: the states some byte string reaches from `start` (a frontier search, a NumPy step per depth)."""
        seen = np.zeros(self.n_states, np.bool_)
        seen[self.start] = True
        frontier = np.array([self.start], np.int64)
        while frontier.size:
            nxt = np.unique(self.delta[frontier])
            nxt = nxt[nxt >= 0]
            frontier = nxt[~seen[nxt]]
            seen[frontier] = True
        return seen

    def accepts(self, data):
        s = self.start
        for b in bytes(data):
            s = int(self.delta[s, b])
            if s < 0:
                return False
        return bool(self.accepting[s])



class ByteWFSA(ByteDFA):
    """A deterministic automaton over bytes in the log semiring: delta as in `ByteDFA`, arc_logw float32 [S, 256], final_logw
    float32 [S] (-inf: not accepting).  It is the `ByteDFA` with accepting = final_logw > -inf.  An arc of weight -inf is
    removed (delta becomes -1) before `live` is computed; NaN, +inf and a finite weight on an arc that delta does not have
    are errors."""

    def __init__(self, delta, arc_logw, final_logw, start):
        delta = np.array(delta)
        arc = np.array(arc_logw, dtype=np.float32)
        fin = np.ascontiguousarray(final_logw, dtype=np.float32)
        if delta.ndim != 2 or arc.shape != delta.shape:
            raise ValueError(f"arc_logw must have delta's shape [S, 256], got {arc.shape} beside {delta.shape}")
        if fin.shape != delta.shape[:1]:
            raise ValueError(f"final_logw must be [{delta.shape[0]}], got {fin.shape}")
        for name, a in (("arc_logw", arc), ("final_logw", fin)):
            if np.isnan(a).any() or np.isposinf(a).any():
                raise ValueError(f"{name} holds NaN or +inf")
        if not np.issubdtype(delta.dtype, np.integer):
            raise ValueError("delta must hold integers")
        if (np.isfinite(arc) & (delta == -1)).any():
            raise ValueError("arc_logw is finite where delta has no arc")
        delta[np.isneginf(arc)] = -1
        arc[delta < 0] = -np.inf
        super().__init__(delta, fin > -np.inf, start)
        self.arc_logw, self.final_logw = np.ascontiguousarray(arc), fin

    @classmethod
    def from_dfa(cls, dfa):
        """`dfa` with weight zero on every arc and every accepting state."""
        return cls(dfa.delta, np.where(dfa.delta >= 0, 0.0, -np.inf), np.where(dfa.accepting, 0.0, -np.inf), dfa.start)

    @classmethod
    def from_weighted_strings(cls, weights):
        """The trie automaton of {byte string: log-weight}: arcs weigh zero, a string's weight sits on its final state."""
        strings = [bytes(s) for s in weights]
        dfa = ByteDFA.from_strings(strings)
        fin = np.full(dfa.n_states, -np.inf, np.float32)
        for s, w in zip(strings, weights.values()):
            cur = dfa.start
            for b in s:
                cur = int(dfa.delta[cur, b])
            fin[cur] = w
        return cls(dfa.delta, np.where(dfa.delta >= 0, 0.0, -np.inf), fin, dfa.start)

    def path_logw(self, data):
        """float32: the arcs' weights summed left to right, plus the final weight; -inf where `data` is not accepted."""
        s, w = self.start, np.float32(0.0)
        for b in bytes(data):
            w = np.float32(w + self.arc_logw[s, b])
            s = int(self.delta[s, b])
            if s < 0:
                return np.float32(-np.inf)
        return np.float32(w + self.final_logw[s])
