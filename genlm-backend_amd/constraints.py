"""Byte-level DFA constraints on the device (include/glb.h glb_dfa_*).

`ByteDFA` is the automaton a user brings (a compiled regex, a literal set, a schema: a transition table over bytes);
`DeviceConstraint` keeps it on the GPU beside the vocabulary's byte strings and produces what the fused step consumes:
a bank of token bit masks, one row per automaton state that some particle has reached, and every particle's row.  States
advance on the device from the tokens drawn; nothing crosses the host per step.

`ByteWFSA` is the same automaton in the log semiring (arc and final log-weights): a `DeviceConstraint` over one
keeps a bank of float32 rows - the token log-weights from every state reached - that the step adds to the log-probabilities.

`DeviceConstraint(..., on_full="evict")` lets the bank be smaller than the automaton: a cache over the states,
the least recently requested rows recycled and filled again on the device.
"""
import ctypes as C

import numpy as np

from . import _lib


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
    def from_regex(cls, pattern, max_states=65536):
        """The automaton of a regular expression over bytes: accepts exactly the byte strings `d` for which
        `re.compile(pattern).fullmatch(d)` matches, `pattern` read as Python's `re` reads a BYTES pattern without flags (a
        `str` is encoded as UTF-8 first: a non-ASCII character is the sequence of its bytes, and a quantifier behind it
        repeats the last byte).  Supported: literals, the escapes \\\\ \\n \\t \\r \\xHH and escaped punctuation, `.` (any byte
        but 0x0A), classes [...] with ranges and negation, \\d \\D \\w \\W \\s \\S (ASCII) inside and outside classes, groups
        (...) and (?:...), alternation, and the quantifiers * + ? {m} {m,} {m,n} {,n} with bounds up to 1000.  Everything
        else - anchors, backreferences, lookaround, lazy and possessive quantifiers, inline flags, named groups, \\b \\B \\A
        \\Z - raises ValueError naming the construct and its position, and so does a subset construction that passes
        `max_states`.  Start state 0; the result is not minimised (`minimize`, `DeviceConstraint(minimize=True)`).  Host
        only: a Thompson automaton and its subset construction."""
        if isinstance(pattern, str):
            pattern = pattern.encode("utf-8")
        if isinstance(max_states, bool) or not isinstance(max_states, (int, np.integer)) or max_states < 1:
            raise ValueError(f"max_states must be an int >= 1, got {max_states!r}")
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


# ---- the regex compiler (ByteDFA.from_regex) -----------------------------------------------------------------------------------
_REGEX_MAX_BOUND = 1000


def _byteset(*items):
    s = np.zeros(256, np.bool_)
    for it in items:
        if isinstance(it, tuple):
            s[it[0]:it[1] + 1] = True
        else:
            s[it] = True
    return s


_SHORTHAND = {ord("d"): _byteset((48, 57)), ord("w"): _byteset((48, 57), (65, 90), (97, 122), 95), ord("s"): _byteset((9, 13), 32)}
_ESCAPED = {ord("n"): 10, ord("t"): 9, ord("r"): 13}
_REFUSED_ESCAPES = {ord("b"): "the word boundary \\b", ord("B"): "the word boundary \\B", ord("A"): "the anchor \\A",
                    ord("Z"): "the anchor \\Z"}


class _RegexParser:
    """Recursive descent over a bytes pattern into a tree of ("set", bool[256]) / ("cat", [nodes]) / ("alt", [nodes]) /
    ("rep", node, m, n or None)."""

    def __init__(self, pattern):
        self.p, self.i = pattern, 0

    def fail(self, what, at=None):
        raise ValueError(f"from_regex: {what} at position {self.i if at is None else at} of {self.p!r} is not supported")

    def peek(self):
        return self.p[self.i] if self.i < len(self.p) else None

    def parse(self):
        node = self.alternation()
        if self.i < len(self.p):
            self.fail("an unbalanced ')'")
        return node

    def alternation(self):
        branches = [self.sequence()]
        while self.peek() == ord("|"):
            self.i += 1
            branches.append(self.sequence())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def sequence(self):
        items = []
        while self.peek() is not None and self.peek() not in b"|)":
            at = self.i
            atom = self.atom()
            q = self.quantifier()
            if q is not None:
                if atom is None:
                    self.fail("a quantifier with nothing to repeat", at)
                nxt = self.peek()
                if nxt == ord("?"):
                    self.fail("a lazy quantifier")
                if nxt == ord("+"):
                    self.fail("a possessive quantifier")
                if nxt == ord("*") or (nxt == ord("{") and self.quantifier(probe=True)):
                    self.fail("a repeated quantifier")
                atom = ("rep", atom, q[0], q[1])
            if atom is not None:
                items.append(atom)
        return ("cat", items)

    def quantifier(self, probe=False):
        """(m, n or None) when a quantifier stands here (consumed unless `probe`), else None; a '{' that opens no
        quantifier is a literal, as in `re`."""
        c, here = self.peek(), self.i
        if c is None or c not in b"*+?{":
            return None
        if c != ord("{"):
            if not probe:
                self.i += 1
            return {ord("*"): (0, None), ord("+"): (1, None), ord("?"): (0, 1)}[c]
        j = here + 1
        lo = hi = b""
        while j < len(self.p) and self.p[j] in b"0123456789":
            lo, j = lo + self.p[j:j + 1], j + 1
        if j < len(self.p) and self.p[j] == ord(","):
            j += 1
            while j < len(self.p) and self.p[j] in b"0123456789":
                hi, j = hi + self.p[j:j + 1], j + 1
            comma = True
        else:
            hi, comma = lo, False
        if j >= len(self.p) or self.p[j] != ord("}") or (not comma and not lo):
            return None  # not a quantifier: '{' is a literal
        m, n = int(lo) if lo else 0, int(hi) if hi else None
        if m > _REGEX_MAX_BOUND or (n is not None and n > _REGEX_MAX_BOUND):
            self.fail(f"a repetition bound above {_REGEX_MAX_BOUND}", here)
        if n is not None and n < m:
            self.fail("a repetition whose maximum lies below its minimum", here)
        if not probe:
            self.i = j + 1
        return (m, n)

    def atom(self):
        """A node, or None where a quantifier stands with nothing before it."""
        c, at = self.peek(), self.i
        if c in b"*+?" or (c == ord("{") and self.quantifier(probe=True)):
            return None
        self.i += 1
        if c == ord("("):
            if self.peek() == ord("?"):
                nxt = self.p[self.i + 1:self.i + 3]
                if nxt[:1] != b":":
                    kinds = [(b"P<", "a named group"), (b"P=", "a backreference"), (b"=", "lookaround"), (b"!", "lookaround"),
                             (b"<=", "lookaround"), (b"<!", "lookaround"), (b"#", "a comment group"), (b"(", "a conditional group"),
                             (b">", "an atomic group")]
                    self.fail(next((name for head, name in kinds if nxt.startswith(head)), "an inline flag or group extension"), at)
                self.i += 2
            node = self.alternation()
            if self.peek() != ord(")"):
                self.fail("an unbalanced '('", at)
            self.i += 1
            return node
        if c == ord("["):
            return ("set", self.char_class(at))
        if c == ord("."):
            s = np.ones(256, np.bool_)
            s[10] = False
            return ("set", s)
        if c == ord("^") or c == ord("$"):
            self.fail(f"the anchor {chr(c)}", at)
        if c == ord("\\"):
            return ("set", self.escape(at, in_class=False))
        return ("set", _byteset(c))

    def escape(self, at, in_class):
        """The byte set of the escape whose backslash stands at `at` (self.i is behind the backslash)."""
        c = self.peek()
        if c is None:
            self.fail("a trailing backslash", at)
        self.i += 1
        if (c | 32) in _SHORTHAND:
            s = _SHORTHAND[c | 32]
            return s.copy() if c & 32 else ~s
        if c in _ESCAPED:
            return _byteset(_ESCAPED[c])
        if c == ord("x"):
            digits = self.p[self.i:self.i + 2]
            if len(digits) != 2 or any(d not in b"0123456789abcdefABCDEF" for d in digits):
                self.fail("an incomplete \\x escape", at)
            self.i += 2
            return _byteset(int(digits, 16))
        if c in _REFUSED_ESCAPES:
            self.fail(_REFUSED_ESCAPES[c], at)
        if c in b"0123456789":
            self.fail("a backreference or octal escape", at)
        if c < 128 and chr(c).isalpha():
            self.fail(f"the escape \\{chr(c)}", at)
        return _byteset(c)  # escaped punctuation (and bytes >= 0x80): the byte itself

    def char_class(self, at):
        s = np.zeros(256, np.bool_)
        negate = self.peek() == ord("^")
        if negate:
            self.i += 1
        first = True
        while True:
            c, here = self.peek(), self.i
            if c is None:
                self.fail("an unterminated character class", at)
            self.i += 1
            if c == ord("]") and not first:
                break
            first = False
            lo = self.escape(here, in_class=True) if c == ord("\\") else _byteset(c)
            if self.peek() == ord("-") and self.i + 1 < len(self.p) and self.p[self.i + 1] != ord("]"):
                self.i += 1
                c2, here2 = self.peek(), self.i
                self.i += 1
                hi = self.escape(here2, in_class=True) if c2 == ord("\\") else _byteset(c2)
                if lo.sum() != 1 or hi.sum() != 1 or int(np.argmax(hi)) < int(np.argmax(lo)):
                    self.fail("a bad character range", here)
                s[int(np.argmax(lo)):int(np.argmax(hi)) + 1] = True
            else:
                s |= lo
        return ~s if negate else s


class _Nfa:
    """A Thompson automaton: eps[i] the states behind state i's empty arcs, arc[i] its one (byte set, target) or None."""

    def __init__(self, limit):
        self.eps, self.arc, self.limit = [], [], limit

    def state(self):
        if len(self.eps) >= self.limit:
            raise ValueError("from_regex: the pattern's Thompson automaton alone passes 8 * max_states + 4096 states")
        self.eps.append([])
        self.arc.append(None)
        return len(self.eps) - 1

    def build(self, node):
        """(first, last) of a fragment for `node`."""
        kind = node[0]
        if kind == "set":
            a, b = self.state(), self.state()
            self.arc[a] = (node[1], b)
            return a, b
        if kind == "cat":
            a = b = self.state()
            for item in node[1]:
                f, l = self.build(item)
                self.eps[b].append(f)
                b = l
            return a, b
        if kind == "alt":
            a, b = self.state(), self.state()
            for item in node[1]:
                f, l = self.build(item)
                self.eps[a].append(f)
                self.eps[l].append(b)
            return a, b
        _, inner, m, n = node
        a = b = self.state()
        for _ in range(m):
            f, l = self.build(inner)
            self.eps[b].append(f)
            b = l
        end = self.state()
        if n is None:  # a loop: zero or more further copies
            f, l = self.build(inner)
            self.eps[b] += [f, end]
            self.eps[l] += [f, end]
        else:  # n - m optional copies in a row, each one's entry also the way out
            for _ in range(n - m):
                f, l = self.build(inner)
                self.eps[b] += [f, end]
                b = l
            self.eps[b].append(end)
        return a, end


def _regex_dfa(pattern, max_states):
    """(delta int32 [S, 256], accepting bool [S]) of `pattern` by subset construction, state 0 the start."""
    nfa = _Nfa(8 * max_states + 4096)
    first, last = nfa.build(_RegexParser(pattern).parse())
    n = len(nfa.eps)
    arcs = [i for i in range(n) if nfa.arc[i] is not None]

    def closure(i):
        """The states behind empty arcs from i that matter to a subset: those with a byte arc, and `last`."""
        seen, todo = {i}, [i]
        while todo:
            for v in nfa.eps[todo.pop()]:
                if v not in seen:
                    seen.add(v)
                    todo.append(v)
        return frozenset(v for v in seen if v == last or nfa.arc[v] is not None)

    # bytes that no arc's set tells apart move together: one representative each
    if arcs:
        sets = np.stack([nfa.arc[i][0] for i in arcs])
        _, rep, group = np.unique(sets, axis=1, return_index=True, return_inverse=True)
        group = np.asarray(group).reshape(-1)
    else:
        sets, rep, group = np.zeros((0, 256), np.bool_), np.zeros(1, np.int64), np.zeros(256, np.int64)
    by_arc = {i: (np.nonzero(sets[k][rep])[0].tolist(), closure(nfa.arc[i][1])) for k, i in enumerate(arcs)}
    start = closure(first)
    ids, order, rows = {start: 0}, [start], []
    k = 0
    while k < len(order):
        cur = order[k]
        k += 1
        nxt = [set() for _ in rep]
        for i in cur:
            if i in by_arc:
                groups, target = by_arc[i]
                for g in groups:
                    nxt[g] |= target
        row = []
        for t in nxt:
            t = frozenset(t)
            if t and t not in ids:
                if len(order) >= max_states:
                    raise ValueError(f"from_regex: the subset construction of {pattern!r} passes max_states={max_states}")
                ids[t] = len(order)
                order.append(t)
            row.append(ids[t] if t else -1)
        rows.append(row)
    delta = np.asarray(rows, np.int32).reshape(len(order), len(rep))[:, group]
    accepting = np.array([last in t for t in order], np.bool_)
    return np.ascontiguousarray(delta), accepting


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


# ---- minimisation (include/glb.h glb_dfa_refine / glb_dfa_quotient) -------------------------------------------------
_MIN_BATCH = 64  # rounds enqueued between two reads of the status words


def _minimize_on_device(eng, delta, keep, final_bits, arc_bits, arc_logw, final_logw, accepting, max_rounds):
    """Refinement and quotient of the tables on the device (`keep` a host bool [S], the others device tensors or None).
    Returns (new_id host int32 [S], outputs {"delta", "arc_logw", "final_logw", "accepting"} on the device, rounds).
    Quotient states are numbered by their smallest member, in increasing order: the class of state 0 is state 0."""
    import torch

    dev, S = eng.device, delta.shape[0]
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    slots = 1 << max(1, (2 * S - 1).bit_length())
    cls, scratch, table = i32(S), i32(S), torch.empty(slots * 12 // 8, dtype=torch.int64, device=dev)
    status = torch.zeros(_lib.DFA_MIN_STATUS, dtype=torch.int32, device=dev)
    keep_d = torch.from_numpy(np.ascontiguousarray(keep, dtype=np.uint8)).to(dev)
    p = _lib.DfaMinArgs()
    p.struct_size, p.n_states = C.sizeof(_lib.DfaMinArgs), S
    p.delta, p.keep, p.final_bits = delta.data_ptr(), keep_d.data_ptr(), final_bits.data_ptr()
    p.arc_bits = None if arc_bits is None else arc_bits.data_ptr()
    p.cls, p.scratch, p.table, p.table_slots, p.status = cls.data_ptr(), scratch.data_ptr(), table.data_ptr(), slots, status.data_ptr()
    p.restart = 1
    limit = S + 1 if max_rounds is None else int(max_rounds)
    rounds = converged = flags = 0
    while not converged and not flags and rounds < limit:
        p.rounds = min(_MIN_BATCH, limit - rounds)
        eng.dfa_call("glb_dfa_refine", p)
        p.restart = 0
        rounds, converged, flags = status[:3].tolist()
    if flags:
        raise RuntimeError(f"minimize: the refinement raised its flag word ({flags}: bit 0 - two different signatures shared a "
                           f"64-bit hash; bit 1 - a key found no slot) after {rounds} rounds; nothing was merged on that ground")
    if not converged:
        raise RuntimeError(f"minimize: the partition was still splitting after max_rounds={limit} rounds")
    c = cls.cpu().numpy()
    rep = np.unique(c[c >= 0]).astype(np.int32)
    new_id = np.where(c >= 0, np.searchsorted(rep, c), -1).astype(np.int32)
    n_new = len(rep)
    both = torch.from_numpy(np.concatenate([new_id, rep])).to(dev)  # (one upload)
    out = {"delta": i32(n_new, 256), "arc_logw": None, "final_logw": None, "accepting": None}
    p.new_id, p.rep, p.n_new, p.delta_out = both.data_ptr(), both.data_ptr() + 4 * S, n_new, out["delta"].data_ptr()
    if arc_logw is not None:
        out["arc_logw"] = torch.empty((n_new, 256), dtype=torch.float32, device=dev)
        out["final_logw"] = torch.empty(n_new, dtype=torch.float32, device=dev)
        p.arc_logw, p.final_logw = arc_logw.data_ptr(), final_logw.data_ptr()
        p.arc_out, p.final_out = out["arc_logw"].data_ptr(), out["final_logw"].data_ptr()
    out["accepting"] = torch.empty(n_new, dtype=torch.uint8, device=dev)
    p.accepting, p.accepting_out = accepting.data_ptr(), out["accepting"].data_ptr()
    eng.dfa_call("glb_dfa_quotient", p)
    return new_id, out, rounds


def _kept(automaton):
    """live & reachable, and the start state whatever it is: the quotient always has one."""
    keep = automaton.live & automaton.reachable
    keep[automaton.start] = True
    return keep


def _host_quotient(automaton, new_id, out):
    """The host automaton of the quotient tables, of `automaton`'s kind."""
    start = int(new_id[automaton.start])
    if isinstance(automaton, ByteWFSA):
        return ByteWFSA(out["delta"].cpu().numpy(), out["arc_logw"].cpu().numpy(), out["final_logw"].cpu().numpy(), start)
    return ByteDFA(out["delta"].cpu().numpy(), out["accepting"].cpu().numpy().astype(np.bool_), start)


def minimize(llm_or_engine, automaton, max_rounds=None):
    """(minimal, state_map): the smallest automaton that `automaton`'s labels allow, made on the device (include/glb.h
    glb_dfa_refine / glb_dfa_quotient), and int32 [S] - every state's state in it, -1 for the states dropped
    (those not live or not reachable from the start).  A `ByteDFA` gives the minimal `ByteDFA` of its language.  A
    `ByteWFSA` gives the quotient by the coarsest bisimulation on (byte, weight bits): states merge where their final
    weights and the weights of their arcs are equal bit for bit, so `path_logw` of every string is unchanged bit for bit;
    nothing is merged within a tolerance.  Quotient states are numbered in the order of their smallest members, so a start
    state 0 stays 0.  `max_rounds` (None: S + 1, which always suffices): RuntimeError when the partition still splits
    after that many rounds, or when the device reports a hash collision."""
    import torch

    if not isinstance(automaton, ByteDFA):
        raise ValueError("minimize needs a ByteDFA or a ByteWFSA")
    if max_rounds is not None and (isinstance(max_rounds, bool) or not isinstance(max_rounds, (int, np.integer)) or max_rounds < 1):
        raise ValueError(f"max_rounds must be None or an int >= 1, got {max_rounds!r}")
    eng = getattr(llm_or_engine, "engine", llm_or_engine)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    delta, acc = up(automaton.delta), up(automaton.accepting.astype(np.uint8))
    if isinstance(automaton, ByteWFSA):
        arc, fin = up(automaton.arc_logw), up(automaton.final_logw)
        new_id, out, _ = _minimize_on_device(eng, delta, _kept(automaton), fin, arc, arc, fin, acc, max_rounds)
    else:
        new_id, out, _ = _minimize_on_device(eng, delta, _kept(automaton), up(automaton.accepting.astype(np.int32)), None, None, None,
                                             acc, max_rounds)
    return _host_quotient(automaton, new_id, out), new_id


class DeviceConstraint:
    """A `ByteDFA` over a vocabulary's byte strings, resident on the device.

    llm_or_engine    an `AsyncAmdLM` (its engine and, for the default `skip_ids`, its tokenizer's `all_special_ids`) or a
                     `HipEngine`
    byte_vocab       the byte string of every token id (`llm.byte_vocab`); objects with a `byte_string` are accepted
    eos_id           allowed exactly in accepting states
    skip_ids         tokens never allowed (special tokens)
    mask_bank_bytes  budget of the mask bank: one row of ceil(V / 32) words per distinct state reached, plus two.  What
                     happens when a state a particle reaches finds the bank full is `on_full`'s to say.
    on_full          "error" (default): the state gets no row, its particles the empty mask, and `check()` raises.
                     "evict": the bank is a cache over the states (include/glb.h glb_dfa_evict_*) - a
                     `mask_rows` call recycles the least recently requested rows for the states that have none and fills
                     them again, all on the device; rows requested in the same call are never taken.  The bank then only has
                     to hold one step's working set: as many rows as the particles occupy distinct states, plus two
                     (`check()` raises when a single call asked for more).  A bank that holds every state (S + 2 rows)
                     never evicts and takes the path of "error".

    push             None (default): the automaton's weights are served as they are.  "log" / "max" (a `ByteWFSA` only): the
                     weights are pushed toward the start state on the device before anything is served (include/glb.h
                     glb_dfa_backward / glb_dfa_push_weights).  `backward` (float32 [S] device tensor) holds
                     beta[s], the semiring sum ("log": logsumexp, "max": the best) over all accepted byte strings from s;
                     every arc becomes arc + beta[next] - beta[s], every final weight final - beta[s].  An accepted
                     string then weighs what it weighed minus `start_logw` = beta[start], but every state's row carries
                     the look-ahead: a particle sees the weight of a branch when it enters it, not at EOS.  `DeviceSIS`
                     starts its particles at `start_logw`; `push_stats()`, `pushed_wfsa()` are for inspection.
    push_tol         "log": the sweeps stop when no state moved by more than push_tol * max(1, |beta|); the default 2^-20 is
                     four float32 ulps, above the one-ulp oscillation of a converged float32 iteration.
    push_max_sweeps  ValueError when the backward weights have not converged after this many sweeps (or, under "max",
                     after S + 1): the weights do not sum - a cycle of total mass >= 1 under "log".

    minimize         False (default): the automaton is served as it is.  True: equivalent states are merged on the device
                     before anything is served (include/glb.h glb_dfa_refine / glb_dfa_quotient) - after the
                     push, if any, on the tables the push left.  The constraint then serves the quotient: `dfa` is the
                     quotient's host automaton (with a push: carrying the pushed weights), and `n_states`, `start`, `live`,
                     the bank's rows, `warm()`, eviction and `pushed_wfsa()` are the quotient's.  `source_dfa` is what
                     the caller passed, `state_map` (int32 [S] device tensor) every source state's quotient state, -1 for
                     the states dropped (not live, or not reachable from the start); `minimize_stats()`.  States and
                     the ids `advance` returns are the quotient's.  `start_logw` and `backward` keep their meaning;
                     `backward` stays indexed by the SOURCE automaton's states.  A `ByteWFSA` merges states whose weights
                     are equal bit for bit (after a push: what weighted minimisation merges, where rounding left equal
                     bits); every string weighs what it weighed, bit for bit.

    Lifetime of row ids: the ids a `mask_rows` call returns are valid until the next `mask_rows` / `warm` call on this
    constraint - under "evict" that call may hand their rows to other states.  Stream order makes this safe for `DeviceSIS`
    and `batch_next_token_step_device`: each makes one `mask_rows` call a step and enqueues the step that reads the ids
    before the next one.

    With a `ByteWFSA` the bank holds float32 rows [rows, ld] instead (ld: V rounded up to 64 floats), the token log-weights
    from each state (include/glb.h glb_dfa_weight_*): rows = min(S + 2, 65535, mask_bank_bytes / (4 ld)).  A row is 32 times
    a bit row - about 201 KB at V = 50257, so the default 256 MiB hold 1332 states.  `step_masks` then hands the bank over
    as `MASK_F32` in either form of the step; everything else keeps its meaning.
    """

    def __init__(self, llm_or_engine, dfa, byte_vocab, eos_id, skip_ids=None, mask_bank_bytes=256 << 20, on_full="error",
                 push=None, push_tol=2.0 ** -20, push_max_sweeps=4096, minimize=False):
        if on_full not in ("error", "evict"):
            raise ValueError(f'on_full must be "error" or "evict", got {on_full!r}')
        if push not in (None, "log", "max"):
            raise ValueError(f'push must be None, "log" or "max", got {push!r}')
        if push is not None:
            if not isinstance(dfa, ByteWFSA):
                raise ValueError(f"push={push!r} needs a ByteWFSA: a ByteDFA has no weights to push")
            if not float(push_tol) >= 0.0:
                raise ValueError(f"push_tol must be >= 0, got {push_tol!r}")
            if isinstance(push_max_sweeps, bool) or not isinstance(push_max_sweeps, (int, np.integer)) or push_max_sweeps < 1:
                raise ValueError(f"push_max_sweeps must be an int >= 1, got {push_max_sweeps!r}")
        if not isinstance(minimize, bool):
            raise ValueError(f"minimize must be True or False, got {minimize!r}")
        import torch

        self.on_full = on_full
        eng = getattr(llm_or_engine, "engine", llm_or_engine)
        self.eng, self.dev, self.dfa = eng, eng.device, dfa
        toks = [bytes(getattr(t, "byte_string", t)) for t in byte_vocab]
        V = len(toks)
        if V == 0:
            raise ValueError("empty vocabulary")
        if skip_ids is None:
            skip_ids = getattr(getattr(llm_or_engine, "tokenizer", None), "all_special_ids", None) or ()
        skip = np.zeros(V, np.uint8)
        for t in skip_ids:
            if 0 <= int(t) < V:
                skip[int(t)] = 1
        ptr = np.zeros(V + 1, np.int64)
        np.cumsum([len(t) for t in toks], out=ptr[1:])
        if ptr[-1] > 0x7fffffff:
            raise ValueError("the vocabulary's byte strings exceed 2^31 bytes")
        flat = np.frombuffer(b"".join(toks) or b"\0", np.uint8).copy()
        self.vocab, self.eos_id, self.words = V, int(eos_id), (V + 31) // 32
        self.n_bytes = int(ptr[-1])
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self._delta, self._acc, self._live = up(dfa.delta), up(dfa.accepting.astype(np.uint8)), up(dfa.live.astype(np.uint8))
        self._bytes, self._ptr, self._skip = up(flat), up(ptr.astype(np.int32)), up(skip)
        self.mask_bank_bytes = int(mask_bank_bytes)
        self._gathered, self._cus = None, None
        self.weighted = isinstance(dfa, ByteWFSA)
        if self.weighted:
            self._arc_logw, self._final_logw = up(dfa.arc_logw), up(dfa.final_logw)
        self.push, self.backward, self.start_logw, self._push_sweeps = push, None, 0.0, 0
        if push is not None:
            self._push_weights(float(push_tol), int(push_max_sweeps))
        self.source_dfa, self.state_map, self._min_rounds = dfa, None, 0
        if minimize:
            dfa = self._minimize()
        # The bank's kind, decided here once: a row's elements (bit words, or with weights the floats of a 256-byte aligned row),
        # how many of them a caller's bank needs, the step's mask kind, the library's calls and the argument block they take
        (self._bank_dtype, self.row_elems, self._row_need, self._mask_kind, bank_rows, self._init, self._fill, self._bank_args) = \
            (torch.float32, (V + 63) // 64 * 64, V, _lib.MASK_F32, eng.lib.glb_dfa_weight_bank_rows, "glb_dfa_weight_bank_init",
             "glb_dfa_fill_weights", self._weight_args) if self.weighted else \
            (torch.int32, self.words, self.words, _lib.MASK_BITS, eng.lib.glb_dfa_bank_rows, "glb_dfa_bank_init",
             "glb_dfa_fill_masks", lambda a: a)
        rows = int(bank_rows(self.mask_bank_bytes, V, dfa.n_states))
        if rows < 3:
            raise ValueError(f"mask_bank_bytes={mask_bank_bytes} holds no state's mask: a row of this vocabulary takes "
                             f"{self.row_elems * 4} bytes{' (float32 weights: 32 times a bit row)' if self.weighted else ''} "
                             "and the bank needs at least three")
        self._row_of_state = torch.empty(dfa.n_states, dtype=torch.int32, device=self.dev)
        self._counters = torch.zeros(_lib.DFA_COUNTERS, dtype=torch.int32, device=self.dev)
        self._set_bank(torch.zeros((rows, self.row_elems), dtype=self._bank_dtype, device=self.dev))

    # ---- weight pushing ------------------------------------------------------------------------------------------------
    _PUSH_BATCH = 64  # sweeps enqueued between two reads of the status words

    def _push_weights(self, tol, max_sweeps):
        """Backward weights by Jacobi sweeps on the device (glb_dfa_backward, in batches; the stop rule is the device's, the
        host reads three words a batch), then the automaton reweighted by them (glb_dfa_push_weights): `_arc_logw` /
        `_final_logw` become the pushed tables, everything downstream serves them as it serves any `ByteWFSA`."""
        import torch

        S = self.dfa.n_states
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.dev)
        beta, scratch, arc_out, final_out = f32(S), f32(S), f32(S, 256), f32(S)
        status = torch.zeros(_lib.DFA_PUSH_STATUS, dtype=torch.int32, device=self.dev)
        p = _lib.DfaPushArgs()
        p.struct_size = C.sizeof(_lib.DfaPushArgs)
        p.n_states, p.start = S, self.dfa.start
        p.semiring = _lib.DFA_PUSH_LOG if self.push == "log" else _lib.DFA_PUSH_MAX
        p.delta, p.arc_logw, p.final_logw = self._delta.data_ptr(), self._arc_logw.data_ptr(), self._final_logw.data_ptr()
        p.beta, p.scratch, p.arc_out, p.final_out = beta.data_ptr(), scratch.data_ptr(), arc_out.data_ptr(), final_out.data_ptr()
        p.status, p.tol, p.restart = status.data_ptr(), tol, 1
        sweeps = converged = flags = 0
        while not converged and not flags and sweeps < max_sweeps and not (self.push == "max" and sweeps > S + 1):
            p.sweeps = min(self._PUSH_BATCH, max_sweeps - sweeps)
            self._call("glb_dfa_backward", p)
            p.restart = 0
            sweeps, converged, flags = status[:3].tolist()
        if flags or not converged or (self.push == "max" and sweeps > S + 1):
            raise ValueError(f"the automaton's weights do not sum: the backward weights "
                             f"{'overflowed' if flags else 'had not converged'} after {sweeps} sweeps under push={self.push!r} "
                             '(under "log": a cycle of total mass >= 1; under "max": a cycle of positive weight).  '
                             'push="max" needs only that no cycle gains weight; push=None serves the weights as they are.')
        p.sweeps = 1
        self._call("glb_dfa_push_weights", p)
        self._arc_logw, self._final_logw, self.backward, self._push_sweeps = arc_out, final_out, beta, sweeps
        self.start_logw = float(beta[self.dfa.start].item())

    def _minimize(self):
        """The tables on the device (`_delta`, and with weights `_arc_logw` / `_final_logw` as the push left them) replaced
        by their quotient's; returns the quotient's host automaton, which becomes `dfa`."""
        import torch

        src = self.source_dfa
        keep = _kept(src)
        if self.weighted:
            new_id, out, rounds = _minimize_on_device(self.eng, self._delta, keep, self._final_logw, self._arc_logw, self._arc_logw,
                                                      self._final_logw, self._acc, None)
            self._arc_logw, self._final_logw = out["arc_logw"], out["final_logw"]
        else:
            new_id, out, rounds = _minimize_on_device(self.eng, self._delta, keep, self._acc.to(torch.int32), None, None, None,
                                                      self._acc, None)
        self._delta, self._acc = out["delta"], out["accepting"]
        self.dfa = _host_quotient(src, new_id, out)
        self._live = torch.from_numpy(self.dfa.live.astype(np.uint8)).to(self.dev)
        self.state_map, self._min_rounds = torch.from_numpy(new_id).to(self.dev), rounds
        return self.dfa

    def minimize_stats(self):
        """{"states_in", "states_out", "rounds"}: the source automaton's states, the states served, and the refinement
        rounds taken, the one that found nothing to split included (0: nothing was minimised)."""
        return {"states_in": self.source_dfa.n_states, "states_out": self.dfa.n_states, "rounds": self._min_rounds}

    def push_stats(self):
        """{"semiring", "sweeps"}: what `push` was (None: nothing pushed) and the Jacobi sweeps the backward weights took,
        the one that found nothing moving included."""
        return {"semiring": self.push, "sweeps": self._push_sweeps}

    def pushed_wfsa(self):
        """A host `ByteWFSA` of the weights this constraint serves (the pushed ones; under push=None the automaton's own),
        for inspection: the arcs into states that are not live weigh -inf and are gone from its `delta` (copies the tables
        from the device)."""
        if not self.weighted:
            raise ValueError("a ByteDFA has no weights")
        return ByteWFSA(self.dfa.delta, self._arc_logw.cpu().numpy(), self._final_logw.cpu().numpy(), self.dfa.start)

    # ---- the bank ------------------------------------------------------------------------------------------------------
    def _set_bank(self, bank):
        """Use `bank` (int32 [rows, >= ceil(V / 32)], with weights float32 [rows, >= V]; unit inner stride; rows may be
        padded) and start it over."""
        import torch

        if bank.dtype != self._bank_dtype or bank.dim() != 2 or bank.stride(1) != 1 or bank.shape[0] < 3 or bank.shape[1] < self._row_need \
                or bank.device != self.dev:
            raise ValueError("bank must be an int32 [rows >= 3, >= ceil(V / 32)] (with weights: float32 [rows >= 3, >= V]) "
                             "device tensor with unit inner stride")
        self.bank = bank
        self._work = torch.zeros((bank.shape[0], 2), dtype=torch.int32, device=self.dev)
        # a bank that cannot hold every state, allowed to evict: the tables of glb_dfa_evict_args, one allocation
        self._evicting = self.on_full == "evict" and self.dfa.n_states + 2 > bank.shape[0]
        self._evict_tables = torch.zeros(4 * bank.shape[0] + _lib.DFA_EVICT_COUNTERS + 1, dtype=torch.int32, device=self.dev) \
            if self._evicting else None
        self._reset_bank()

    def _reset_bank(self):
        """Forget every state's row (rows 0 and 1 are written again, the overflow word cleared)."""
        self._warm = False
        if self._evicting:
            self._call("glb_dfa_evict_bank_init", self._evict_args(self._args()))
        else:
            self._call(self._init, self._bank_args(self._args()))

    capacity = property(lambda self: self.bank.shape[0])

    def _args(self):
        a = _lib.DfaArgs()
        a.struct_size = C.sizeof(_lib.DfaArgs)
        a.n_states, a.start, a.eos_id = self.dfa.n_states, self.dfa.start, self.eos_id
        a.delta, a.accepting, a.live = self._delta.data_ptr(), self._acc.data_ptr(), self._live.data_ptr()
        a.vocab, a.tok_bytes, a.n_bytes = self.vocab, self._bytes.data_ptr(), self.n_bytes
        a.tok_ptr, a.skip = self._ptr.data_ptr(), self._skip.data_ptr()
        a.bank, a.bank_ld, a.capacity = self.bank.data_ptr(), self.bank.stride(0), self.bank.shape[0]
        a.row_of_state, a.work, a.counters = self._row_of_state.data_ptr(), self._work.data_ptr(), self._counters.data_ptr()
        return a

    def _weight_args(self, a):
        """The block of glb_dfa_weight_bank_init / glb_dfa_fill_weights round `a`."""
        w = _lib.DfaWeightArgs()
        w.struct_size, w.dfa = C.sizeof(_lib.DfaWeightArgs), a
        w.arc_logw, w.final_logw = self._arc_logw.data_ptr(), self._final_logw.data_ptr()
        w.wbank, w.wbank_ld = self.bank.data_ptr(), self.bank.stride(0)
        return w

    def _evict_args(self, a):
        """The block of glb_dfa_evict_bank_init / glb_dfa_evict_serve round `a`, for either kind of bank."""
        e = _lib.DfaEvictArgs()
        e.struct_size, e.dfa = C.sizeof(_lib.DfaEvictArgs), a
        if self.weighted:
            e.arc_logw, e.final_logw = self._arc_logw.data_ptr(), self._final_logw.data_ptr()
            e.wbank, e.wbank_ld = self.bank.data_ptr(), self.bank.stride(0)
        cap, base = self.capacity, self._evict_tables.data_ptr()
        e.row_state, e.row_stamp, e.claimants, e.victims = (base + 4 * cap * i for i in range(4))
        e.ecounters = base + 16 * cap
        e.epoch = e.ecounters + 4 * _lib.DFA_EVICT_COUNTERS
        return e

    def _call(self, name, a):
        self.eng.dfa_call(name, a)

    def _states(self, states):
        import torch

        if states.dtype != torch.int32 or states.dim() != 1 or states.device != self.dev or not states.is_contiguous():
            raise ValueError("states must be a contiguous int32 [n] tensor on the engine's device")
        return states

    # ---- states --------------------------------------------------------------------------------------------------------
    def states0(self, n):
        import torch

        return torch.full((n,), self.dfa.start, dtype=torch.int32, device=self.dev)

    def advance(self, states, tokens, frm, to, out=None):
        """The states after tokens[i, frm[i] .. to[i]) (int32 [n, ld], unit inner stride), from states[i] (None: the start
        state); -1 once dead.  One launch (glb_dfa_advance)."""
        import torch

        if tokens.dtype != torch.int32 or tokens.dim() != 2 or tokens.device != self.dev:
            raise ValueError("tokens must be an int32 [n, ld] tensor on the engine's device")
        tokens = tokens.contiguous()
        n = tokens.shape[0]
        if out is None:
            out = torch.empty(n, dtype=torch.int32, device=self.dev)
        if n == 0:
            return out
        for t in (frm, to):
            if t.dtype != torch.int32 or t.shape != (n,) or t.device != self.dev or not t.is_contiguous():
                raise ValueError("frm / to must be contiguous int32 [n] tensors on the engine's device")
        a = self._args()
        a.n, a.tokens, a.ld = n, tokens.data_ptr(), tokens.shape[1]
        if tokens.shape[1] == 0:  # nothing to walk: from == to == 0 is the only range inside
            a.tokens, a.ld = self._ptr.data_ptr(), 1
            to = torch.minimum(to, frm)
        a.from_, a.to = frm.data_ptr(), to.data_ptr()
        a.state_in = None if states is None else self._states(states).data_ptr()
        a.state_out = out.data_ptr()
        self._call("glb_dfa_advance", a)
        return out

    def _claim_and_fill(self, states):
        """Every state of `states` that has no bank row yet gets one, and the new rows are filled (two launches)."""
        n = states.numel()
        if n == 0:
            return
        a = self._args()
        a.n, a.state_in = n, self._states(states).data_ptr()
        self._call("glb_dfa_claim_rows", a)
        a.max_work = min(n, self.dfa.n_states, self.capacity)
        self._call(self._fill, self._bank_args(a))

    def mask_rows(self, states, done=None):
        """int32 [n]: the bank row of every state - 0 (nothing allowed) for a dead one; where `done` (int32 [n]) is set, row
        1 (EOS only) if the state is accepting, else 0.  Claims and fills what is missing first - under on_full="evict" in
        a bank smaller than the automaton, in rows taken from the states requested longest ago; no host synchronisation.
        The ids are valid until the next `mask_rows` / `warm` call on this constraint."""
        import torch

        n = states.numel()
        out = torch.empty(n, dtype=torch.int32, device=self.dev)
        if n == 0:
            return out
        if not self._warm and not self._evicting:
            self._claim_and_fill(states)
        a = self._args()
        a.n, a.state_in, a.out_rows = n, self._states(states).data_ptr(), out.data_ptr()
        if done is not None:
            if done.dtype != torch.int32 or done.shape != (n,) or not done.is_contiguous() or done.device != self.dev:
                raise ValueError("done must be a contiguous int32 [n] tensor on the engine's device")
            a.done = done.data_ptr()
        if self._evicting:  # touch, select, fill and ids in one call: rows are recycled for the states that have none
            a.max_work = min(n, self.dfa.n_states, self.capacity - 2)
            self._call("glb_dfa_evict_serve", self._evict_args(a))
        else:
            self._call("glb_dfa_mask_ids", a)
        return out

    def step_masks(self, logits, ids, by_row, n_particles, parity=False):
        """The fused step's mask arguments (masks.py; `logits` is not read) for bank rows `ids` (int32 [n_units]: per logits
        row when `by_row`, else per particle), and whether the bank itself is handed over.  `GLB_MASK_BITS` rows are read as they are only by the
        step's one-launch form; its two-launch form first brings ALL rows of the table it is given into the kernels'
        layout.  So the bank is handed over where glb_logprob_mask_sample takes the one-launch form (csrc/glb_api.hip,
        `fused`: no parity draw, more than 512 (unit, 4096-token chunk) items, at most 16 x 8 x CUs particles), and
        otherwise only the units' rows, gathered into a buffer of this object.  This is the one place the rule is
        restated; where it guesses wrong (a stream being captured, a workspace nobody registered) the step still computes
        the same results from the whole bank, only slower.
        A weight bank (`GLB_MASK_F32`) is read where it lies by both forms: always handed over, nothing gathered."""
        import torch

        key = "row_mask_id" if by_row else "mask_id"
        n_units = ids.numel()
        if self._cus is None:
            self._cus = torch.cuda.get_device_properties(self.dev).multi_processor_count
        if self.weighted or (not parity and n_units * ((self.vocab + 4095) // 4096) > 512 and n_particles <= 16 * 8 * self._cus):
            return {"mask_kind": self._mask_kind, "mask": self.bank, key: ids}, True
        if self._gathered is None or self._gathered[0].shape[0] != n_units:
            self._gathered = (torch.empty((n_units, self.words), dtype=torch.int32, device=self.dev),
                              torch.arange(n_units, dtype=torch.int32, device=self.dev))
        buf, own = self._gathered
        self.eng.gather_rows_i32(self.bank[:, :self.words], ids, out=buf)
        return {"mask_kind": _lib.MASK_BITS, "mask": buf, key: own}, False

    def forced_final_logw(self, states, forced):
        """float32 [n]: final_logw[states[i]] where `forced` (bool [n]: the particle was served row 1 and ended) and 0.0
        elsewhere - what a caller adds to the log-weight of a particle made to end, so that it weighs what one that chose
        EOS from its state's own row does.  One gather, one select; no synchronisation."""
        import torch

        fw = self._final_logw[states.clamp(min=0).long()]
        return torch.where(forced & (states >= 0), fw, torch.zeros_like(fw))

    def warm(self):
        """Fill the rows of ALL states when the bank holds them (later `mask_rows` calls are then one small launch).
        Returns whether it did."""
        import torch

        if self.dfa.n_states + 2 > self.capacity:
            return False
        if not self._warm:
            self._claim_and_fill(torch.arange(self.dfa.n_states, dtype=torch.int32, device=self.dev))
            self._warm = True
        return True

    def _overflow_word(self):
        """int32 [1] device view of the sticky overflow word, for hosts that let it ride on a copy they make anyway."""
        return self._counters[2:3]

    def _rows_in_use(self):
        """(synchronises)"""
        return int(self._counters[0].item())

    def stats(self):
        """{"rows_in_use", "fills", "evictions"}: the bank's rows that hold something (its own two included), the rows
        filled so far and how many of those were taken from another state (synchronises)."""
        rows, filled = self._counters[:2].tolist()
        if not self._evicting:
            return {"rows_in_use": rows, "fills": filled, "evictions": 0}
        fills, evictions = self._evict_tables[4 * self.capacity + 2:4 * self.capacity + 4].tolist()
        return {"rows_in_use": rows, "fills": fills, "evictions": evictions}

    def check(self, word=None):
        """Raises when a state found no row in the bank (synchronises unless `word`, the overflow word's value already on
        the host, is given).  Under eviction that is: one call asked for more distinct states than the bank has rows."""
        if not (int(self._counters[2].item()) if word is None else int(word)):
            return
        if self._evicting:
            raise RuntimeError(f"the constraint's mask bank is smaller than one step's working set: a single mask_rows call "
                               f"asked for more distinct automaton states than its {self.capacity - 2} rows for states "
                               f"({self.capacity} rows of {self.row_elems * 4} bytes, mask_bank_bytes={self.mask_bank_bytes}); "
                               "the states left over were served the empty mask.  The bank must hold at least as many rows "
                               "as the particles occupy distinct states, plus two.  Raise mask_bank_bytes.")
        raise RuntimeError(f"the constraint's mask bank is full: {self.capacity} rows of {self.row_elems * 4} bytes "
                           f"(mask_bank_bytes={self.mask_bank_bytes}) do not hold the automaton states the particles "
                           "reached; their masks were empty.  Raise mask_bank_bytes.")
