"""`ByteDFA.from_regex`'s compiler: a parser, a Thompson automaton, its subset construction.  NumPy only."""
import numpy as np

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


def _thompson(pattern, max_states):
    """(automaton, first, last): the Thompson automaton of `pattern`, what `_regex_dfa` and `ByteNFA.from_regex` both start from."""
    nfa = _Nfa(8 * max_states + 4096)
    first, last = nfa.build(_RegexParser(pattern).parse())
    return nfa, first, last


def _regex_dfa(pattern, max_states):
    """(delta int32 [S, 256], accepting bool [S]) of `pattern` by subset construction, state 0 the start."""
    nfa, first, last = _thompson(pattern, max_states)
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
