"""A plain restatement of the token -> byte trie masses, for tests: NumPy over `TokenByteTrie.flat()`, written from the
operation's definition and independent of oracle/glb_oracle.c (tests/test_trie_ref_cpu.py holds the two against each
other bit for bit, and this one against the reference's recorded numbers).

  leaves           the row's value of the leaf's token
  internal nodes   in the trie's level order (`level_nodes`: a node comes after all of its children), the float64 sum of
                   its children taken in ascending child order from +0.0 - or the maximum from +0.0, where a child
                   replaces the running value only if it is GREATER (a NaN never is, neither is a negative or -0.0) -
                   stored as float32

The children of the k-th position of all nodes of a level are added in one NumPy operation; every node still sees its own
children one after the other in ascending order, which is all the float64 additions depend on.
"""
import numpy as np


class TrieRef:
    def __init__(self, flat):
        self.n_nodes = int(flat["n_nodes"])
        self.vocab = int(flat["vocab"])
        self.leaf_node = np.asarray(flat["leaf_node"], np.int64)
        cp = np.asarray(flat["child_ptr"], np.int64)
        ci = np.asarray(flat["child_idx"], np.int64)
        ls = np.asarray(flat["level_start"], np.int64)
        order = np.asarray(flat["level_nodes"], np.int64)
        self.parent = np.full(self.n_nodes, -1, np.int64)
        self.parent[ci] = np.repeat(np.arange(self.n_nodes), np.diff(cp))
        self.internal = order
        inside = np.ones(max(len(ci) - 1, 0), bool)  # pairs of neighbours in child_idx that belong to one node
        ends = cp[1:-1]
        inside[ends[(ends > 0) & (ends < len(ci))] - 1] = False
        assert (np.diff(ci)[inside] > 0).all(), "children must be listed in ascending order"
        # per level: for k = 0, 1, ...: (nodes with more than k children, their k-th child)
        self.levels = []
        for d in range(len(ls) - 1):
            nodes = order[ls[d]:ls[d + 1]]
            cnt = cp[nodes + 1] - cp[nodes]
            steps = []
            for k in range(int(cnt.max()) if len(nodes) else 0):
                has = cnt > k
                steps.append((nodes[has], ci[cp[nodes[has]] + k]))
            self.levels.append((nodes, steps, nodes[cnt == 1], ci[cp[nodes[cnt == 1]]]))
        self.n_children = np.diff(cp)

    def reduce(self, ws, op=0, folded=False):
        """ws: [B, V] float32 leaf values in token order -> float32 [B, n_nodes] (op 0: sum, 1: max).
        folded: what the kernels over the FOLDED trie (`TokenByteTrie.compact()`, every plan of glb_trie_rows) give: a node
        with exactly one child has no value of its own and shows its child's, as it is.  For weights that are +0.0 or
        greater - every weight a softmax or a mask produces - that is the sum and the maximum of one term bit for bit; a
        -0.0, a negative or a NaN child shows where the unfolded reduction gives +0.0 (sum of -0.0; max of a negative or a
        NaN).  Nodes with two children and more reduce from +0.0 either way."""
        ws = np.asarray(ws)
        assert ws.dtype == np.float32 and ws.ndim == 2 and ws.shape[1] == self.vocab
        out = np.zeros((ws.shape[0], self.n_nodes), np.float32)
        out[:, self.leaf_node] = ws
        with np.errstate(over="ignore", invalid="ignore"):
            for nodes, steps, one, one_kid in self.levels:
                acc = np.zeros((ws.shape[0], len(nodes)), np.float64)
                pos = np.full(self.n_nodes, -1, np.int64)
                pos[nodes] = np.arange(len(nodes))
                for par, kid in steps:
                    v = out[:, kid].astype(np.float64)
                    at = pos[par]
                    if op == 0:
                        acc[:, at] = acc[:, at] + v
                    else:
                        cur = acc[:, at]
                        acc[:, at] = np.where(v > cur, v, cur)
                out[:, nodes] = acc.astype(np.float32)
                if folded:
                    out[:, one] = out[:, one_kid]
        return out

    def chain(self, leaf):
        """The one-child nodes between `leaf` and its first ancestor with two children and more: the nodes that share the
        leaf's slot in the folded trie."""
        up = []
        for x in self.ancestors(leaf):
            if self.n_children[x] != 1:
                break
            up.append(x)
        return up

    def ancestors(self, leaf):
        """The nodes strictly above `leaf` (any node id), nearest first, the root last."""
        up, x = [], int(self.parent[int(leaf)])
        while x >= 0:
            up.append(x)
            x = int(self.parent[x])
        return up


def reduce(flat, ws, op=0):
    """`TrieRef(flat).reduce(ws, op)` for a single use."""
    return TrieRef(flat).reduce(ws, op)


def leaves_from_logits(x, scale, lse):
    """exp(x * scale - lse[r]) in float64: x [B, V] (any float type, upcast exactly), lse [B]."""
    x = np.asarray(x).astype(np.float64)
    lse = np.asarray(lse).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.exp(x * float(scale) - lse[:, None])


def same_bits(a, b):
    """float32 arrays equal bit for bit, NaNs by position (not by payload)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def first_difference(a, b):
    """For failure messages: (row, column, a, b) of the first element where `same_bits` fails, or None."""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    bad = (na != nb) | (~(na | nb) & (a.view(np.uint32) != b.view(np.uint32)))
    if not bad.any():
        return None
    r, c = np.argwhere(bad)[0]
    return int(r), int(c), float(a[r, c]), float(b[r, c]), int(bad.sum())


# ---- inputs the trie tests share ---------------------------------------------------------------------------------------
def synthetic_vocab(seed, n, letters, max_len, skew=0.0):
    """`n` distinct byte strings of 1 .. max_len of the first `letters` lowercase letters, in the order drawn.  skew > 0:
    letter i is drawn with probability ~ (1 + i) ** -skew, which gives nodes of very different widths."""
    rs = np.random.default_rng(seed)
    words, seen = [], set()
    p = (1.0 + np.arange(letters)) ** -float(skew)
    p /= p.sum()
    while len(words) < n:
        if skew:
            w = bytes((97 + rs.choice(letters, int(rs.integers(1, max_len + 1)), p=p)).astype(np.uint8))
        else:
            w = bytes(rs.integers(97, 97 + letters, int(rs.integers(1, max_len + 1))).astype(np.uint8))
        if w not in seen:
            seen.add(w)
            words.append(w)
    return words


def palette(kind="float32"):
    """The hostile values, as float32 that the element type `kind` ("float32" / "bfloat16" / "float16") holds exactly:
    name -> value.  `tiny` is the type's smallest subnormal, `min_normal` its FLT_MIN, `big` its largest finite value."""
    tiny, min_normal, big = {"float32": (2.0 ** -149, 2.0 ** -126, float(np.finfo(np.float32).max)),
                             "bfloat16": (2.0 ** -133, 2.0 ** -126, float(np.uint32(0x7f7f0000).view(np.float32))),
                             "float16": (2.0 ** -24, 2.0 ** -14, 65504.0)}[kind]
    return {"+0": np.float32(0.0), "-0": np.float32(-0.0), "tiny": np.float32(tiny), "min_normal": np.float32(min_normal),
            "one": np.float32(1.0), "big": np.float32(big), "+inf": np.float32(np.inf), "-inf": np.float32(-np.inf),
            "nan": np.float32(np.nan), "negative": np.float32(-0.375)}


def nested_pair(words, skip=0):
    """Two tokens (i, j) with words[j] = words[i] + one byte: both leaves lie below the node of words[i] (a node has one
    leaf of its own at most), so two of the largest finite value there overflow that node's float32 store.  None when
    the vocabulary has no such pair; `skip`: take the skip-th pair."""
    index = {w: i for i, w in enumerate(words)}
    for j, w in enumerate(words):
        i = index.get(w[:-1])
        if i is not None and len(w) > 1:
            if skip == 0:
                return i, j
            skip -= 1
    return None


def round_to(x, kind):
    """float32 values rounded (to nearest even) to what the element type `kind` holds, as float32."""
    x = np.ascontiguousarray(x, np.float32)
    if kind == "float16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(np.float32)
    if kind == "bfloat16":
        u = x.view(np.uint32)
        return ((u + (((u >> 16) & 1) + 0x7FFF)) & np.uint32(0xFFFF0000)).view(np.float32)
    return x.copy()


def hostile_rows(words, kind, n_rows, seed, places=None):
    """Weight rows for the hostile-value tests: float32 [n_rows, V] of values `kind` holds exactly, mostly uniform(0, 1)
    with a handful of palette values placed deliberately, and what was placed: a dict with
      "nan"      [(row, token)]: rows that carry a single NaN and nothing else unusual
      "clean"    rows of plain uniform values (the neighbours of the single-NaN rows)
      "negative" the row of all negatives, "minus_zero" the row of all -0.0, "tiny" the row of all smallest subnormals
      "big"      (row, token i, token j): the type's largest finite value twice under the node of token i
      "inf"      [(row, token, sign)]: rows with a single infinity
    places: name -> token (the first and the last token are always there).  The deliberate rows come first, the most
    telling ones among the first nine; rows past them are uniform with every palette value sprinkled in at random tokens
    (NaN and the infinities in one row in three).  The same arguments always give the same rows."""
    rs = np.random.default_rng(seed)
    V = len(words)
    pal = palette(kind)
    places = dict(places or {})
    places.setdefault("first", 0)
    places.setdefault("last", V - 1)
    toks = list(dict.fromkeys(int(t) for t in places.values()))  # (distinct, in order)
    uniform = lambda: round_to(rs.random(V).astype(np.float32), kind)
    rows, info = [], {"nan": [], "clean": [], "inf": []}

    def add(row):
        rows.append(row)
        return len(rows) - 1

    # 0: a bit of everything at the named places and at random tokens (the row a batch of one gets)
    mix = uniform()
    names = list(pal)
    for n, t in enumerate(toks + [int(t) for t in rs.choice(V, min(V, 2 * len(names)), replace=False)]):
        mix[t] = pal[names[n % len(names)]]
    add(mix)
    # 1 .. : a single NaN at each place, a clean row between any two of them
    def single_nan(t):
        row = uniform()
        row[t] = pal["nan"]
        info["nan"].append((add(row), t))
        info["clean"].append(add(uniform()))

    for t in toks[:2]:
        single_nan(t)
    # (among the first nine rows: the rows of whole-row properties)
    info["negative"] = add(round_to(-uniform() - np.float32(0.5), kind))
    info["minus_zero"] = add(np.full(V, -0.0, np.float32))
    info["tiny"] = add(np.full(V, pal["tiny"], np.float32))
    pair = nested_pair(words)
    if pair is not None:
        row = uniform()
        row[list(pair)] = pal["big"]
        info["big"] = (add(row), pair[0], pair[1])
    for t in toks[2:]:
        single_nan(t)
    for t in toks:
        for sign in ("+inf", "-inf"):
            row = uniform()
            row[t] = pal[sign]
            info["inf"].append((add(row), t, sign))
    assert len(rows) <= n_rows or n_rows in (1, 9), (len(rows), n_rows)
    k = 0
    while len(rows) < n_rows:
        row = uniform()
        pick = rs.choice(V, min(V, len(names)), replace=False)
        for n, t in zip(names, pick):
            if k % 3 == 0 or n not in ("nan", "+inf", "-inf"):
                row[t] = pal[n]
        add(row)
        k += 1
    out = np.stack(rows[:n_rows])
    assert np.array_equal(np.isnan(out), np.isnan(round_to(out, kind))) and same_bits(out, round_to(out, kind)), "not exact in " + kind
    return out, info
