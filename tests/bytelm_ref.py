"""float64 restatement of the byte-level beam (`genlm_backend_amd.bytelm.ByteBeam`, glb_bytelm_*), written from
the contract, dict-based, one group at a time.

A beam is at most `width` candidates in slots that never move, each a dict(x=committed tokens, n=node, u=log-probability of
x, w=u + log M_x[n]).  A node is any hashable: here the bytes read since the last committed token (b"" is the root); the
GPU tests use the device's node ids instead.  The three steps take the candidates and, per slot, the tables the device reads:

    tables[slot] = (bytes_tbl, leaves_tbl)
    bytes_tbl    {byte: (child node, mass of the child)}
    leaves_tbl   [(token, mass)] for the node's leaf children in token order (ignored tokens left out); at the root: the EOS

so the same code runs on float64 masses of a host model (`RefBeam`) and on the masses a device computed."""
import math
import zlib

import numpy as np

EOS = 256
NINF = float("-inf")


def extend_group(cands, tables, width, root, fresh=True):
    """Step 1.  Returns (new candidates, parent per slot, token per slot, gap, number of entries that competed): parent = the slot itself for a kept candidate,
    the offering slot for a spawned one, -1 for an empty slot; gap = the smaller of (a) the difference between the width-th and
    the next weight and (b) the smallest difference between two spawned survivors next to each other in weight order (it
    decides which freed slot each gets) - inf where there is no such pair."""
    entries = []  # (weight, 0 existing / 1 spawned, slot, leaf index, token)
    for s, c in enumerate(cands):
        if c is not None and math.isfinite(c["w"]) and math.isfinite(c["u"]):
            entries.append((c["w"], 0, s, 0, -1))
    if fresh:
        for s, c in enumerate(cands):
            if c is None or c["n"] == root or not math.isfinite(c["u"]):
                continue
            for j, (tok, m) in enumerate(tables[s][1]):
                if m > 0:
                    wt = c["u"] + math.log(m)
                    if math.isfinite(wt):
                        entries.append((wt, 1, s, j, tok))
    entries.sort(key=lambda e: (-e[0], e[1], e[2], e[3]))
    gap = entries[width - 1][0] - entries[width][0] if len(entries) > width else math.inf
    keep = entries[:width]
    born = [e for e in keep if e[1] == 1]
    for a, b in zip(born, born[1:]):
        gap = min(gap, a[0] - b[0])
    new, parent, token = [None] * width, [-1] * width, [-1] * width
    for wt, kind, s, j, tok in keep:
        if kind == 0:
            new[s], parent[s] = cands[s], s
    free = [s for s in range(width) if new[s] is None]
    for wt, kind, s, j, tok in born:  # best offer first, lowest freed slot first
        to = free.pop(0)
        new[to] = dict(x=cands[s]["x"] + (tok,), n=root, u=wt, w=wt)
        parent[to], token[to] = s, tok
    return new, parent, token, gap, len(entries)


def next_row(cands, tables, root):
    """Step 3: (float64 [257] log-probabilities, logZ); all -inf for a group without a live candidate or without mass."""
    num = np.zeros(257)
    for s, c in enumerate(cands):
        if c is None or not math.isfinite(c["u"]):
            continue
        e = math.exp(c["u"])
        for b, (child, m) in tables[s][0].items():
            if m > 0:
                num[b] += e * m
        if c["n"] == root:
            num[EOS] += e * sum(m for _, m in tables[s][1] if m > 0)
    Z = num.sum()
    if not Z > 0:
        return np.full(257, NINF), NINF
    with np.errstate(divide="ignore"):
        return np.log(num) - math.log(Z), math.log(Z)


def advance_group(cands, tables, byte, root):
    """Step 4 without the logp bookkeeping: every candidate moves to its child under `byte` or dies; 256 ends the group."""
    new = [None] * len(cands)
    for s, c in enumerate(cands):
        if c is None or byte == EOS:
            continue
        child, m = tables[s][0].get(byte, (None, 0.0))
        if child is not None and m > 0 and math.isfinite(c["u"]):
            new[s] = dict(x=c["x"], n=child, u=c["u"], w=c["u"] + math.log(m))
    return new


class RefTrie:
    """The trie by byte prefix: EOS and ignored tokens spell nothing."""

    def __init__(self, vocab, eos_ids, ignore_ids=()):
        self.eos, self.ignore = [int(t) for t in eos_ids], {int(t) for t in ignore_ids}
        silent = set(self.eos) | self.ignore
        self.words = [b"" if k in silent else bytes(wd) for k, wd in enumerate(vocab)]
        self.kids = {b"": {}}
        self.leaves = {}
        for k, wd in enumerate(self.words):
            for i in range(len(wd)):
                self.kids.setdefault(wd[:i], {})[wd[i]] = wd[:i + 1]
                self.kids.setdefault(wd[:i + 1], {})
            if k not in self.ignore:
                self.leaves.setdefault(wd, []).append(k)

    def tables(self, node, p):
        """The tables of a candidate at `node` whose context's next-token probabilities are `p` (float64 [V])."""
        mass = lambda prefix: float(sum(p[k] for k, wd in enumerate(self.words) if wd.startswith(prefix)))
        return ({b: (child, mass(child)) for b, child in self.kids[node].items()},
                [(k, float(p[k])) for k in self.leaves.get(node, [])])

    def node_mass(self, node, p):
        return float(sum(p[k] for k, wd in enumerate(self.words) if wd.startswith(node)))


class RefBeam:
    """One group of `ByteBeam` on the host: lm(tokens tuple) -> float64 [V] next-token probabilities after prompt + tokens."""

    def __init__(self, lm, vocab, eos_ids, width, ignore_ids=()):
        self.trie, self.lm, self.width = RefTrie(vocab, eos_ids, ignore_ids), lm, width
        self._p = {}
        self.reset()

    def reset(self):
        self.cands = [dict(x=(), n=b"", u=0.0, w=0.0)] + [None] * (self.width - 1)
        self.logp, self.fresh, self.min_gap, self.pruned, self._row = 0.0, False, math.inf, False, None

    def _probs(self, x):
        if x not in self._p:
            self._p[x] = np.asarray(self.lm(x), np.float64)
        return self._p[x]

    def _tables(self):
        return [None if c is None else self.trie.tables(c["n"], self._probs(c["x"])) for c in self.cands]

    def next_byte_logprobs(self):
        if self._row is None:
            self.cands, _, _, gap, entries = extend_group(self.cands, self._tables(), self.width, b"", self.fresh)
            self.min_gap, self.pruned, self.fresh = min(self.min_gap, gap), self.pruned or entries > self.width, False
            self._row = next_row(self.cands, self._tables(), b"")
        return self._row[0]

    def advance(self, byte):
        row = self.next_byte_logprobs()
        self.logp += row[byte]
        self.cands = advance_group(self.cands, self._tables(), byte, b"")
        self.fresh, self._row = True, None

    def live(self):
        return [c for c in self.cands if c is not None]


# ---- brute force over tokenisations ------------------------------------------------------------------------------------------------
def hashed_lm(V, salt=0):
    """A deterministic float64 model: the next-token distribution is seeded by a hash of the context."""
    def lm(x):
        rng = np.random.default_rng(zlib.crc32(repr((salt,) + tuple(x)).encode()))
        z = rng.standard_normal(V) * 1.5
        p = np.exp(z - z.max())
        return p / p.sum()

    return lm


def brute_force(lm, vocab, eos_id, s):
    """(P(s), P(s . EOS)): the summed probability of every token sequence whose bytes have `s` as a prefix while the bytes
    without the last token are shorter than `s` (the empty sequence for the empty `s`), and of every sequence that spells
    exactly `s` followed by EOS."""
    words = [bytes(wd) for wd in vocab]

    def covers(x, done, p):  # done: the bytes x spells, a proper prefix of s
        total = 0.0
        probs = lm(x)
        for k, wd in enumerate(words):
            if k == eos_id or not wd:
                continue
            got = done + wd
            if len(got) >= len(s):
                if got[:len(s)] == s:
                    total += p * probs[k]
            elif s.startswith(got):
                total += covers(x + (k,), got, p * probs[k])
        return total

    def spells(x, done, p):
        if done == s:
            return p * lm(x)[eos_id]
        total = 0.0
        probs = lm(x)
        for k, wd in enumerate(words):
            if k != eos_id and wd and s.startswith(done + wd):
                total += spells(x + (k,), done + wd, p * probs[k])
        return total

    return (1.0 if not s else covers((), b"", 1.0)), spells((), b"", 1.0)


SMALL_VOCAB = [b"<eos>", b"a", b"b", b"c", b"ab", b"bc", b"abc", b"ca", b"aa", b"b"]  # id 0: EOS; ids 2 and 9 spell the same


def vocab257():
    """257 tokens, id 0 the EOS: the 8 letters a..h, their 64 pairs, and 184 triples in a fixed order - every text over
    a..h has many tokenisations."""
    letters = b"abcdefgh"
    out = [b"<eos>"] + [bytes([c]) for c in letters] + [bytes([c, d]) for c in letters for d in letters]
    triples = [bytes([c, d, e]) for c in letters for d in letters for e in letters]
    return out + triples[::2][:184]


# ---- seeded inputs of the kernel tests (tests/test_bytelm_gpu.py), reproducible without a GPU -------------------------------------
def kernel_vocab():
    """64 tokens over a, b, c: two EOS ids (0 and 1), strings of 1..4 letters with repeats (never more than four alike)."""
    rng = np.random.default_rng(2032)
    vocab, count = [b"<eos>", b"<eos2>", b"a", b"b", b"c", b"ab", b"ab", b"ab", b"abc", b"abc"], {}
    for wd in vocab[2:]:
        count[wd] = count.get(wd, 0) + 1
    while len(vocab) < 64:
        wd = bytes(rng.choice(np.frombuffer(b"abc", np.uint8), int(rng.integers(1, 5))))
        if count.get(wd, 0) < 2:
            vocab.append(wd)
            count[wd] = count.get(wd, 0) + 1
    return vocab, [0, 1]


def round_to(x, dtype):
    """float32 values as the store's dtype holds them ("float32" / "bfloat16")."""
    if dtype == "float32":
        return np.asarray(x, np.float32)
    import torch

    return torch.from_numpy(np.asarray(x, np.float32)).to(torch.bfloat16).float().numpy()


def kernel_case(seed, G, width, dtype):
    """The state a kernel test starts from: dict(logits float32 [N, 64] (already rounded to `dtype`; the last slot of group 0
    is a row of -inf when width > 1), node (byte prefixes), alive, u, w).  w = u + log M[node] from the float64 masses of the
    rows, as float32.  With G == 3 the last group has no live candidate."""
    from tests import synth

    vocab, eos = kernel_vocab()
    trie = RefTrie(vocab, eos)
    N = G * width
    rng = np.random.default_rng(seed)
    logits = round_to(synth.logits(seed, N, len(vocab)), dtype)
    if width > 1:
        logits[width - 1] = -np.inf
    inner = sorted(trie.kids)  # every node that is not a leaf
    with_leaves = [n for n in inner if n and n in trie.leaves]
    node, alive, u, w = [], np.zeros(N, np.int32), np.full(N, -np.inf, np.float32), np.full(N, -np.inf, np.float32)
    for s in range(N):
        r = rng.random()
        node.append(b"" if r < 0.15 else with_leaves[rng.integers(len(with_leaves))] if r < 0.85 else inner[rng.integers(len(inner))])
        if (rng.random() < 0.85 or s % width == 0) and not (G == 3 and s >= 2 * width):
            alive[s] = 1
            u[s] = np.float32(-8.0 * rng.random())
            x = logits[s].astype(np.float64)
            if np.isfinite(x).any():
                p = np.exp(x - x.max())
                m = trie.node_mass(node[s], p / p.sum())
                w[s] = np.float32(u[s] + math.log(m)) if m > 0 else -np.inf
            else:
                w[s] = u[s]  # (a row without mass: the kernel only compares w)
    return dict(vocab=vocab, eos=eos, trie=trie, logits=logits, node=node, alive=alive, u=u, w=w)


def host_tables(case, s, node=None):
    """`tables[s]` of a kernel case from float64 masses of its logits row (a row of -inf: no mass anywhere)."""
    x = case["logits"][s].astype(np.float64)
    p = np.zeros(len(x))
    if np.isfinite(x).any():
        p = np.exp(x - x.max())
        p /= p.sum()
    return case["trie"].tables(case["node"][s] if node is None else node, p)


def host_cands(case, g, width):
    return [dict(x=(), n=case["node"][s], u=float(case["u"][s]), w=float(case["w"][s])) if case["alive"][s] else None
            for s in range(g * width, (g + 1) * width)]


KERNEL_CASES = [(G, width, dtype) for G in (1, 3) for width in (1, 2, 5, 64) for dtype in ("float32", "bfloat16")]
MARGIN = 1e-4     # what the host's gap must exceed: ten times the bar below which the GPU test may skip a case


def case_gap(seed, G, width, dtype):
    case = kernel_case(seed, G, width, dtype)
    gap = math.inf
    for g in range(G):
        tables = [host_tables(case, s) for s in range(g * width, (g + 1) * width)]
        gap = min(gap, extend_group(host_cands(case, g, width), tables, width, b"")[3])
    return gap


# per (G, width): the first seed at which the host's gap is finite (something is pruned or two spawned candidates compete) and
# above 1e-3 for both dtypes - found by counting up from 1 with `case_gap`
SEEDS = {(1, 1): 5, (1, 2): 5, (1, 5): 1, (1, 64): 1, (3, 1): 3, (3, 2): 3, (3, 5): 1, (3, 64): 1}


def kernel_seed(G, width, dtype):
    return SEEDS[(G, width)]
