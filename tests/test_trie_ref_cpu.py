"""tests/trie_ref.py, the plain NumPy restatement of the trie masses that tests/test_trie_exact_gpu.py holds every kernel
form against, earns its trust here, without a GPU: it gives the CPU oracle's bits (oracle/glb_oracle.c: an independent
restatement in C) on random and on hostile weights, for sums and maxima, and the reference's own recorded numbers
(tests/golden/ref_round2.npz)."""
import os

import numpy as np
import pytest

from tests import trie_ref

GD = os.path.join(os.path.dirname(__file__), "golden")

VOCABS = {"S": lambda: trie_ref.synthetic_vocab(101, 1500, 5, 6), "M": lambda: trie_ref.synthetic_vocab(202, 8000, 6, 7),
          "W": lambda: trie_ref.synthetic_vocab(303, 2500, 26, 4, skew=1.0),
          "a": lambda: [b"a"], "abc": lambda: [b"abc"], "a,b": lambda: [b"a", b"b"], "nested": lambda: [b"a", b"ab", b"abc"]}


def _trie(words):
    from genlm_backend_amd.tokenization import Token
    from genlm_backend_amd.trie import TokenByteTrie

    return TokenByteTrie([Token(i, w) for i, w in enumerate(words)])


@pytest.mark.parametrize("name", list(VOCABS))
def test_trie_ref_gives_the_oracles_bits(oracle, name):
    words = VOCABS[name]()
    trie = _trie(words)
    flat = trie.flat()
    ref = trie_ref.TrieRef(flat)
    rs = np.random.default_rng(5)
    batches = [("random", rs.random((7, len(words))).astype(np.float32)),
               ("signed", (rs.standard_normal((5, len(words))) * 1e3).astype(np.float32))]
    for kind in ("float32", "bfloat16", "float16"):
        rows, info = trie_ref.hostile_rows(words, kind, 40, seed=11)
        assert np.isnan(rows).any() and np.isinf(rows).any() and (rows == 0).any() and (rows < 0).any()
        assert len(words) < 3 or "big" in info or name == "a,b"
        batches.append(("hostile " + kind, rows))
    for what, ws in batches:
        for op in (0, 1):
            got, want = ref.reduce(ws, op), oracle.trie_reduce(ws, flat, op)
            assert trie_ref.same_bits(got, want), (what, op, trie_ref.first_difference(got, want))
            assert trie_ref.same_bits(got[:, flat["leaf_node"]], ws)  # the leaves are the row, untouched
    assert trie_ref.same_bits(trie_ref.reduce(flat, batches[0][1], 1), ref.reduce(batches[0][1], 1))
    # the folded trie's semantics (a one-child node shows its child as it is): the same bits for weights >= +0.0, and for
    # hostile ones a difference at one-child nodes only
    one_child = ref.n_children == 1
    for what, ws in batches:
        for op in (0, 1):
            plain, folded = ref.reduce(ws, op), ref.reduce(ws, op, folded=True)
            differ = (plain.view(np.uint32) != folded.view(np.uint32)) & ~(np.isnan(plain) & np.isnan(folded))
            assert not differ[:, ~one_child].any(), (what, op)
            assert what != "random" or not differ.any()


def test_trie_ref_hostile_rows_mean_what_they_say(oracle):
    """The properties the GPU tests assert of the kernels hold of the reference itself: a single NaN contaminates exactly
    its leaf's ancestors under sum and nothing under max; negatives and -0.0 leave +0.0; two of the largest finite value
    overflow their node's float32 store; subnormals are summed, not flushed."""
    words = VOCABS["S"]()
    flat = _trie(words).flat()
    ref = trie_ref.TrieRef(flat)
    leaf = flat["leaf_node"]
    internal = np.setdiff1d(np.arange(flat["n_nodes"]), leaf)
    for kind in ("float32", "bfloat16", "float16"):
        rows, info = trie_ref.hostile_rows(words, kind, 40, seed=3, places={"some": 700})
        s, m = ref.reduce(rows, 0), ref.reduce(rows, 1)
        assert len(info["nan"]) == 3
        for r, t in info["nan"]:
            want = np.zeros(flat["n_nodes"], bool)
            want[[int(leaf[t])] + ref.ancestors(leaf[t])] = True
            assert ref.ancestors(leaf[t])[-1] == flat["n_nodes"] - 1  # the root is the last node
            assert np.array_equal(np.isnan(s[r]), want)
            assert np.array_equal(np.nonzero(np.isnan(m[r]))[0], [int(leaf[t])])
        for r in info["clean"]:
            assert not np.isnan(s[r]).any() and not np.isnan(m[r]).any()
        for r in (info["negative"], info["minus_zero"]):
            assert (m[r, internal].view(np.uint32) == 0).all()
        assert (s[info["minus_zero"], internal].view(np.uint32) == 0).all() and (s[info["negative"], internal] < 0).all()
        tiny = trie_ref.palette(kind)["tiny"]
        assert s[info["tiny"], -1] == np.float32(float(tiny) * len(words)) and (m[info["tiny"], internal] == tiny).all()
        r, i, j = info["big"]
        assert words[j][:-1] == words[i]
        above = ref.ancestors(leaf[i])
        assert np.isposinf(s[r, above]).all() == (kind != "float16") and (m[r, above] == trie_ref.palette(kind)["big"]).all()


@pytest.mark.parametrize("tag", ["kat", "syn"])
def test_trie_ref_gives_the_references_numbers(tag):
    gold = np.load(os.path.join(GD, "ref_round2.npz"))
    words = bytes(gold[f"trie::{tag}::words"]).split(b"\x00")
    trie = _trie(words)
    ws = np.ascontiguousarray(gold[f"trie::{tag}::ws"], np.float32)
    for op, key in ((0, "sum"), (1, "max")):
        assert np.abs(trie_ref.reduce(trie.flat(), ws, op) - gold[f"trie::{tag}::{key}"]).max() < 1e-6


def test_leaves_from_logits_is_a_float64_softmax():
    rs = np.random.default_rng(9)
    x = (rs.standard_normal((4, 300)) * 3).astype(np.float32)
    x[1, 5] = -np.inf
    x[3] = -np.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        lse = np.log(np.exp(x.astype(np.float64) * 0.5).sum(1))
    p = trie_ref.leaves_from_logits(x, 0.5, lse)
    assert p.dtype == np.float64 and np.abs(p[:3].sum(1) - 1.0).max() < 1e-12 and p[1, 5] == 0.0
    assert np.isnan(p[3]).all()  # -inf - -inf
