"""The byte-level beam without a GPU: the float64 restatement (tests/bytelm_ref.py) against brute force over
tokenisations, the trie's `child_sym` against its `children`, the constructor's refusals, the argument errors of the three
entry points (they return before any launch) and the seeds of the GPU kernel tests."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

from tests import bytelm_ref as R


def test_restatement_equals_brute_force_over_tokenisations():
    """width 64: nothing is pruned, so the rows are P(s . b) / P(s) and logp is log P(s) - to 1e-12."""
    lm = R.hashed_lm(len(R.SMALL_VOCAB))
    P = {}
    strings = [bytes(t) for n in range(5) for t in itertools.product(b"abc", repeat=n)]
    for s in strings + [s + bytes([b]) for s in strings if len(s) == 4 for b in b"abc"]:
        P[s] = R.brute_force(lm, R.SMALL_VOCAB, 0, s)
    assert P[b""][0] == 1.0
    for s in strings:
        beam = R.RefBeam(lm, R.SMALL_VOCAB, [0], 64)
        for b in s:
            beam.advance(b)
        row = beam.next_byte_logprobs()
        assert len(beam.live()) < 64 and not beam.pruned
        assert abs(beam.logp - math.log(P[s][0])) < 1e-12, s
        for b in b"abc":
            assert abs(row[b] - math.log(P[s + bytes([b])][0] / P[s][0])) < 1e-12, (s, b)
        assert abs(row[R.EOS] - math.log(P[s][1] / P[s][0])) < 1e-12, s
        assert abs(np.logaddexp.reduce(row)) < 1e-12
        assert all(row[b] == -np.inf for b in range(256) if b not in b"abc")
        assert row is beam.next_byte_logprobs()  # the same row until the next advance


def test_restatement_prunes_by_weight_and_keeps_slots():
    lm = R.hashed_lm(len(R.SMALL_VOCAB), salt=1)
    beam = R.RefBeam(lm, R.SMALL_VOCAB, [0], 2)
    for b in b"abca":
        beam.advance(b)
        assert len(beam.live()) <= 2
    assert beam.pruned
    # a kept candidate stays in its slot; the best spawned one takes the lowest freed slot
    cands = [dict(x=(), n=b"ab", u=-1.0, w=-0.5), None, dict(x=(), n=b"a", u=-3.0, w=-2.9)]
    tables = [({}, [(4, 0.5), (7, 0.25)]), None, ({}, [(1, 0.9)])]
    new, parent, token, gap, entries = R.extend_group(cands, tables, 3, b"")
    # weights: -0.5 (slot 0), -1.69 (slot 0 commits 4), -2.39 (slot 0 commits 7) | -2.9 (slot 2), -3.1 (slot 2 commits 1)
    assert parent == [0, 0, 0] and token == [-1, 4, 7] and new[1]["x"] == (4,) and new[1]["n"] == b"" and new[2]["x"] == (7,)
    assert entries == 5 and gap == pytest.approx(-1.0 + math.log(0.25) + 2.9)


@pytest.mark.parametrize("which", ["small", "257"])
def test_child_sym_names_every_edge(which):
    from genlm_backend_amd.bytelm import byte_trie, byte_trie_arrays, children_table

    vocab = R.SMALL_VOCAB if which == "small" else R.vocab257()
    ignore = () if which == "small" else (5,)
    trie = byte_trie(vocab, [0], ignore)
    f = trie.flat()
    assert f["child_sym"].dtype == np.int16 and f["child_sym"].shape == f["child_idx"].shape
    ref = R.RefTrie(vocab, [0], ignore)
    for n, kids in enumerate(trie.children):
        lo, hi = f["child_ptr"][n], f["child_ptr"][n + 1]
        got = dict(zip(f["child_sym"][lo:hi].tolist(), f["child_idx"][lo:hi].tolist()))
        leaves = sorted(c for sym, c in kids.items() if isinstance(sym, tuple) and sym[1] not in ignore)
        want = {sym: c for sym, c in kids.items() if not isinstance(sym, tuple)}
        want.update({256 + j: c for j, c in enumerate(leaves)})
        if any(isinstance(sym, tuple) and sym[1] in ignore for sym in kids):
            assert set(f["child_idx"][lo:hi][f["child_sym"][lo:hi] == -2].tolist()) == {kids[(None, k)] for k in ignore}
            got.pop(-2)
        assert got == want, n
        # ... and the restatement's trie is the same trie
        prefix = bytes(trie.node2prefix[n])
        if kids:
            assert {b: bytes(trie.node2prefix[c]) for b, c in want.items() if b < 256} == ref.kids[prefix]
            assert [trie.leaf2word[c][1] for c in leaves] == ref.leaves.get(prefix, [])
    arr = byte_trie_arrays(trie)
    assert arr["root"] == trie.root and arr["leaf_token"][trie.word2leaf[(b"", 0)]] == 0
    assert (arr["leaf_token"] >= 0).sum() == len(vocab)
    tab = children_table(trie, [trie.root])
    assert tab[0, 256] == trie.word2leaf[(b"", 0)] and (tab[0, 257:] == -1).all() and tab[0, ord("a")] >= 0


def test_constructor_refusals_name_the_token():
    from genlm_backend_amd.bytelm import ByteBeam

    ok = [b"<eos>", b"a", b"b"]
    with pytest.raises(ValueError, match="token 2 has an empty byte string"):
        ByteBeam(None, [b"<eos>", b"a", b"", b"b"], [0])
    with pytest.raises(ValueError, match=r"tokens \[1, 2, 3, 4, 5\] all spell b'ab'"):
        ByteBeam(None, [b"<eos>"] + [b"ab"] * 5, [0])
    for width in (0, 65):
        with pytest.raises(ValueError, match="width must be an integer in 1..64"):
            ByteBeam(None, ok, [0], width=width)
    with pytest.raises(ValueError, match="eos_ids must name 1..4 distinct tokens"):
        ByteBeam(None, ok, [])
    with pytest.raises(ValueError, match="temperature"):
        ByteBeam(None, ok, [0], temperature=0.0)

    class NoBos:
        tokenizer = None
        engine = None

    with pytest.raises(ValueError, match="give prompt_ids"):
        ByteBeam(NoBos(), ok, [0])
    # an ignored empty token is fine, and four tokens alike are
    from genlm_backend_amd.bytelm import byte_trie

    trie = byte_trie([b"<eos>", b"", b"ab", b"ab", b"ab", b"ab"], [0], ignore_ids=[1])
    assert (trie.flat()["child_sym"] == -2).sum() == 1 and trie.flat()["child_sym"].max() == 259


def test_entry_points_reject_bad_arguments_before_any_launch():
    import genlm_backend_amd  # noqa: F401
    from genlm_backend_amd import _lib

    lib = _lib.load()
    calls = (lib.glb_bytelm_children, lib.glb_bytelm_extend, lib.glb_bytelm_next)
    for call in calls:
        assert call(None, None) == _lib.GLB_EINVAL
    hdr = ('#include "glb.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) { printf("%zu %zu %d %d %d\\n", '
           'sizeof(glb_bytelm_args), offsetof(glb_bytelm_args, logp), GLB_BYTELM_SEL, GLB_BYTELM_ROW, GLB_BYTELM_LEAVES); return 0; }\n')
    import os
    import subprocess
    import tempfile

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(hdr)
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got == [C.sizeof(_lib.ByteLmArgs), _lib.ByteLmArgs.logp.offset, 260, 257, 4]

    def block(**kw):
        a = _lib.ByteLmArgs()
        a.struct_size = C.sizeof(_lib.ByteLmArgs)
        a.width, a.n_groups, a.n_nodes, a.root = 4, 2, 10, 9
        for f, _ in _lib.ByteLmArgs._fields_:
            if f not in ("struct_size", "width", "n_groups", "n_nodes", "root", "fresh", "byte"):
                setattr(a, f, 4096 + 64 * len(f))  # any distinct non-null value: nothing may be read
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    bad = [dict(struct_size=8), dict(width=0), dict(width=65), dict(n_groups=0), dict(n_nodes=0), dict(n_groups=1 << 30),
           dict(n_nodes=1 << 31), dict(root=10), dict(root=-1), dict(node=None), dict(alive=None), dict(sel=None)]
    for kw in bad:
        for call in calls:
            assert call(C.byref(block(**kw)), None) == _lib.GLB_EINVAL, kw
    for f in ("child_ptr", "child_idx", "child_sym"):
        assert calls[0](C.byref(block(**{f: None})), None) == _lib.GLB_EINVAL, f
    for f in ("u", "w", "mass", "leaf_token", "out_parent", "out_token", "out_node", "out_alive", "out_u", "out_w", "out_spawned",
              "out_n_spawned"):
        assert calls[1](C.byref(block(**{f: None})), None) == _lib.GLB_EINVAL, f
    a = block()
    a.out_u = a.u
    assert calls[1](C.byref(a), None) == _lib.GLB_EINVAL and "may not lie over" in _lib.last_error()
    for f in ("u", "w", "mass", "out_next", "out_logZ"):
        assert calls[2](C.byref(block(**{f: None})), None) == _lib.GLB_EINVAL, f
    assert calls[2](C.byref(block(byte=4096, logp=None)), None) == _lib.GLB_EINVAL


def test_kernel_test_seeds_have_wide_gaps_on_the_host():
    """tests/test_bytelm_gpu.py may skip a pruning case only where the device's own masses bring the deciding weights within
    1e-5 of each other; the seeds are chosen so that float64 masses of the same rows keep them 1e-4 apart and more: the
    restatement alone skips none."""
    for G, width, dtype in R.KERNEL_CASES:
        gap = R.case_gap(R.kernel_seed(G, width, dtype), G, width, dtype)
        assert R.MARGIN < gap < math.inf, (G, width, dtype, gap)
    vocab, eos = R.kernel_vocab()
    assert len(vocab) == 64 and len(set(vocab)) < 64 and len(eos) == 2
