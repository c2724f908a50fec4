"""Every form of the token -> byte trie mass kernels against a plain reference (tests/trie_ref.py, itself held against the
CPU oracle and the reference's numbers in tests/test_trie_ref_cpu.py):

  A  the structure is exact whatever the leaves: a kernel's own leaf columns, reduced by the reference, give the kernel's
     every node bit for bit - also for masses straight from logits, without trusting the hardware's exp;
  B  the leaves from logits are accurate against float64 within a derived bound, -inf logits give +0.0, a row that allows
     one token puts mass 1 on that token's path and +0.0 elsewhere, a row without any allowed token is NaN the same way
     in every form;
  C  hostile weights (zeros of both signs, subnormals, the largest finite value, infinities, NaN, negatives) at the places
     where the kernels read past a node, store other parts' tokens into slack or hand values from a part to the top;
  D  the switches of the level kernels (32 rows: row-major / node-major; 256 output columns: narrow / wide untranspose)
     at the boundaries themselves;
  E  nothing is written outside the output asked for: pitched outputs between guard rows, selections with ids outside the
     trie.

`forms()` lists every way the library produces all-node rows.  Not covered here: the sweep kernel's loop for rows longer
than 7 units of 8 tokens a thread (V > 57344) - tests/test_host_gpu.py's 128k-token test reaches it, and a vocabulary of
that size does not fit a test of a few seconds.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import trie_ref

pytestmark = pytest.mark.gpu

DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}
# name -> (vocabulary, slots per part of the gathered plan with several parts and a top, of the sweep plan with several)
VOCABS = {"S": (lambda: trie_ref.synthetic_vocab(101, 1500, 5, 6), 250, 300),
          "M": (lambda: trie_ref.synthetic_vocab(202, 8000, 6, 7), 400, 300),
          # 26 letters of very different frequencies: nodes of 2 .. 27 children in one wave of the sweep kernel's reduction
          # (its eight-children trips, the lanes that finish before the wave's widest node does)
          "W": (lambda: trie_ref.synthetic_vocab(303, 2500, 26, 4, skew=1.0), 250, 300)}
DEGENERATE = {"a": [b"a"], "abc": [b"abc"], "a,b": [b"a", b"b"], "nested": [b"a", b"ab", b"abc"]}
ONE_PART_CAP = 20000
SENTINEL = 0x5EA7BEEF  # (as float32: 6.04e18 - never a mass)

_cache = {}


class Case:
    """A vocabulary's trie, its reference and its plans, built once per module."""

    def __init__(self, name, engine):
        from genlm_backend_amd.tokenization import Token
        from genlm_backend_amd.trie import TokenByteTrie

        self.name = name
        if name in VOCABS:
            make, self.small_cap, self.sweep_cap = VOCABS[name]
            self.words = make()
        else:
            self.words, self.small_cap, self.sweep_cap = DEGENERATE[name], None, None
        self.trie = TokenByteTrie([Token(i, w) for i, w in enumerate(self.words)], engine=engine)
        self.flat = self.trie.flat()
        self.ref = trie_ref.TrieRef(self.flat)
        self.V, self.nn = len(self.words), len(self.trie)
        self.leaf = np.asarray(self.flat["leaf_node"], np.int64)
        self.internal = np.setdiff1d(np.arange(self.nn), self.leaf)
        self.kinds = ALL_KINDS if name in VOCABS else DEGENERATE_KINDS


def case(name, engine):
    if name not in _cache:
        _cache[name] = Case(name, engine)
    return _cache[name]


ALL_KINDS = ("levels", "levels-folded", "gathered-parts", "gathered-one", "sweep-parts", "sweep-one")
DEGENERATE_KINDS = ("levels", "gathered-one", "sweep-one")  # (no top to cut off, no node with two children to fold around)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _trie_masses_into(engine, ws, flat, op, from_logprobs, lse, logit_scale, nodes, out):
    """glb_trie_masses with a caller's (pitched) output: `HipEngine.trie_masses` allocates its own."""
    from genlm_backend_amd import _lib
    from genlm_backend_amd.engine import _DT

    B, n_nodes = ws.shape[0], flat["n_nodes"]
    a = _lib.TrieArgs()
    a.struct_size = C.sizeof(_lib.TrieArgs)
    a.weights, a.dtype = ws.data_ptr(), _DT[ws.dtype]
    a.ld = ws.stride(0) if B > 1 else max(flat["vocab"], ws.stride(0))
    a.n_rows, a.vocab = B, flat["vocab"]
    a.lse = None if lse is None else lse.data_ptr()
    a.logit_scale, a.from_logprobs, a.op = logit_scale, 1 if from_logprobs else 0, op
    a.n_nodes, a.n_levels = n_nodes, flat["n_levels"]
    ls = flat["level_start_host"]
    a.leaf_node, a.level_start_host = flat["leaf_node"].data_ptr(), ls.ctypes.data
    a.level_nodes, a.child_ptr, a.child_idx = (flat[k].data_ptr() for k in ("level_nodes", "child_ptr", "child_idx"))
    scratch = torch.empty(engine.lib.glb_trie_workspace_ex(B, n_nodes), dtype=torch.uint8, device=engine.device)
    a.workspace, a.workspace_bytes = scratch.data_ptr(), scratch.numel()
    assert out.dtype == torch.float32 and out.stride(1) == 1
    if nodes is not None:
        assert out.shape == (B, nodes.numel())
        a.sel_nodes, a.n_sel, a.out_sel, a.out_sel_ld = nodes.data_ptr(), nodes.numel(), out.data_ptr(), out.stride(0)
    else:
        assert out.shape == (B, n_nodes)
        a.out, a.out_ld = out.data_ptr(), out.stride(0)
    rc = engine.lib.glb_trie_masses(C.byref(a), engine._stream())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()  # (the scratch lives until the kernels are done)
    return out


def _trie_rows_into(engine, ws, plan, op, from_logprobs, lse, logit_scale, nodes=None, out_nodes=None, out_slots=None, out_sel=None):
    """glb_trie_rows with a caller's pitched outputs (`HipEngine.trie_rows` takes contiguous ones only); any of the three
    kinds of output at once."""
    from genlm_backend_amd import _lib
    from genlm_backend_amd.engine import _DT

    B = ws.shape[0]
    pl = _lib.TriePlan()
    pl.struct_size = C.sizeof(_lib.TriePlan)
    for k in ("n_parts", "n_top", "n_cut", "n_slots", "max_local", "top_base", "lds_bytes", "n_nodes"):
        setattr(pl, k, int(plan[k]))
    for k in ("desc", "idepth", "leaf_src", "leaf_local", "run_tab", "top_local", "slot_of", "cptr16", "inode16", "pn_local16"):
        setattr(pl, k, plan[k].data_ptr())
    if plan.get("sweep"):
        pl.tok_local16, pl.inode64 = plan["tok_local16"].data_ptr(), plan["inode64"].data_ptr()
        pl.lds_top_bytes, pl.vocab = int(plan["lds_top_bytes"]), int(plan["vocab"])
    a = _lib.TrieRowsArgs()
    a.struct_size = C.sizeof(_lib.TrieRowsArgs)
    a.weights, a.dtype = ws.data_ptr(), _DT[ws.dtype]
    a.ld = ws.stride(0) if B > 1 else max(plan["vocab"], ws.stride(0))
    a.n_rows, a.vocab = B, plan["vocab"]
    a.lse = None if lse is None else lse.data_ptr()
    a.logit_scale, a.from_logprobs, a.op = logit_scale, 1 if from_logprobs else 0, op
    scratch = torch.empty(max(1, engine.lib.glb_trie_rows_workspace(B, C.byref(pl))), dtype=torch.uint8, device=engine.device)
    a.workspace, a.workspace_bytes = scratch.data_ptr(), scratch.numel()
    for o, width in ((out_nodes, plan["n_nodes"]), (out_slots, plan["n_slots"])):
        assert o is None or (o.shape == (B, width) and o.dtype == torch.float32 and o.stride(1) == 1)
    if out_nodes is not None:
        a.out_nodes, a.out_nodes_ld = out_nodes.data_ptr(), out_nodes.stride(0)
    if out_slots is not None:
        a.out_slots, a.out_slots_ld = out_slots.data_ptr(), out_slots.stride(0)
    if out_sel is not None:
        per_row = nodes.dim() == 2
        width = nodes.shape[1] if per_row else nodes.numel()
        assert nodes.dtype == torch.int32 and nodes.is_contiguous() and out_sel.shape == (B, width) and out_sel.stride(1) == 1
        assert not per_row or nodes.shape[0] == B
        a.sel_nodes, a.n_sel, a.out_sel, a.out_sel_ld = nodes.data_ptr(), width, out_sel.data_ptr(), out_sel.stride(0)
        a.sel_row_stride = width if per_row else 0
    rc = engine.lib.glb_trie_rows(C.byref(a), C.byref(pl), engine._stream())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()  # (the scratch lives until the kernels are done)


def sweep_lanes(n_parts, n_rows, cus):
    """Rows in flight of the sweep kernel (glb_trie.hip: launch_sweep1, one workgroup a CU): lane g takes rows g, g + lanes, ..."""
    lanes = max(8, (cus // n_parts) & ~7)
    return min(lanes, (n_rows + 7) & ~7)


def forms(trie, engine, n_rows=9, kinds=ALL_KINDS, small_cap=250, sweep_cap=300):
    """(name, call) for every way the library produces all-node rows from a [n_rows, V] device tensor:
    call(ws, op=0, from_logprobs=False, lse=None, logit_scale=1.0, alloc=None) -> float32 [n_rows, n_nodes] in node order.
    alloc(shape): where the kernel's own output(s) go (default: fresh tensors of exactly that shape).  What a form needs of
    the trie and the row count is asserted: a form never silently becomes another one."""
    dev, nn = engine.device, len(trie)

    if "levels" in kinds:
        flat = trie.device_arrays()

        def levels(ws, op=0, from_logprobs=False, lse=None, logit_scale=1.0, alloc=None):
            assert ws.shape[0] == n_rows
            if alloc is None:
                return engine.trie_masses(ws, flat, op, from_logprobs, lse=lse, logit_scale=logit_scale)
            return _trie_masses_into(engine, ws, flat, op, from_logprobs, lse, logit_scale, None, alloc((n_rows, nn)))

        # (glb_trie_levels.hip: kTrieNodeMajorRows = 32; all nodes out: the narrow untranspose below 256 nodes)
        yield ("levels-row-major" if n_rows < 32 else "levels-node-major"), levels
    if "levels-folded" in kinds:  # what TokenByteTrie._batch does from 32 rows on: the folded trie, every node selected
        c = trie.compact_device_arrays()
        assert trie.compact()["n_levels"] > 0 and trie.compact()["n_nodes"] < nn

        def folded(ws, op=0, from_logprobs=False, lse=None, logit_scale=1.0, alloc=None):
            assert ws.shape[0] == n_rows
            if alloc is None:
                return engine.trie_masses(ws, c, op, from_logprobs, lse=lse, logit_scale=logit_scale, nodes=c["slot_of"])
            return _trie_masses_into(engine, ws, c, op, from_logprobs, lse, logit_scale, c["slot_of"], alloc((n_rows, nn)))

        yield "levels-folded-selected", folded

    perm = torch.from_numpy(np.random.default_rng(nn).permutation(nn).astype(np.int32)).to(dev)
    inv = torch.argsort(perm.long())

    def rows_forms(tag, cap, sweep, outputs):
        host = trie.plan(cap, sweep=sweep)
        assert host is not None and bool(host["sweep"]) == sweep, (tag, cap)
        pl = trie.plan_device_arrays(cap, sweep=sweep)
        slot_of = torch.from_numpy(host["slot_of"].astype(np.int64)).to(dev)
        assert int(slot_of.min()) >= 0
        n_slots = host["n_slots"]

        def make(output):
            def call(ws, op=0, from_logprobs=False, lse=None, logit_scale=1.0, alloc=None):
                assert ws.shape[0] == n_rows
                kw = dict(lse=lse, logit_scale=logit_scale)
                if alloc is not None:  # (pitched outputs: the C entry point itself)
                    o_nodes = alloc((n_rows, nn)) if output == "nodes" else None
                    o_slots = alloc((n_rows, n_slots)) if "slots" in output else None
                    o_sel = alloc((n_rows, nn)) if "selected" in output else None
                    _trie_rows_into(engine, ws, pl, op, from_logprobs, lse, logit_scale, perm, o_nodes, o_slots, o_sel)
                    got = o_nodes if output == "nodes" else (o_slots[:, slot_of] if output == "slots" else o_sel[:, inv])
                    if output == "selected+slots":
                        assert torch.equal(_bits(o_slots[:, slot_of]), _bits(got)), f"{tag}: slots and selected nodes of one call differ"
                    return got
                if output == "nodes":
                    return engine.trie_rows(ws, pl, op, from_logprobs, **kw)
                if output == "slots":
                    return engine.trie_rows(ws, pl, op, from_logprobs, layout="slots", **kw)[:, slot_of]
                if output == "selected":
                    return engine.trie_rows(ws, pl, op, from_logprobs, nodes=perm, **kw)[:, inv]
                both = torch.empty((n_rows, n_slots), dtype=torch.float32, device=dev)
                got = engine.trie_rows(ws, pl, op, from_logprobs, nodes=perm, out_slots=both, **kw)[:, inv]
                assert torch.equal(_bits(both[:, slot_of]), _bits(got)), f"{tag}: slots and selected nodes of one call differ"
                return got
            return call

        for output in outputs:
            yield f"{tag}-{output}", make(output)
        return host

    every = ("nodes", "slots", "selected", "selected+slots")  # the sweep kernel's OUT = 2, 1, 4, 7
    if "gathered-parts" in kinds:
        host = trie.plan(small_cap)
        assert host is not None and host["n_parts"] > 1 and host["n_top"] > 0 and host["lds_bytes"] * 8 <= 160 * 1024, "several parts, a top, 256 threads"
        yield from rows_forms(f"gathered-{small_cap}", small_cap, False, ("nodes", "selected+slots"))
    if "gathered-one" in kinds:
        host = trie.plan(ONE_PART_CAP)
        assert host is not None and host["n_parts"] == 1 and host["n_top"] == 0
        yield from rows_forms("gathered-one-part", ONE_PART_CAP, False, ("nodes",))
    if "sweep-parts" in kinds:
        host = trie.plan(sweep_cap, sweep=True)
        assert host is not None and host["n_parts"] > 1 and host["n_top"] > 0
        yield from rows_forms(f"sweep-{sweep_cap}", sweep_cap, True, every)
    if "sweep-one" in kinds:
        host = trie.plan(None, sweep=True)
        assert host is not None and host["n_parts"] == 1 and host["n_top"] == 0
        yield from rows_forms("sweep-one-part", None, True, every)


def case_forms(cs, engine, n_rows, kinds=None):
    kinds = cs.kinds if kinds is None else kinds
    return forms(cs.trie, engine, n_rows, kinds, cs.small_cap or 250, cs.sweep_cap or 300)


def is_folded(fname):
    """Forms over the folded trie (every one but the level kernels on the trie's own arrays): a node with one child shows
    its child's value as it is - `trie_ref.TrieRef.reduce(folded=True)`, `TokenByteTrie.batch_weight_max`'s docstring."""
    return not fname.startswith(("levels-row-major", "levels-node-major"))


def check_structure(cs, got, op, what):
    """A: the kernel's leaf columns, reduced by the reference, are the kernel's every node (NaN by position)."""
    got = got.cpu().numpy()
    want = cs.ref.reduce(np.ascontiguousarray(got[:, cs.leaf]), op, folded=is_folded(what[0]))
    assert trie_ref.same_bits(got, want), (what, "row, node, got, want, differing:", trie_ref.first_difference(got, want))
    return got


def rounded(x, dt, dev):
    """float32 host rows -> device rows of type dt, and the values they hold (float64, upcast exactly)."""
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev).to(dt)
    return xd, xd.float().double().cpu().numpy()


def wide_logits(rs, B, V):
    """Logits of a wide range: normal * 3; 2 % of the entries 40 .. 85 below the row's maximum; 1 % -inf; row B - 2 allows
    one token only; row B - 1 allows none (B >= 4)."""
    x = (rs.standard_normal((B, V)) * 3).astype(np.float32)
    top = x.max(1, keepdims=True)
    low = rs.random((B, V)) < 0.02
    x = np.where(low, top - rs.uniform(40, 85, (B, V)).astype(np.float32), x)
    x[rs.random((B, V)) < 0.01] = -np.inf
    x[np.arange(B), rs.integers(0, V, B)] = top[:, 0]  # (the maximum itself is never masked)
    one_tok = int(rs.integers(0, V))
    if B >= 4:
        x[B - 2] = -np.inf
        x[B - 2, one_tok] = 1.25
        x[B - 1] = -np.inf
    return x.astype(np.float32), one_tok


# ---------------------------------------------------------------------------------------------------------------------
def test_the_vocabularies_reach_the_branches_they_are_for(engine):
    """M at one gathered part: more than 8 * 512 slots (twelve leaves a thread in flight) and more table words than
    12 * 512 (the loop for a part too big for kT words a thread); W: a wave of the sweep kernel's reduction whose widest
    node takes three eight-children trips and more while another lane's node is done after one."""
    m = case("M", engine).trie.plan(ONE_PART_CAP)
    assert m["n_parts"] == 1 and m["lds_bytes"] * 8 > 160 * 1024 and m["max_local"] > 8 * 512
    d = m["desc"][0]
    assert ((d[1] + 2) >> 1) + ((d[12] + 1) >> 1) + d[3] + 1 > 12 * 512
    for cap in (VOCABS["W"][2], None):
        assert examined_part(case("W", engine).trie.plan(cap, sweep=True), min_widest=17) is not None


def examined_part(host, min_widest=5):
    """(part, depth, widest, narrowest) of the first part of a sweep plan that has, at some depth, in the first wave of the
    reduction (1024 threads: lanes 0 .. 63 take the depth's first 64 nodes, widest first) a widest node whose child count is
    no multiple of 8 and a narrower node beside it; None if there is none."""
    d, i64 = host["desc"], host["inode64"]
    for p in range(host["n_parts"]):
        idp = host["idepth"][d[p, 13]:d[p, 13] + d[p, 3] + 1]
        cnt = (i64[d[p, 11]:d[p, 11] + d[p, 12]] >> np.uint64(32)).astype(np.int64)
        for k in range(len(idp) - 1):
            c = cnt[idp[k]:idp[k + 1]][:64]
            if len(c) > 1 and c[0] % 8 != 0 and c[0] >= min_widest and c[-1] < c[0] and c[-1] <= 8:
                return p, k, int(c[0]), int(c[-1])
    return None


@pytest.mark.parametrize("kind", list(DTYPES))
@pytest.mark.parametrize("name", list(VOCABS) + list(DEGENERATE))
def test_structure_is_exact_whatever_the_leaves(engine, name, kind):
    """A.  Every form, sum and max, weights and masses from logits at logit_scale 1.0 and 0.5 (`masses_from_logits(op=1)`
    is these calls with op = 1: every form has it)."""
    cs, dt, dev = case(name, engine), DTYPES[kind], engine.device
    rs = np.random.default_rng(21)
    for B in (1, 9, 70):
        wd, _ = rounded(rs.random((B, cs.V)), dt, dev)
        x, _ = wide_logits(rs, B, cs.V)
        xd, _ = rounded(x, dt, dev)
        lses = {s: engine.step(xd, vocab=cs.V, rng_mode=0, logit_scale=s)[1] for s in (1.0, 0.5)}
        for fname, call in case_forms(cs, engine, B):
            for op in (0, 1):
                check_structure(cs, call(wd, op), op, (fname, B, op, "weights"))
                for s, lse in lses.items():
                    got = check_structure(cs, call(xd, op, True, lse, s), op, (fname, B, op, "logits", s))
                    if B >= 4 and op == 0:  # (the rows are not empty; how good the leaves are is B's business)
                        assert (np.abs(got[:B - 2, cs.trie.root] - 1) < 1e-3).all(), (fname, B, op, s)


@pytest.mark.parametrize("kind", list(DTYPES))
@pytest.mark.parametrize("name", list(VOCABS))
def test_leaves_from_logits_are_accurate(engine, name, kind):
    """B.  With x the logit as the kernel reads it (upcast exactly), a = x * scale - lse in float64 (lse: the float32 the
    fused step wrote) and want = exp(a), every leaf holds  |got - want| <= want * 2^-23 * (|x * scale| + 3 |a| + 2).
    Derivation, in units of 2^-24 relative to want (an error d of the exponent is a relative error d of the result):
      - the float32 subtraction x * scale - lse, one rounding with contraction and two without: |x * scale| + |a|
        (scales 0.5, 1, 2 are exact; the unfused product rounds to within 2^-24 |x * scale|, the difference to 2^-24 |a|);
      - the product with the float32 log2(e) (a rounded constant, a rounded product), carried through 2^y: 2 |a|;
      - v_exp_f32 itself: 1 ulp = 2 (glb_trie.hpp; the ISA guide);
      - all of it times two for the second-order terms: 2^-23 * (|x * scale| + 3 |a| + 2).
    The root holds the float64 sum of `want` within the sum of the leaves' bounds plus 2 * 2^-24 of the sum for every
    level above them (a float32 store each).  A -inf logit gives exactly +0.0.  Where want < 2^-126 the raw 2^y may flush:
    0.0 or the bound; the test's inputs keep those under 5 % of the leaves (asserted from the float64 values alone).
    The row that allows one token: mass 1 within the bound on that token's leaf and its ancestors, +0.0 at every other
    node.  The row that allows none has lse = -inf, every leaf is exp(-inf + inf) = NaN in every form, every sum above NaN
    and every max above +0.0 (a NaN is never taken: test A compares those rows with the reference bit for bit)."""
    cs, dt, dev = case(name, engine), DTYPES[kind], engine.device
    rs = np.random.default_rng(33)
    worst, root_worst = 0.0, 0.0
    for B in (9, 70):
        x, one_tok = wide_logits(rs, B, cs.V)
        xd, xv = rounded(x, dt, dev)
        for scale in (0.5, 1.0, 2.0):
            lse = engine.step(xd, vocab=cs.V, rng_mode=0, logit_scale=scale)[1]
            lse_h = lse.cpu().numpy()
            assert np.isfinite(lse_h[:B - 1]).all() and (np.isneginf(lse_h[B - 1]) or np.isnan(lse_h[B - 1])), lse_h[-3:]
            lse[B - 1] = float("-inf")
            live = np.arange(B - 1)
            xs = xv[live] * scale
            a = xs - lse_h[live].astype(np.float64)[:, None]
            want = trie_ref.leaves_from_logits(xv[live], scale, lse_h[live])
            masked = np.isneginf(xv[live])
            assert (want[masked] == 0).all()
            with np.errstate(invalid="ignore"):
                bound = np.where(masked, 0.0, want * 2.0 ** -23 * (np.abs(xs) + 3 * np.abs(a) + 2))
            tiny = ~masked & (want < 2.0 ** -126)
            assert tiny.mean() < 0.05 and np.abs(want[:B - 2].sum(1) - 1).max() < 1e-4, (tiny.mean(), want.sum(1))
            levels_up = cs.flat["n_levels"]
            for fname, call in case_forms(cs, engine, B):
                got = call(xd, 0, True, lse, scale).cpu().numpy()
                L = got[:, cs.leaf].astype(np.float64)
                assert np.isnan(got[B - 1]).all(), (fname, "the row without an allowed token", got[B - 1][~np.isnan(got[B - 1])][:4])
                gm = call(xd, 1, True, lse, scale).cpu().numpy()
                reducing = cs.internal[cs.ref.n_children[cs.internal] >= 2] if is_folded(fname) else cs.internal
                assert np.isnan(gm[B - 1, cs.leaf]).all() and (gm[B - 1, reducing].view(np.uint32) == 0).all(), fname
                check_structure(cs, torch.from_numpy(gm), 1, (fname, B, "max", scale))
                Ll = L[live]
                assert (got[live][:, cs.leaf][masked].view(np.uint32) == 0).all(), (fname, "-inf logit: not +0.0")
                err = np.abs(Ll - want)
                flushed = tiny & (Ll == 0)
                with np.errstate(invalid="ignore", divide="ignore"):
                    ratio = np.where(masked | flushed, 0.0, err / bound)
                worst = max(worst, float(ratio.max()))
                r, t = np.unravel_index(ratio.argmax(), ratio.shape)
                assert ratio.max() <= 1.0, (f"{fname} B={B} scale={scale} {kind}: error / bound = {ratio.max():.3f} at row {r} token {t}: "
                                            f"x={xv[r, t]!r} lse={lse_h[r]!r} got={Ll[r, t]!r} want={want[r, t]!r}")
                root_bound = np.where(flushed, want, bound).sum(1) + 2 * levels_up * 2.0 ** -24 * want.sum(1)
                rr = np.abs(got[live, cs.trie.root].astype(np.float64) - want.sum(1)) / root_bound
                root_worst = max(root_worst, float(rr.max()))
                assert rr.max() <= 1.0, (fname, B, scale, "root", rr.max())
                # the row that allows one token
                path = [int(cs.leaf[one_tok])] + cs.ref.ancestors(cs.leaf[one_tok])
                off = np.setdiff1d(np.arange(cs.nn), path)
                assert (got[B - 2, off].view(np.uint32) == 0).all(), (fname, "mass off the only allowed token's path")
                assert abs(want[B - 2, one_tok] - 1) < 1e-5  # (the step's lse of that row is its one logit)
                assert np.abs(got[B - 2, path].astype(np.float64) - want[B - 2, one_tok]).max() <= bound[B - 2, one_tok], (fname, got[B - 2, path])
    print(f"\ntrie leaves from logits, {name} {kind}: worst error / bound {worst:.4f} (root: {root_worst:.4f})")


def hostile_case(cs, kind, B):
    """C's rows for a vocabulary: `trie_ref.hostile_rows` with the places the plans name, and (from 40 rows on) rows whose
    every token OUTSIDE the examined part of the sweep plan is NaN / +inf / a negative: whatever the sweep kernel stores into
    the slack behind that part's values, and reads there past a node's last child, is hostile."""
    if not hasattr(cs, "places"):
        cs.places, cs.own, cs.inside = _hostile_places(cs)
    rows, info = trie_ref.hostile_rows(cs.words, kind, B, seed=77, places=cs.places)
    if cs.own is not None and B >= 40:
        pal = trie_ref.palette(kind)
        for r, v in zip((B - 3, B - 2, B - 1), (pal["nan"], pal["+inf"], pal["negative"])):
            rows[r] = np.where(cs.own, trie_ref.round_to(np.random.default_rng(r).random(cs.V).astype(np.float32), kind), v)
        info["outside"] = (B - 3, cs.inside)
    return rows, info


def _hostile_places(cs):
    places, own, inside = {}, None, None
    if cs.small_cap:
        for tag, host in (("gathered", cs.trie.plan(cs.small_cap)), ("sweep", cs.trie.plan(cs.sweep_cap, sweep=True))):
            d = host["desc"]
            last = host["n_parts"] - 1
            places[tag + "-first-part"] = int(host["leaf_src"][d[0, 6]])
            places[tag + "-last-part"] = int(host["leaf_src"][d[last, 6] + d[last, 7] - 1])
            # a token whose leaf hangs directly under a node of the top: the first ancestor with a slot of its own is the top's
            slot = host["slot_of"]
            for t in range(cs.V):
                up = [n for n in cs.ref.ancestors(cs.leaf[t]) if slot[n] != slot[cs.leaf[t]]]
                if slot[cs.leaf[t]] < host["top_base"] <= slot[up[0]]:
                    places[tag + "-under-top"] = t
                    break
            assert tag + "-under-top" in places
        host = cs.trie.plan(cs.sweep_cap, sweep=True)
        found = examined_part(host)
        assert found is not None, "no part with a wave of nodes of different widths, the widest no multiple of 8"
        d = host["desc"][found[0]]
        own = np.zeros(cs.V, bool)
        own[host["leaf_src"][d[6]:d[6] + d[7]]] = True
        outside = ~own
        assert outside.sum() > 256  # (every one of the 32 slack words gets tokens of other parts)
        places["outside-examined-part"] = int(np.nonzero(outside)[0][len(np.nonzero(outside)[0]) // 2])
        inside = np.ones(cs.nn, bool)  # the nodes with no token outside the examined part below them
        inside[cs.leaf[outside]] = False
        for n in range(cs.nn):  # (ascending ids: children first)
            if not inside[n] and cs.ref.parent[n] >= 0:
                inside[cs.ref.parent[n]] = False
        assert inside.sum() > own.sum()
    return places, own, inside


def check_hostile(cs, got, rows, info, op, what):
    B = rows.shape[0]
    folded = is_folded(what[0])
    want = cs.ref.reduce(rows, op, folded=folded)
    reducing = cs.internal[cs.ref.n_children[cs.internal] >= 2] if folded else cs.internal  # (the nodes with a value of their own)
    assert trie_ref.same_bits(got, want), (what, "row, node, got, want, differing:", trie_ref.first_difference(got, want))
    nan = np.isnan(got)
    for r, t in info["nan"]:
        if r >= B:
            continue
        path = np.zeros(cs.nn, bool)
        path[int(cs.leaf[t])] = True
        path[cs.ref.ancestors(cs.leaf[t]) if op == 0 else (cs.ref.chain(cs.leaf[t]) if folded else [])] = True
        assert np.array_equal(nan[r], path), (what, "a single NaN at token", t, "NaN at nodes", np.nonzero(nan[r] != path)[0][:8])
    for r in info["clean"]:
        assert r >= B or not nan[r].any(), (what, "NaN in a neighbouring row", r)
    for key in ("negative", "minus_zero"):
        r = info[key]
        if r < B and (op == 1 or key == "minus_zero"):
            assert (got[r, reducing].view(np.uint32) == 0).all(), (what, key, "not +0.0 at every internal node")
    r = info["tiny"]
    if r < B:
        tiny = trie_ref.palette(what[-1])["tiny"]
        assert got[r, cs.trie.root] == (np.float32(float(tiny) * cs.V) if op == 0 else tiny), (what, "subnormals flushed", got[r, cs.trie.root])
        assert (got[r] >= tiny).all()
    if "outside" in info and info["outside"][0] < B:
        r, inside = info["outside"]
        assert np.isfinite(got[r:r + 3][:, inside]).all(), (what, "another part's NaN / inf inside the examined part")


@pytest.mark.parametrize("kind", list(DTYPES))
@pytest.mark.parametrize("name", list(VOCABS) + list(DEGENERATE))
def test_hostile_weights(engine, name, kind):
    """C.  Weights (from_logprobs off), every form, sum and max, bit for bit against the reference on the upcast values; and
    said out loud: a single NaN shows at its leaf and, for sum, at exactly its ancestors - in no other node and no
    neighbouring row -, for max nowhere above the leaf; all negatives and all -0.0 leave +0.0 (max from +0 as the
    reference's max(0, ...); a sum that starts from +0); subnormals come back unflushed."""
    cs, dt, dev = case(name, engine), DTYPES[kind], engine.device
    for B in (1, 9, 70):
        rows, info = hostile_case(cs, kind, B)
        wd, back = rounded(rows, dt, dev)
        assert trie_ref.same_bits(back.astype(np.float32), rows)  # (the device holds the values the reference gets)
        for fname, call in case_forms(cs, engine, B):
            for op in (0, 1):
                check_hostile(cs, call(wd, op).cpu().numpy(), rows, info, op, (fname, B, op, kind))


@pytest.mark.parametrize("name", ["S", "W"])
def test_sweep_lanes_that_take_three_rows(engine, name):
    """The persistent sweep kernel with a lane that takes three rows and more (rows g, g + lanes, g + 2 lanes of lane g: the
    next row's head in flight during a reduction, the values read out before the next row lands on them): hostile weights
    and masses from logits, every output kind, the three element types."""
    cs, dev = case(name, engine), engine.device
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    for kind_of_plan, cap in (("sweep-parts", cs.sweep_cap), ("sweep-one", None)):
        n_parts = cs.trie.plan(cap, sweep=True)["n_parts"]
        B = max(2 * max(8, (cus // n_parts) & ~7) + 1, 45)  # (45: room for every deliberate row of `hostile_case`)
        assert -(-B // sweep_lanes(n_parts, B, cus)) >= 3
        for kind, dt in DTYPES.items():
            rows, info = hostile_case(cs, kind, B)
            wd, _ = rounded(rows, dt, dev)
            x, _ = wide_logits(np.random.default_rng(B), B, cs.V)
            xd, _ = rounded(x, dt, dev)
            lse = engine.step(xd, vocab=cs.V, rng_mode=0)[1]
            for fname, call in case_forms(cs, engine, B, (kind_of_plan,)):
                for op in (0, 1):
                    check_hostile(cs, call(wd, op).cpu().numpy(), rows, info, op, (fname, B, op, kind))
                check_structure(cs, call(xd, 0, True, lse), 0, (fname, B, "logits", kind))


@pytest.mark.parametrize("B", [31, 32, 33, 63, 64, 65])
def test_level_kernel_switches(engine, B):
    """D.  The level kernels at their switches: 32 rows (row-major below, node-major with the 64 x 64 transpose from there on;
    63 / 64 / 65: a full tile of rows and one more) and 256 output columns (the narrow / the wide untranspose, chosen by the
    number of columns alone): all nodes - 3599 of them, no multiple of 4: the wide kernel's partial last quad -, selections of
    1, 255, 256 and 257 ids with repeats, and the node-major layout.  Weights: the reference's bits; masses from logits: the
    bits of the row-major kernels on 9 rows at a time."""
    cs, dev = case("S", engine), engine.device
    assert cs.nn % 4 != 0
    flat = cs.trie.device_arrays()
    rs = np.random.default_rng(B)
    rows, _ = trie_ref.hostile_rows(cs.words, "float32", B, seed=B)
    x, _ = wide_logits(rs, B, cs.V)
    sels = [torch.from_numpy(np.concatenate([rs.integers(0, cs.nn, n - n // 2), rs.integers(0, 40, n // 2)]).astype(np.int32)).to(dev)
            for n in (1, 255, 256, 257)]
    for kind, dt in DTYPES.items():
        wd, wv = rounded(trie_ref.round_to(rows, kind), dt, dev)
        xd, _ = rounded(x, dt, dev)
        lse = engine.step(xd, vocab=cs.V, rng_mode=0)[1]
        small = [engine.trie_masses(xd[i:i + 9], flat, 0, True, lse=lse[i:i + 9]) for i in range(0, B, 9)]
        assert all(s.shape[0] < 32 for s in small)
        from_logits = torch.cat(small)
        for op in (0, 1):
            want = torch.from_numpy(cs.ref.reduce(wv.astype(np.float32), op)).to(dev)
            for src, flp, l, ref_rows in ((wd, False, None, want),) + (((xd, True, lse, from_logits),) if op == 0 else ()):
                got = engine.trie_masses(src, flat, op, flp, lse=l)
                assert torch.equal(_bits(got), _bits(ref_rows)) or trie_ref.same_bits(got.cpu().numpy(), ref_rows.cpu().numpy()), (B, kind, op, flp)
                for sel in sels:
                    g = engine.trie_masses(src, flat, op, flp, lse=l, nodes=sel)
                    assert trie_ref.same_bits(g.cpu().numpy(), ref_rows[:, sel.long()].cpu().numpy()), (B, kind, op, flp, sel.numel())
                nm = engine.trie_masses(src, flat, op, flp, lse=l, layout="nodes")
                assert nm.shape == (cs.nn, (B + 63) // 64 * 64)
                assert trie_ref.same_bits(nm[:, :B].t().contiguous().cpu().numpy(), ref_rows.cpu().numpy()), (B, kind, op, flp, "node-major")
    # ... and through the trie's own entry points with the resident kernels off
    from genlm_backend_amd.trie import TokenByteTrie

    off = TokenByteTrie(cs.trie.decode, engine=engine)
    off.resident = False
    xd, _ = rounded(x, torch.float32, dev)
    lse = engine.step(xd, vocab=cs.V, rng_mode=0)[1]
    want = torch.cat([engine.trie_masses(xd[i:i + 9], flat, 0, True, lse=lse[i:i + 9]) for i in range(0, B, 9)])
    assert torch.equal(_bits(off.masses_from_logits(xd, lse)), _bits(want))
    assert torch.equal(_bits(off.masses_from_logits(xd, lse, nodes=sels[2])), _bits(want[:, sels[2].long()]))
    for op in (0, 1):
        # (from 32 rows on `_batch` takes the folded trie)
        assert trie_ref.same_bits(off._batch(torch.from_numpy(rows), op, False).cpu().numpy(), cs.ref.reduce(rows, op, folded=B >= 32))


class Guarded:
    """Outputs of a pitch of width + 3 with a guard row before and after, prefilled with a sentinel."""

    def __init__(self, dev):
        self.dev, self.made = dev, []

    def __call__(self, shape):
        B, width = shape
        raw = torch.full((B + 2, width + 3), SENTINEL, dtype=torch.int32, device=self.dev)
        self.made.append((raw, B, width))
        return raw.view(torch.float32)[1:B + 1, :width]

    def check(self, what):
        assert self.made, what
        for raw, B, width in self.made:
            assert bool((raw[0] == SENTINEL).all()) and bool((raw[B + 1] == SENTINEL).all()), (what, "a guard row was written")
            assert bool((raw[:, width:] == SENTINEL).all()), (what, "the pad columns were written")


@pytest.mark.parametrize("kind", list(DTYPES))
@pytest.mark.parametrize("name", ["S", "W", "nested"])
def test_nothing_is_written_that_was_not_asked_for(engine, name, kind):
    """E.  Every form into outputs of a pitch of width + 3 (rows start on any word) between two guard rows: the pads and the
    guards keep the sentinel, the body holds what the unpitched call gives."""
    cs, dt, dev = case(name, engine), DTYPES[kind], engine.device
    rs = np.random.default_rng(55)
    for B in (1, 9, 70):
        wd, _ = rounded(rs.random((B, cs.V)), dt, dev)
        x, _ = wide_logits(rs, B, cs.V)
        xd, _ = rounded(x, dt, dev)
        lse = engine.step(xd, vocab=cs.V, rng_mode=0)[1]
        for fname, call in case_forms(cs, engine, B):
            for args in ((wd, 0), (wd, 1), (xd, 0, True, lse)):
                guard = Guarded(dev)
                got = call(*args, alloc=guard)
                torch.cuda.synchronize()
                guard.check((fname, B, kind, len(args)))
                assert torch.equal(_bits(got), _bits(call(*args))), (fname, B, kind, "pitched and unpitched results differ")


@pytest.mark.parametrize("name", ["S", "W"])
def test_selections_with_ids_outside_the_trie(engine, name):
    """E.  `glb_trie_rows` with selections that hold -1 and n_nodes: a shared selection leaves those columns untouched (the
    sentinel stays), a per-row selection writes 0.0 there; rows whose own selection is all -1 get zeros only; nothing
    beside the [B, K] body is written."""
    cs, dev = case(name, engine), engine.device
    rs = np.random.default_rng(66)
    B, K = 41, 37
    x, _ = wide_logits(rs, B, cs.V)
    xd, _ = rounded(x, torch.float32, dev)
    lse = engine.step(xd, vocab=cs.V, rng_mode=0)[1]
    shared = rs.integers(0, cs.nn, K).astype(np.int32)
    shared[[0, 5, K - 1]] = (-1, cs.nn, -1)
    shared[7] = cs.trie.root
    own = rs.integers(0, cs.nn, (B, K)).astype(np.int32)
    own[rs.random((B, K)) < 0.2] = -1
    own[rs.random((B, K)) < 0.05] = cs.nn
    own[3] = -1
    own[B - 1] = -1
    own[:, 2] = cs.trie.root  # (a node of the top: every part of the row is needed)
    own[3, 2] = own[B - 1, 2] = -1
    for tag, cap, sweep in (("gathered", cs.small_cap, False), ("gathered-one", ONE_PART_CAP, False),
                            ("sweep", cs.sweep_cap, True), ("sweep-one", None, True)):
        host = cs.trie.plan(cap, sweep=sweep)
        assert host["n_parts"] <= 62
        pl = cs.trie.plan_device_arrays(cap, sweep=sweep)
        for op in (0, 1):
            full = engine.trie_rows(xd, pl, op, True, lse=lse)
            # one selection for every row
            guard = Guarded(dev)
            got = guard((B, K))
            _trie_rows_into(engine, xd, pl, op, True, lse, 1.0, torch.from_numpy(shared).to(dev), out_sel=got)
            guard.check((tag, op, "shared"))
            inside = (shared >= 0) & (shared < cs.nn)
            assert bool((_bits(got)[:, torch.from_numpy(~inside).to(dev)] == SENTINEL).all()), (tag, op, "an id outside the trie was written")
            assert torch.equal(_bits(got[:, torch.from_numpy(inside).to(dev)]), _bits(full[:, torch.from_numpy(shared[inside]).long().to(dev)])), (tag, op)
            # a selection per row
            guard = Guarded(dev)
            got = guard((B, K))
            _trie_rows_into(engine, xd, pl, op, True, lse, 1.0, torch.from_numpy(own).to(dev), out_sel=got)
            guard.check((tag, op, "per row"))
            assert torch.equal(_bits(got), _bits(engine.trie_rows(xd, pl, op, True, lse=lse, nodes=torch.from_numpy(own).to(dev))))
            inside = (own >= 0) & (own < cs.nn)
            want = np.where(inside, full.cpu().numpy()[np.arange(B)[:, None], np.where(inside, own, 0)], np.float32(0.0))
            assert trie_ref.same_bits(got.cpu().numpy(), want.astype(np.float32)), (tag, op, trie_ref.first_difference(got.cpu().numpy(), want.astype(np.float32)))
            assert (got[3].cpu().numpy().view(np.uint32) == 0).all() and (got[B - 1].cpu().numpy().view(np.uint32) == 0).all()
