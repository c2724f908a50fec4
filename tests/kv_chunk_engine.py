"""Pure-Python restatement of glb_match_prefix_rows and glb_kv_plan_chunk (include/glb.h) and a `CpuOracleEngine` that
serves the three chunk methods on the CPU.  TEST INFRASTRUCTURE: lives under tests/, is never imported by the product
package.  The restatement is written from the header's text, row by row and group by group, with no regard for how the
kernels go about it."""
import asyncio

import numpy as np
import torch

from oracle import oracle as O
from tests.cpu_engine import CpuOracleEngine, _np


def match_prefix_rows(contexts, rep, n_groups, row_tok, row_len, max_new):
    """(old_row, keep, hash) per dedup group: the row with the longest shared prefix that leaves at most max_new tokens to
    feed; ties: a row that holds exactly the context, then the smallest row index."""
    R, cap = row_tok.shape
    old, keep, gh = np.full(n_groups, -1, np.int32), np.zeros(n_groups, np.int32), np.zeros(n_groups, np.uint64)
    for u in range(n_groups):
        c = [int(t) for t in contexts[rep[u]]]
        L = len(c)
        gh[u] = O.ctx_hash(c)
        if L > cap:
            continue
        best = None
        for r in range(R):
            rl = int(row_len[r])
            if rl <= 0:
                continue
            row = [int(t) for t in row_tok[r, :rl]]
            common = 0
            while common < min(rl, L) and row[common] == c[common]:
                common += 1
            k = min(common, L - 1)
            if k < 1 or L - k > max_new:
                continue
            key = (-k, 0 if row == c else 1, r)
            if best is None or key < best:
                best = key
        if best is not None:
            old[u], keep[u] = best[2], -best[0]
    return old, keep, gh


def kv_plan_chunk(group_of, rep, n_groups, old, old_keep, lengths, n_rows, cap, row_len, stamps=None, call_no=0):
    """glb_kv_plan_chunk's outputs as a dict of int32 arrays (`old`, `old_keep`: per GROUP; `row_len`: the table's lengths
    BEFORE the call); `stamps` is updated in place.  `n_valid`: how many leading entries of each output mean something."""
    n, U, R = len(group_of), int(n_groups), int(n_rows)
    L = [int(lengths[rep[u]]) for u in range(U)]
    o = []
    for u in range(U):
        ok = 0 <= int(old[u]) < R and L[u] <= cap and 0 <= int(old_keep[u]) <= L[u] - 1 and L[u] - int(old_keep[u]) <= 16
        o.append(int(old[u]) if ok else -1)
    keep = [int(old_keep[u]) if o[u] >= 0 else 0 for u in range(U)]
    # who keeps a matched row in place: the first group that may (the row holds at most keep + 1 tokens)
    keeper, matched = {}, set()
    for u in range(U):
        if o[u] >= 0:
            matched.add(o[u])
            if int(row_len[o[u]]) <= keep[u] + 1:
                keeper.setdefault(o[u], u)
    in_place = [u for u in range(U) if o[u] >= 0 and keeper.get(o[u]) == u]
    cand = [u for u in range(U) if o[u] >= 0 and keeper.get(o[u]) != u]
    fresh = [u for u in range(U) if o[u] < 0 and L[u] <= cap]
    free = [r for r in range(R) if r not in matched]  # (a matched row nobody keeps stays as it is: not free)
    if stamps is not None:
        free.sort(key=lambda r: (int(stamps[r]), r))
    grp_row = np.full(n, -1, np.int32)
    for u in in_place:
        grp_row[u] = o[u]
    for u, r in zip(cand + fresh, free):
        grp_row[u] = r
    has = [u for u in range(U) if o[u] >= 0 and grp_row[u] >= 0]
    one = [u for u in has if L[u] - keep[u] == 1]
    many = [u for u in has if L[u] - keep[u] > 1]
    in_b = [u for u in range(U) if u not in set(has)]
    out = {k: np.zeros(n, np.int32) for k in ("logits_row", "rows_a", "ctx_a", "pos_a", "n_new_a", "ctx_b", "rows_b")}
    out["group_row"] = grp_row
    out["copy_src"], out["copy_len"] = np.full(R, -1, np.int32), np.zeros(R, np.int32)
    out["ctx_of_row"], out["pos_of_row"] = np.full(R, -1, np.int32), np.zeros(R, np.int32)
    out["n_new_of_row"] = np.zeros(R, np.int32)
    copied = 0
    for k, u in enumerate(one + many):
        r = int(grp_row[u])
        out["logits_row"][u] = k
        out["rows_a"][k], out["ctx_a"][k], out["pos_a"][k], out["n_new_a"][k] = r, rep[u], keep[u], L[u] - keep[u]
        out["ctx_of_row"][r] = rep[u] if L[u] - keep[u] == 1 else -3
        out["pos_of_row"][r], out["n_new_of_row"][r] = keep[u], L[u] - keep[u]
        if r != o[u]:
            out["copy_src"][r], out["copy_len"][r] = o[u], keep[u]
            copied += 1
            if stamps is not None:
                stamps[o[u]] = call_no
    for k, u in enumerate(in_b):
        out["logits_row"][u] = len(has) + k
        out["ctx_b"][k], out["rows_b"][k] = rep[u], grp_row[u]
        if grp_row[u] >= 0:
            out["ctx_of_row"][grp_row[u]] = -2
    if stamps is not None:
        for u in range(U):
            if grp_row[u] >= 0:
                stamps[grp_row[u]] = call_no
    out["row_of_context"] = grp_row[np.asarray(group_of, np.int64)].astype(np.int32)
    out["head"] = np.array([U, len(has), len(in_b), copied, sum(1 for u in in_b if grp_row[u] < 0),
                            max([L[u] for u in in_b], default=0), len(free), 0, len(many),
                            max([L[u] - keep[u] for u in has], default=0)], np.int32)
    out["n_valid"] = dict(group_row=U, logits_row=U, rows_a=len(has), ctx_a=len(has), pos_a=len(has), n_new_a=len(has),
                          ctx_b=len(in_b), rows_b=len(in_b), row_of_context=n)
    return out


def write_table(out, U, rep, lengths, tokens, starts, group_hash, row_tok, row_len, row_hash):
    """The table rows of every group that holds a row now: the whole context, zero-padded (torch tensors, in place)."""
    for u in range(U):
        r = int(out["group_row"][u])
        if r >= 0:
            c = int(rep[u])
            L = int(lengths[c])
            row_tok[r] = 0
            row_tok[r, :L] = torch.from_numpy(np.ascontiguousarray(tokens[starts[c]:starts[c] + L]))
            row_len[r] = L
            row_hash[r] = int(group_hash[u])


class ChunkCpuEngine(CpuOracleEngine):
    """`CpuOracleEngine` with match_prefix_rows / kv_plan_chunk from the restatement above.  There is no attention kernel
    on the CPU: `slab_attention_chunk` is absent, so chunk forwards take the SDPA path with the explicit mask."""

    def kv_append(self, slab, new_rows, pos, rows=None):  # (glb_kv_append: a position outside the row appends nothing)
        n = new_rows.shape[0]
        r = torch.arange(n) if rows is None else rows.long()
        ok = (pos >= 0) & (pos < slab.shape[2])
        slab[r[ok], :, pos.long()[ok]] = new_rows[ok][:, :, 0]

    def match_prefix_rows(self, tokens, starts, lengths, rep, n_groups, row_tok, row_len, row_hash, max_new):
        ctxs = self._ctxs(tokens, starts, lengths)
        U = int(n_groups.item())
        old, keep, gh = match_prefix_rows(ctxs, _np(rep), U, _np(row_tok), _np(row_len), max_new)
        n = len(ctxs)
        old_f, keep_f, gh_f = np.full(n, -1, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint64)
        old_f[:U], keep_f[:U], gh_f[:U] = old, keep, gh
        # (the hashes the table keeps come from the engine's own hash, so that a test that makes every context collide
        # reaches the table too; the lookup above compares tokens and nothing else)
        gh_t = torch.from_numpy(gh_f.view(np.int64).copy())
        gh_t[:U] = self.hash_contexts(tokens, starts, lengths)[rep[:U].long()]
        return torch.from_numpy(old_f), torch.from_numpy(keep_f), gh_t

    def kv_plan_chunk(self, group_of, rep, n_groups, old_row, old_keep, lengths, n_rows, cap, stamps=None, call_no=0,
                      table=None):
        U = int(n_groups.item())
        row_tok, row_len, row_hash, group_hash, tokens, starts = table
        st = None if stamps is None else stamps.numpy()  # (updated in place)
        out = kv_plan_chunk(_np(group_of), _np(rep), U, _np(old_row)[:U], _np(old_keep)[:U], _np(lengths), n_rows, cap,
                            _np(row_len), stamps=st, call_no=call_no)
        out.pop("n_valid")
        write_table(out, U, _np(rep), _np(lengths), _np(tokens), _np(starts), _np(group_hash), row_tok, row_len, row_hash)
        return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}


# ---- the call sequence of the end-to-end tests ---------------------------------------------------------------------------
KINDS = ("grow", "repeat", "shrink-grow", "fork", "jump", "nowhere", "too-long")


def call_sequence(V, n_ctx=12, n_calls=14, cap=24, chunk=8, seed=11):
    """[(contexts, kinds)] per call: every context grows by 1 .. 5 tokens, is asked again, shrinks by 2 and grows by 3, is a
    fork of another context, jumps ahead by chunk + 1 tokens, comes from nowhere, or is longer than a row."""
    rnd = np.random.default_rng(seed)
    new = lambda k: [int(t) for t in rnd.integers(1, V, k)]
    ctxs = [new(int(rnd.integers(2, 6))) for _ in range(n_ctx)]
    calls = [(list(map(list, ctxs)), ["nowhere"] * n_ctx)]
    for _ in range(n_calls - 1):
        nxt, kinds = [], []
        for i, c in enumerate(ctxs):
            r = rnd.random()
            if len(c) > cap - 6:
                kind = "nowhere"
            elif r < 0.45:
                kind = "grow"
            elif r < 0.55:
                kind = "repeat"
            elif r < 0.65 and len(c) >= 3:
                kind = "shrink-grow"
            elif r < 0.75:
                kind = "fork"
            elif r < 0.85 and len(c) + chunk + 1 <= cap:
                kind = "jump"
            elif r < 0.93:
                kind = "nowhere"
            else:
                kind = "too-long"
            if kind == "grow":
                c2 = c + new(int(rnd.integers(1, 6)))
            elif kind == "repeat":
                c2 = list(c)
            elif kind == "shrink-grow":
                c2 = c[:-2] + new(3)
            elif kind == "fork":
                o = ctxs[int(rnd.integers(0, n_ctx))]
                c2 = o[:max(1, len(o) - int(rnd.integers(0, 3)))] + new(int(rnd.integers(1, 4)))
            elif kind == "jump":
                c2 = c + new(chunk + 1)
            elif kind == "nowhere":
                c2 = new(int(rnd.integers(1, 8)))
            else:
                c2 = new(cap + int(rnd.integers(1, 4)))
            nxt.append(c2)
            kinds.append(kind)
        ctxs = nxt
        calls.append((list(map(list, ctxs)), kinds))
    return calls


class ShadowTable:
    """The tests' own bookkeeping: a table of what the rows hold, kept beside the backend's and never read from it - every
    call's distinct contexts (in order of first occurrence, as the dedup orders its groups) go through the restatement of
    the matcher and the plan above.  `step` returns (head, tokens fed to rows that are fed more than one, the contexts
    that found no usable relative)."""

    def __init__(self, R, cap, chunk):
        self.R, self.cap, self.chunk, self.t = R, cap, chunk, 0
        self.row_tok, self.row_len = np.zeros((R, cap), np.int32), np.zeros(R, np.int32)
        self.stamps = np.zeros(R, np.int64)

    def held(self):
        return {tuple(int(t) for t in self.row_tok[r, :self.row_len[r]]) for r in range(self.R) if self.row_len[r] > 0}

    def step(self, ctxs):
        distinct = list(dict.fromkeys(tuple(c) for c in ctxs))
        U = len(distinct)
        old, keep, _ = match_prefix_rows(distinct, np.arange(U), U, self.row_tok, self.row_len, self.chunk)
        self.t += 1
        plan = kv_plan_chunk(np.arange(U), np.arange(U), U, old, keep, np.array([len(c) for c in distinct]), self.R, self.cap,
                             self.row_len, stamps=self.stamps, call_no=self.t)
        for u, c in enumerate(distinct):
            r = int(plan["group_row"][u])
            if r >= 0:
                self.row_tok[r] = 0
                self.row_tok[r, :len(c)] = c
                self.row_len[r] = len(c)
        fed = plan["n_new_of_row"]
        return plan["head"], int(fed[fed > 1].sum()), [c for u, c in enumerate(distinct) if old[u] < 0]


def run_sequence(make, V, tol, collide=False, R=10, cap=24, K=8):
    """The end-to-end check (shared with the GPU test): `make(**kw)` -> a backend.  Returns the chunk backend's stats."""
    plain, chunk, one = make(), make(auto_kv_rows=R, auto_kv_cap=cap, auto_kv_chunk=K), make(auto_kv_rows=R, auto_kv_cap=cap)
    if collide:
        for m in (chunk, one):
            eng = m.engine
            real = eng.hash_contexts
            eng.hash_contexts = lambda tok, st, ln, real=real: torch.full_like(real(tok, st, ln), 12345)
    calls = call_sequence(V, cap=cap, chunk=K)
    seen = set()
    want = dict(one_token_rows=0, chunk_rows=0, chunk_tokens=0, encoded_rows=0)
    rnd = np.random.default_rng(2)
    akv, shadow = chunk._auto_kv, ShadowTable(R, cap, K)
    for call, (ctxs, kinds) in enumerate(calls):
        seen.update(kinds)
        mids = [int(rnd.integers(0, 2)) for _ in ctxs]
        res = []
        for m in (plain, chunk, one):
            m.set_rng("torch", 77 + call)
            res.append(m.batch_next_token_step_sync(ctxs, mids))
        (z0, t0) = res[0]
        fin = np.isfinite(z0)
        for z, t in res[1:]:
            assert np.array_equal(fin, np.isfinite(z)) and np.abs(z0[fin] - z[fin]).max() < tol, call
            assert np.array_equal(t0, t), call
        # the test's own bookkeeping (a shadow table, never read from the backend's): rows of each kind, and that only
        # contexts that jumped, came from nowhere or are too long - or whose predecessor found no row in the call before
        # (twelve contexts, ten rows) - are without a usable relative
        before = shadow.held()
        head, fed, alone = shadow.step(ctxs)
        want["one_token_rows"] += int(head[1] - head[8])
        want["chunk_rows"] += int(head[8])
        want["chunk_tokens"] += fed
        want["encoded_rows"] += int(head[2])
        for c in alone:
            for i, (cc, k) in enumerate(zip(ctxs, kinds)):
                if call and len(c) > 1 and tuple(cc) == c and k in ("grow", "repeat", "shrink-grow"):
                    assert tuple(calls[call - 1][0][i]) not in before, (call, c, k)
        # ... and the backend's table holds what the shadow holds, row by row
        assert np.array_equal(akv.row_len.cpu().numpy(), shadow.row_len), call
        assert np.array_equal(akv.row_tok.cpu().numpy(), shadow.row_tok), call
        assert {k: akv.stats[k] for k in want} == want, (call, akv.stats, want)
    assert seen == set(KINDS), set(KINDS) - seen  # a sequence that misses a kind hides a failure
    got = {k: akv.stats[k] for k in want}
    assert got == want, (got, want)
    assert got["chunk_rows"] > 0 and got["chunk_tokens"] > 2 * got["chunk_rows"] - 1 and got["encoded_rows"] > 0
    assert one._auto_kv.stats["chunk_rows"] == 0 and one._auto_kv.stats["chunk_tokens"] == 0
    assert one._auto_kv.stats["encoded_rows"] > got["encoded_rows"]  # (what the parent re-encodes, chunks serve)
    # the queued log-prob path goes through the same rows: one more growth by 1 .. 3 tokens, rows against the plain backend
    ctxs = [c + [int(t) for t in rnd.integers(1, V, int(rnd.integers(1, 4)))] for c in calls[-1][0] if len(c) + 3 <= cap]
    rows = [asyncio.run(m.batch_next_token_logprobs(ctxs)) for m in (plain, chunk, one)]
    for a, b, c in zip(*rows):
        assert (a.float() - b.float()).abs().max().item() < tol and (a.float() - c.float()).abs().max().item() < tol
    return akv.stats
