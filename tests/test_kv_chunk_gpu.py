"""glb_match_prefix_rows, glb_kv_plan_chunk and glb_slab_attention_chunk on the MI355X against the pure-Python restatement
(tests/kv_chunk_engine.py), the one-token kernels they extend and torch; then auto_kv_chunk end to end."""
import ast
import os

import numpy as np
import pytest
import torch

from tests import synth
from tests.kv_chunk_engine import call_sequence, kv_plan_chunk, match_prefix_rows, run_sequence

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden", "ref_hotpath_tiny.npz")
TOL = 1e-4  # (tests/test_host_gpu.py)
R_T, CAP_T = 24, 12


class Tok:
    pad_token_id = None
    eos_token_id = 0


def _planted(seed):
    """<= 64 distinct contexts (lengths up to cap + 2) and a table of 24 rows planted with their relatives: parents, exact
    holders, siblings, longer rows, grandparents (keep = L - 3), each with an impostor beside it - the same hash and length,
    other tokens.  Returns (contexts, row_tok, row_len, row_hash, kinds planted)."""
    from oracle import oracle as O

    rnd = np.random.default_rng(seed)
    ctxs = [list(map(int, c)) for c in synth.contexts(seed, 64, 40, lo=1, hi=CAP_T + 2)]
    ctxs = [c for c in ctxs if len(c) >= 1]
    row_tok, row_len = np.zeros((R_T, CAP_T), np.int32), np.zeros(R_T, np.int32)
    row_hash = np.zeros(R_T, np.uint64)
    kinds, r = [], 0
    order = ["parent", "exact", "sibling", "longer", "grandparent"]
    usable = [c for c in ctxs if 4 <= len(c) <= CAP_T - 2]
    for k, c in zip(order * 3, usable):
        if r + 2 > R_T - 2:  # (two rows stay empty)
            break
        row = dict(parent=c[:-1], exact=list(c), sibling=c[:-1] + [c[-1] % 40 + 1], longer=c + [3, 5],
                   grandparent=c[:-3])[k]
        imp = list(row)
        imp[0] = imp[0] % 40 + 1  # other tokens from the first one on ...
        for rr, t, h in ((r, imp, row), (r + 1, row, row)):  # ... under the real row's hash, in the SMALLER row index
            row_tok[rr, :len(t)], row_len[rr], row_hash[rr] = t, len(t), O.ctx_hash(h)
        kinds.append(k)
        r += 2
    return ctxs, row_tok, row_len, row_hash, kinds


def _dev(engine, *arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(engine.device) for a in arrs]


@pytest.fixture(scope="module")
def planted(engine, oracle):
    ctxs, row_tok, row_len, row_hash, kinds = _planted(3)
    tok, st, ln = oracle.ragged(ctxs)
    g_o, rep_o, ng_o = oracle.group_contexts(ctxs)
    tok_d, st_d, ln_d = _dev(engine, tok, st, ln)
    g, rep, ng = engine.group_contexts(tok_d, st_d, ln_d)
    assert int(ng.item()) == ng_o and np.array_equal(rep.cpu().numpy()[:ng_o], rep_o)
    return dict(ctxs=ctxs, row_tok=row_tok, row_len=row_len, row_hash=row_hash, kinds=kinds, tok=tok, st=st, ln=ln, g_o=g_o,
                rep_o=rep_o, ng_o=ng_o, tok_d=tok_d, st_d=st_d, ln_d=ln_d, g=g, rep=rep, ng=ng)


@pytest.mark.parametrize("max_new", [1, 3, 16])
def test_match_prefix_rows_equals_the_restatement(engine, planted, max_new):
    p = planted
    assert set(p["kinds"]) == {"parent", "exact", "sibling", "longer", "grandparent"}  # a list that misses a kind hides a failure
    want_old, want_keep, want_h = match_prefix_rows(p["ctxs"], p["rep_o"], p["ng_o"], p["row_tok"], p["row_len"], max_new)
    rt, rl, rh = _dev(engine, p["row_tok"], p["row_len"], p["row_hash"].view(np.int64))
    old, keep, gh = engine.match_prefix_rows(p["tok_d"], p["st_d"], p["ln_d"], p["rep"], p["ng"], rt, rl, rh, max_new)
    U = p["ng_o"]
    assert np.array_equal(old.cpu().numpy()[:U], want_old)
    assert np.array_equal(keep.cpu().numpy()[:U], want_keep)
    assert np.array_equal(gh.cpu().numpy()[:U].view(np.uint64), want_h)
    L = np.array([len(p["ctxs"][i]) for i in p["rep_o"][:U]])
    hit = want_old >= 0
    assert hit.any() and (~hit).any() and (L > CAP_T).any() and not hit[L > CAP_T].any()
    assert not (want_old[hit] % 2 == 0).any()  # no impostor (they sit in the even rows) ever wins
    if max_new == 3:
        assert (L[hit] - want_keep[hit] == 3).any() and (L[hit] - want_keep[hit] == 1).any()
        # an exact holder and a longer row tie on keep = L - 1 somewhere: the exact holder must have won there
        assert any(p["row_len"][o] == l and k == l - 1 for o, k, l in zip(want_old[hit], want_keep[hit], L[hit]))
        assert any(p["row_len"][o] > l for o, l in zip(want_old[hit], L[hit]))


def _plan_both(engine, oracle, ctxs, row_tok, row_len, row_hash, old, keep, stamps, call_no, R, cap):
    """(device outputs, restatement) of glb_kv_plan_chunk on one input; the tables after the call are compared too."""
    tok, st, ln = oracle.ragged(ctxs)
    g_o, rep_o, ng_o = oracle.group_contexts(ctxs)
    n = len(ctxs)
    rep_f = np.concatenate([rep_o, np.zeros(n - ng_o, np.int32)]).astype(np.int32)
    st_w = stamps.copy()
    want = kv_plan_chunk(g_o, rep_f, ng_o, old, keep, ln, R, cap, row_len, stamps=st_w, call_no=call_no)
    gh = np.array([oracle.ctx_hash(ctxs[rep_o[u]]) for u in range(ng_o)] + [0] * (n - ng_o), np.uint64)
    tok_d, st_d, ln_d, g_d, rep_d = _dev(engine, tok, st, ln, g_o.astype(np.int32), rep_f)
    ng_d = torch.tensor([ng_o], dtype=torch.int32, device=engine.device)
    pad = lambda a, fill: np.concatenate([a, np.full(n - len(a), fill, a.dtype)])
    old_d, keep_d, gh_d, rt, rl, rh, st_g = _dev(engine, pad(old.astype(np.int32), -1), pad(keep.astype(np.int32), 0),
                                                  gh.view(np.int64), row_tok, row_len, row_hash.view(np.int64), stamps)
    got = engine.kv_plan_chunk(g_d, rep_d, ng_d, old_d, keep_d, ln_d, R, cap, stamps=st_g, call_no=call_no,
                               table=(rt, rl, rh, gh_d, tok_d, st_d))
    torch.cuda.synchronize()
    assert got["head"].cpu().tolist() == want["head"].tolist()
    for k, cnt in want["n_valid"].items():
        assert np.array_equal(got[k].cpu().numpy()[:cnt], want[k][:cnt]), k
    for k in ("copy_src", "copy_len", "ctx_of_row", "pos_of_row", "n_new_of_row"):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    assert np.array_equal(st_g.cpu().numpy(), st_w)
    rt_h, rl_h = rt.cpu().numpy(), rl.cpu().numpy()
    for u in range(ng_o):
        r = want["group_row"][u]
        if r >= 0:
            c = ctxs[rep_o[u]]
            assert rl_h[r] == len(c) and list(rt_h[r, :len(c)]) == c and not rt_h[r, len(c):].any()
    held = set(int(r) for r in want["group_row"][:ng_o] if r >= 0)
    for r in range(R):  # rows nobody holds now are as they were (a pinned long row among them)
        if r not in held:
            assert rl_h[r] == row_len[r] and np.array_equal(rt_h[r], row_tok[r])
    return got, want, (g_d, rep_d, ng_d, old_d, ln_d, tok_d, st_d, gh_d)


@pytest.mark.parametrize("max_new", [3, 16])
def test_kv_plan_chunk_equals_the_restatement(engine, oracle, planted, max_new):
    p = planted
    old, keep, _ = match_prefix_rows(p["ctxs"], p["rep_o"], p["ng_o"], p["row_tok"], p["row_len"], max_new)
    stamps = np.random.default_rng(1).integers(0, 5, R_T).astype(np.int64)
    got, want, _ = _plan_both(engine, oracle, p["ctxs"], p["row_tok"], p["row_len"], p["row_hash"], old, keep, stamps, 9, R_T, CAP_T)
    h = want["head"]
    # rows of every kind, copies, more groups than free rows (the last ones are encoded and not kept), a pinned long row
    assert h[1] - h[8] > 0 and h[8] > 0 and h[2] > 0 and h[3] > 0 and h[4] > 0 and 1 < h[9] <= max_new
    assert any(p["row_len"][o] > k + 1 for o, k in zip(old, keep) if o >= 0)


def test_kv_plan_chunk_hand_made_cases(engine, oracle):
    cap, R = 8, 5
    rows = [[1, 2, 3, 4, 5, 6], [9, 9], [], [], []]
    row_tok, row_len = np.zeros((R, cap), np.int32), np.array([len(r) for r in rows], np.int32)
    for r, t in enumerate(rows):
        row_tok[r, :len(t)] = t
    row_hash = np.array([oracle.ctx_hash(r) for r in rows], np.uint64)
    z = np.zeros(R, np.int64)
    # two groups match row 0 with different keep; the first may keep it in place (the row holds keep + 1 = 6 tokens), the
    # second copies ITS OWN 4 tokens
    ctxs = [[1, 2, 3, 4, 5, 7, 7], [1, 2, 3, 4, 8]]
    old, keep, _ = match_prefix_rows(ctxs, np.arange(2), 2, row_tok, row_len, 4)
    assert old.tolist() == [0, 0] and keep.tolist() == [5, 4]
    got, want, _ = _plan_both(engine, oracle, ctxs, row_tok, row_len, row_hash, old, keep, z, 1, R, cap)
    assert want["group_row"][:2].tolist() == [0, 1] and (want["copy_src"][1], want["copy_len"][1]) == (0, 4)
    assert want["n_new_a"][:2].tolist() == [1, 2] and want["rows_a"][:2].tolist() == [1, 0]  # the one-token row comes first
    # a group that matches a row longer than keep + 1 must copy: the long row is never truncated, and is not free
    ctxs = [[1, 2, 3, 7]]
    old, keep, _ = match_prefix_rows(ctxs, np.arange(1), 1, row_tok, row_len, 4)
    got, want, _ = _plan_both(engine, oracle, ctxs, row_tok, row_len, row_hash, old, keep, z, 1, R, cap)
    assert (old[0], keep[0]) == (0, 3) and want["group_row"][0] == 1 and want["copy_src"][1] == 0 and want["head"][6] == 4
    # no free row: every row is matched and pinned, so the groups are encoded and nobody keeps them
    full = np.array([[1, 2, 3, 4, 5, 6, 0, 0], [2, 2, 3, 4, 5, 6, 0, 0]], np.int32)
    ctxs = [[1, 2, 3, 9], [2, 2, 3, 9], [5, 5]]
    old, keep, _ = match_prefix_rows(ctxs, np.arange(3), 3, full, np.array([6, 6], np.int32), 4)
    got, want, _ = _plan_both(engine, oracle, ctxs, full, np.array([6, 6], np.int32),
                              np.array([oracle.ctx_hash(list(r[:6])) for r in full], np.uint64), old, keep, z[:2], 1, 2, cap)
    assert want["group_row"][:3].tolist() == [-1, -1, -1] and want["head"].tolist()[:7] == [3, 0, 3, 0, 3, 4, 0]


def test_kv_plan_chunk_with_parents_and_exact_holders_equals_kv_plan(engine, oracle):
    """keep = L - 1 everywhere and matched rows of L - 1 or L tokens: every output glb_kv_plan has is identical."""
    rnd = np.random.default_rng(8)
    cap, R = 10, 16
    base = [list(map(int, rnd.integers(1, 30, int(rnd.integers(1, 8))))) for _ in range(10)]
    rows = base[:8] + [base[0], []] + [list(map(int, rnd.integers(1, 30, 4))) for _ in range(6)]
    ctxs = [b + [int(rnd.integers(1, 30))] for b in base] + [list(base[1]), list(base[2]), base[0] + [7], base[0] + [8]]
    ctxs += [list(map(int, rnd.integers(1, 30, 12))), [4]] + [list(c) for c in ctxs[:5]]
    row_tok, row_len = np.zeros((R, cap), np.int32), np.array([len(r) for r in rows], np.int32)
    for r, t in enumerate(rows):
        row_tok[r, :len(t)] = t
    row_hash = np.array([oracle.ctx_hash(r) for r in rows], np.uint64)
    tok, st, ln = oracle.ragged(ctxs)
    g_o, rep_o, ng_o = oracle.group_contexts(ctxs)
    old_w, _ = oracle.match_rows(ctxs, rep_o, ng_o, row_tok, row_len, row_hash)
    assert (old_w >= 0).sum() >= 10 and (old_w < 0).any()
    keep = np.array([len(ctxs[rep_o[u]]) - 1 for u in range(ng_o)], np.int32)
    stamps = rnd.integers(0, 4, R).astype(np.int64)
    got, want, (g_d, rep_d, ng_d, old_d, ln_d, tok_d, st_d, gh_d) = _plan_both(engine, oracle, ctxs, row_tok, row_len, row_hash,
                                                                              old_w, keep, stamps, 5, R, cap)
    rt, rl, rh, st_g = _dev(engine, row_tok, row_len, row_hash.view(np.int64), stamps)
    ref = engine.kv_plan(g_d, rep_d, ng_d, old_d, ln_d, R, cap, stamps=st_g, call_no=5, table=(rt, rl, rh, gh_d, tok_d, st_d))
    torch.cuda.synchronize()
    for k, v in ref.items():  # (entries past the number of groups / forward rows are unspecified in both)
        cnt = want["n_valid"].get(k, v.numel())
        assert torch.equal(v[:cnt], got[k][:cnt]), k
    assert got["head"][8].item() == 0 and got["head"][9].item() == 1 and ref["head"][3].item() > 0


_REF = {}


@pytest.mark.parametrize("T", [1, 2, 5, 16])
@pytest.mark.parametrize("H,Hkv", [(4, 2), (3, 3)])
@pytest.mark.parametrize("Dh", [64, 128])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_slab_attention_chunk(engine, dtype, Dh, H, Hkv, T):
    dev, n, cap = engine.device, 5, 33
    g = torch.Generator(device=dev)
    g.manual_seed(Dh + H + T)
    ks = torch.randn((n, Hkv, cap, Dh), device=dev, generator=g).to(dtype)
    vs = torch.randn((n, Hkv, cap, Dh), device=dev, generator=g).to(dtype)
    nn = torch.tensor([T, 1, max(1, T // 2), T, 1], dtype=torch.int32, device=dev)
    pos = torch.tensor([0, 7, cap - max(1, T // 2), cap - T, 20], dtype=torch.int32, device=dev)  # pos = 0; pos + n_new = cap twice
    proj = torch.randn((n, T, (H + 2 * Hkv) * Dh), device=dev, generator=g).to(dtype)  # q | k | v of one projection
    q = proj[..., :H * Dh].view(n, T, H, Dh).transpose(1, 2)
    kn = proj[..., H * Dh:(H + Hkv) * Dh].view(n, T, Hkv, Dh).transpose(1, 2)
    vn = proj[..., (H + Hkv) * Dh:].view(n, T, Hkv, Dh).transpose(1, 2)
    scale = Dh ** -0.5
    # T successive one-token calls on clones: rows that have no token t left ride along at a position that is discarded
    k1, v1 = ks.clone(), vs.clone()
    want = torch.zeros((n, T, H, Dh), dtype=dtype, device=dev)
    for t in range(T):
        live = nn > t
        kt, vt = k1.clone(), v1.clone()
        o = engine.slab_attention(q[:, :, t:t + 1], kn[:, :, t:t + 1], vn[:, :, t:t + 1], kt, vt,
                                  torch.where(live, pos + t, torch.zeros_like(pos)), scale)
        want[live, t] = o[live, 0]
        k1[live], v1[live] = kt[live], vt[live]
    k2, v2 = ks.clone(), vs.clone()
    out = engine.slab_attention_chunk(q, kn, vn, k2, v2, pos, nn, scale)
    torch.cuda.synchronize()
    assert out.shape == (n, T, H, Dh) and out.dtype == dtype
    assert torch.equal(out, want) and torch.equal(k2, k1) and torch.equal(v2, v1)  # the bits of successive one-token calls
    # float32 torch softmax on the same values; zeros behind a row's last token; slabs untouched outside the appended positions
    tol = 2e-5 if dtype == torch.float32 else (2e-2 if dtype == torch.bfloat16 else 3e-3)
    k_ref, v_ref = ks.clone(), vs.clone()
    for r in range(n):
        for t in range(int(nn[r])):
            k_ref[r, :, int(pos[r]) + t], v_ref[r, :, int(pos[r]) + t] = kn[r, :, t], vn[r, :, t]
    assert torch.equal(k2, k_ref) and torch.equal(v2, v_ref)
    Gq = H // Hkv
    kf, vf = k_ref.float().repeat_interleave(Gq, dim=1), v_ref.float().repeat_interleave(Gq, dim=1)
    sc = torch.einsum("rhtd,rhpd->rhtp", q.float(), kf) * scale
    last = pos[:, None] + torch.arange(T, device=dev)[None, :]
    sc = sc.masked_fill(torch.arange(cap, device=dev)[None, None, None, :] > last[:, None, :, None], float("-inf"))
    ref = torch.einsum("rhtp,rhpd->rthd", torch.softmax(sc, -1), vf)
    valid = torch.arange(T, device=dev)[None, :] < nn[:, None]
    print(f"max |chunk - torch| = {(out.float() - ref)[valid].abs().max().item():.3e} (bound {tol})")
    assert (out.float() - ref)[valid].abs().max().item() < tol
    assert not out[~valid].float().any() if (~valid).any() else True
    # a chunk outside its row: NaN for that row, nothing appended, the other rows unchanged
    bad = pos.clone()
    bad[1], bad[2] = -1, cap - int(nn[2]) + 1
    k3, v3 = ks.clone(), vs.clone()
    out3 = engine.slab_attention_chunk(q, kn, vn, k3, v3, bad, nn, scale)
    torch.cuda.synchronize()
    assert torch.isnan(out3[1].float()).all() and torch.isnan(out3[2].float()).all()
    assert torch.equal(out3[[0, 3, 4]], out[[0, 3, 4]])
    assert torch.equal(k3[[1, 2]], ks[[1, 2]]) and torch.equal(v3[[1, 2]], vs[[1, 2]])
    assert torch.equal(k3[[0, 3, 4]], k2[[0, 3, 4]]) and torch.equal(v3[[0, 3, 4]], v2[[0, 3, 4]])
    # rows anywhere in a larger slab (row_of): the same bits in the rows named, nothing else touched
    big_k, big_v = torch.zeros((n + 3, Hkv, cap, Dh), dtype=dtype, device=dev), torch.zeros((n + 3, Hkv, cap, Dh), dtype=dtype, device=dev)
    rows = torch.tensor([6, 0, 3, 7, 2], dtype=torch.int32, device=dev)
    big_k[rows.long()], big_v[rows.long()] = ks, vs
    out4 = engine.slab_attention_chunk(q, kn, vn, big_k, big_v, pos, nn, scale, rows=rows)
    assert torch.equal(out4, out) and torch.equal(big_k[rows.long()], k2) and torch.equal(big_v[rows.long()], v2)
    assert not big_k[[1, 4, 5]].any() and not big_v[[1, 4, 5]].any()
    # one replay from a captured graph: the same bits
    k5, v5 = ks.clone(), vs.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        engine.slab_attention_chunk(q, kn, vn, k5.clone(), v5.clone(), pos, nn, scale)  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out5 = engine.slab_attention_chunk(q, kn, vn, k5, v5, pos, nn, scale)
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(out5, out) and torch.equal(k5, k2) and torch.equal(v5, v2)


@pytest.fixture(scope="module")
def gold():
    return np.load(G)


@pytest.mark.parametrize("collide", [False, True])
def test_chunk_rows_match_a_backend_without_rows_on_the_gpu(engine, gold, collide):
    from transformers import GPT2Config, GPT2LMHeadModel

    from genlm_backend_amd.engine import HipEngine
    from genlm_backend_amd.llm import AsyncAmdLM

    cfg = ast.literal_eval(bytes(gold["config_json"]).decode())

    def make(**kw):
        model = GPT2LMHeadModel(GPT2Config(**cfg)).eval()
        model.load_state_dict({k[3:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("w::")})
        # (an engine of its own: `collide` replaces a method of it)
        m = AsyncAmdLM(model.to(engine.device), None, batch_size=64, timeout=0.02, engine=HipEngine("cuda:0", contract="poly"), **kw)
        m.tokenizer = Tok()
        m.register_masks(torch.from_numpy(gold["sis_masks"]))
        return m

    stats = run_sequence(make, cfg["vocab_size"], TOL, collide=collide)
    print("auto_kv_chunk=8 stats:", stats)


def _llama(dtype, device):
    from transformers import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=160, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, head_dim=64, max_position_embeddings=64)
    return LlamaForCausalLM(cfg).eval().to(dtype).to(device)


@pytest.mark.parametrize("glb_attention", [True, False])
def test_llama_shaped_bf16_chunk_rows_deviate_no_more_than_re_encoding(engine, glb_attention):
    """Each served path's largest deviation from the float32 model's log-prob rows (CPU): the chunk path's may be at most
    1.5 x that of the re-encoding bfloat16 path on the same contexts (chunk rows and re-encoded rows round through
    different GEMM shapes).  glb_attention=False: the SDPA path with the explicit mask."""
    from genlm_backend_amd.kv import ragged
    from genlm_backend_amd.llm import AsyncAmdLM

    ref = _llama(torch.float32, "cpu")
    bf = _llama(torch.float32, "cpu").to(torch.bfloat16).to(engine.device)

    def make(**kw):
        m = AsyncAmdLM(bf, None, batch_size=64, timeout=0.02, engine=engine, glb_attention=glb_attention, **kw)
        m.tokenizer = Tok()
        return m

    plain, chunk = make(), make(auto_kv_rows=10, auto_kv_cap=24, auto_kv_chunk=8)
    # largest deviation per served path (rows fed a chunk, rows fed one token, rows encoded by the chunk backend) and, for
    # the contexts of each path, that of the re-encoding backend
    dev = {k: [0.0, 0.0] for k in ("chunk", "one-token", "encoded")}
    with torch.no_grad():
        for call, (ctxs, _) in enumerate(call_sequence(160, n_ctx=8, n_calls=8)):
            want = torch.stack([torch.log_softmax(ref(torch.tensor([c])).logits[0, -1].float(), -1) for c in ctxs])
            rows_p = torch.stack([plain.next_token_logprobs_uncached(c).float().cpu() for c in ctxs])
            tok_d, st_d, ln_d = (torch.from_numpy(a).to(engine.device) for a in ragged(ctxs))
            g_of, rep, ng = engine.group_contexts(tok_d, st_d, ln_d)
            logits, row_of_group, _, U, _ = chunk._auto_kv.logits(tok_d, st_d, ln_d, g_of, rep, ng)
            _, counts, (n_chunk, _) = chunk._auto_kv.last
            k_of = row_of_group[g_of.long()].long().cpu()  # the logits row that serves every context
            rows_c = torch.log_softmax(logits.float(), -1).cpu()[k_of]
            n_a = counts[1]  # (forward rows: the ones fed one token, the ones fed a chunk, the encoded ones)
            path = ["one-token" if k < n_a - n_chunk else ("chunk" if k < n_a else "encoded") for k in k_of.tolist()]
            for i, p in enumerate(path):
                dev[p][0] = max(dev[p][0], (rows_c[i] - want[i]).abs().max().item())
                dev[p][1] = max(dev[p][1], (rows_p[i] - want[i]).abs().max().item())
    st = chunk._auto_kv.stats
    print(f"llama-shaped bf16, glb_attention={glb_attention}: max |log-prob - float32| per served path, rows / re-encoding "
          "of the same contexts: " + "; ".join(f"{k} {a:.4e} / {b:.4e} (ratio {a / b:.3f})" for k, (a, b) in dev.items())
          + f"; stats {st}")
    assert st["chunk_rows"] > 0 and st["one_token_rows"] > 0 and all(b > 0 for _, b in dev.values())
    assert dev["chunk"][0] <= 1.5 * dev["chunk"][1]


def test_one_token_calls_still_replay_the_graph_after_chunk_calls(engine, gold):
    from transformers import GPT2Config, GPT2LMHeadModel

    from genlm_backend_amd.llm import AsyncAmdLM

    cfg = ast.literal_eval(bytes(gold["config_json"]).decode())
    model = GPT2LMHeadModel(GPT2Config(**cfg)).eval()
    model.load_state_dict({k[3:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("w::")})
    model = model.to(engine.device)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    impl = model.config._attn_implementation
    V = cfg["vocab_size"]

    def make(**kw):
        m = AsyncAmdLM(model, None, batch_size=64, timeout=0.02, engine=engine, **kw)
        m.tokenizer = Tok()
        return m

    plain, m = make(), make(auto_kv_rows=8, auto_kv_cap=24, auto_kv_chunk=4)
    rnd = np.random.default_rng(4)
    ctxs = [[int(t) for t in rnd.integers(1, V, 3)] for _ in range(8)]
    for grow in (0, 3, 1, 1, 1, 1, 2, 1):
        ctxs = [c + [int(t) for t in rnd.integers(1, V, grow)] for c in ctxs]
        z0, _ = plain.batch_next_token_step_sync(ctxs, [0] * 8)
        z1, _ = m.batch_next_token_step_sync(ctxs, [0] * 8)
        assert np.abs(z0 - z1).max() < TOL, grow
    st = m._auto_kv.stats
    assert st["chunk_rows"] == 16 and st["chunk_tokens"] == 40 and st["one_token_rows"] == 40 and st["in_place_calls"] == 5
    fwd = m._auto_kv._slab_fwd
    assert fwd.fused and fwd.calls == 5 and len(fwd.graphs) == 1  # the third one-token call captured, the later ones replay
    assert impl == model.config._attn_implementation
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
