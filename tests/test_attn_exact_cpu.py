"""tests/attn_exact_ref.py on the CPU: every condition tests/test_attn_exact_gpu.py relies on, shown from the reference alone
for every case that test launches - the selector's gap, exactness of every operand in the three element types, distinct V
rows, who sees nothing, and that the kernels' tile-wise online softmax, restated in float32, meets the expected outputs (bit
for bit / within the derived bound) while three deliberately broken restatements do not."""
import pytest
import torch

from tests import attn_exact_ref as X


def check_flat(flat, expected, rows_differ=True):
    """The conditions of one generated case; AssertionError names the one that fails.  Returns the number of queries."""
    q, k, v, see = flat.q, flat.k.nan_to_num(0.0), flat.v.nan_to_num(0.0), flat.see
    # who sees nothing: exactly the listed queries (and the queries that do not exist)
    assert torch.equal(~see.any(-1), flat.blind | ~flat.valid), "a query sees nothing that is not listed (or a listed one sees)"
    live = see.any(-1)
    # every operand exact in bfloat16 and float16, float16 in range; scores and V sums exact integers in float32
    for name, x in (("q", q), ("k", k), ("v", v)):
        for dt in (torch.bfloat16, torch.float16):
            assert torch.equal(x.to(dt).float(), x), f"{name} does not survive {dt}"
        assert x.abs().max().item() < 65504, name
    out64, sc = X.attention_f64(flat)
    assert sc.abs().max().item() < 2 ** 24 and torch.equal(sc, sc.round())
    assert v.abs().sum(2).max().item() < 2 ** 24
    # V rows: pairwise distinct over every (row, KV head, key some query sees)
    # (rows_differ: over the rows of the batch too; packed segments share their prompt's rows)
    seen_key = see.any(1)[:, None, :].expand(v.shape[:3])
    for rows in ([v[seen_key]] if rows_differ else [v[r][seen_key[r]] for r in range(len(v))]):
        assert len(torch.unique(rows, dim=0)) == len(rows), "two visible keys share a V row"
    if flat.family == "selector":
        top = sc.masked_fill(~see[:, None], float("-inf")).topk(min(2, sc.shape[-1]), -1).values  # [R, H, Lq, 2]
        if top.shape[-1] == 2:
            gap = (top[..., 0] - top[..., 1])[live[:, None].expand(top.shape[:3])]
            assert gap.min().item() >= 128, f"winner only {gap.min().item()} above the runner-up"
        assert torch.equal(out64, expected), "float64 attention is not V[winner]"  # (1 + 2.6e-56 rounds to 1)
    else:
        assert (out64 - expected).abs().max().item() < 1e-12
    # the kernels' arithmetic, restated: the same bits / inside the bound
    for dt in X.DTYPES:
        ok, rel, bound = X.compare(X.emulate_tiles(flat, dt).to(dt), expected, flat.family, dt)
        assert ok, f"the tile-wise online softmax misses the expected output in {dt}: {rel:.3e} (bound {bound:.3e})"
    return int(live.sum()) * q.shape[1]


def _slab_flats(T, H, Hkv, Dh):
    for fam in X.FAMILIES:
        c = X.slab_case(*fam, T, H, Hkv, Dh)
        yield fam, c.flat, c.expected, c


@pytest.mark.parametrize("H,Hkv", X.HEADS)
@pytest.mark.parametrize("T,dims", [(T, X.TILE_DIMS) for T in X.TILE_T] + [(T, X.WAVE_DIMS) for T in X.CHUNK_T])
def test_slab_cases(T, dims, H, Hkv):
    n = 0
    for Dh in dims:
        for fam, flat, expected, c in _slab_flats(T, H, Hkv, Dh):
            n += check_flat(flat, expected)
            # the poison: NaN exactly at slab positions >= pos and new positions >= n_new; the slab afterwards = before + new
            s, t = torch.arange(X.CAP)[None, :], torch.arange(T)[None, :]
            for slab, new, after in ((c.k_slab, c.k_new, c.k_after), (c.v_slab, c.v_new, c.v_after)):
                assert torch.equal(torch.isnan(slab).all(-1).all(1), s >= c.pos[:, None]) and torch.equal(torch.isnan(slab).any(-1).any(1), s >= c.pos[:, None])
                assert torch.equal(torch.isnan(new).all(-1).all(1), t >= c.n_new[:, None])
                assert torch.equal(torch.isnan(after).any(-1).any(1), s >= (c.pos + c.n_new)[:, None])
            assert (c.pos + c.n_new).max().item() == X.CAP and not c.expected[~c.valid].any()
    print(f"T = {T}: {n} queries")
    rows = X.slab_rows(T).tolist()
    assert [0, T] in rows and [31, 1] in rows and [32, max(1, T // 2)] in rows and [X.CAP - T, T] in rows and [45, 1] in rows
    assert ([33, T] in rows) == (33 + T <= X.CAP)


@pytest.mark.parametrize("H,Hkv", X.HEADS)
@pytest.mark.parametrize("mask", X.MASKS)
@pytest.mark.parametrize("Lq,Lk,dims", [(a, b, X.WAVE_DIMS) for a, b in X.BATCH_SHAPES + X.ROWS_SHAPES])
def test_batch_cases(Lq, Lk, dims, mask, H, Hkv):
    n = 0
    for Dh in dims:
        for fam in X.FAMILIES:
            c = X.batch_case(*fam, mask, Lq, Lk, H, Hkv, Dh)
            n += check_flat(c.flat, c.expected)
            assert not c.expected[c.blind].any()
    see = c.flat.see
    if mask == "random":  # what the issue asks of it
        assert c.blind.sum().item() == 1 and c.blind[1, Lq // 2]
        assert see[0, Lq // 3].sum().item() == 1 and see[0, Lq // 3, Lk - 1]
        assert not see[3, :, :min(40, Lk // 2)].any() and not see[2, :64, min(64, Lk - 1):128].any()
    if mask == "broadcast":
        assert c.mask.shape == (1, 1, Lq, Lk)
    print(f"({Lq}, {Lk}) {mask}: {n} queries")


@pytest.mark.parametrize("H,Hkv", X.HEADS)
@pytest.mark.parametrize("short,name", [(False, p) for p in X.PLANS] + [(True, p) for p in X.SHORT_PLANS])
def test_packed_cases(short, name, H, Hkv):
    n = 0
    for Dh in (X.WAVE_DIMS if short else X.TILE_DIMS):
        for fam in X.FAMILIES:
            c = X.packed_case(*fam, name, H, Hkv, Dh, short)
            n += check_flat(c.flat, X.packed_flat_expected(c), rows_differ=False)
            assert c.max_keys <= (32 if short else 65536)
            assert torch.equal(c.expected[~c.named], torch.full_like(c.expected[~c.named], X.CANARY))
            # named rows: pairwise distinct V over rows and KV heads; rows nobody names: poison
            assert len(torch.unique(c.v[c.named].flatten(0, 1), dim=0)) == int(c.named.sum()) * Hkv
            assert (c.v[~c.named] == X.POISON_V).all()
    assert ("gap" not in name) or int((~c.named).sum()) == 5
    print(f"{name}: {n} queries")


# ---- the comparison rejects a kernel that is subtly wrong: three broken restatements, every element type ---------------------
# The GPU test launches every family of X.FAMILIES on a case, so a fault is caught when one family's comparison rejects it.
# Which family does depends on the fault and the mask: under a causal mask rank "last" makes the winner the query's own
# position, so the winners meet every slot of a tile, while "first" and "perm" leave a few record holders; under a random mask
# every rank's winners are the few top keys, and the uniform family - p differs from slot to slot - is the one that sees a swap.
def _sample_cases(fam):
    yield "slab", X.slab_case(*fam, 33, 4, 2, 64)
    yield "batch null", X.batch_case(*fam, "null", 96, 257, 4, 2, 64)
    yield "batch random", X.batch_case(*fam, "random", 96, 257, 3, 3, 128)
    yield "packed", X.packed_case(*fam, "mixed", 4, 2, 64)


@pytest.mark.parametrize("dtype", X.DTYPES)
@pytest.mark.parametrize("what,broken,must", [
    ("two key slots of V^T swapped", dict(swap_v=(5, 6)), ()),
    ("two key slots of V^T swapped across the halves of a tile", dict(swap_v=(3, 19)), ()),
    ("one key too many at a boundary", dict(see_one_more=True), (("selector", "last", "k"), ("uniform", "last", "k"))),
    ("o *= c dropped", dict(rescale=False), (("selector", "last", "k"), ("selector", "perm", "q")))])
def test_a_broken_restatement_is_rejected(what, broken, must, dtype):
    """Every sample case rejects every fault in at least one of its launches; `must`: families that reject it in all of them."""
    rejected = {}
    for fam in X.FAMILIES:
        for name, c in _sample_cases(fam):
            expected = X.packed_flat_expected(c) if hasattr(c, "q_row") else c.expected
            assert X.compare(X.emulate_tiles(c.flat, dtype).to(dtype), expected, fam[0], dtype)[0]
            ok = X.compare(X.emulate_tiles(c.flat, dtype, **broken).to(dtype), expected, fam[0], dtype)[0]
            rejected.setdefault(name, []).append(fam) if not ok else rejected.setdefault(name, [])
    for name, fams in rejected.items():
        print(f"{what}, {name}: rejected by {['-'.join(f) for f in fams]}")
        assert fams, (what, name)
        assert all(f in fams for f in must), (what, name, must)


# ---- ... and these checks notice a weakened generator -----------------------------------------------------------------------------
def test_a_weakened_generator_is_noticed(monkeypatch):
    c = X.slab_case("selector", "perm", "k", 17, 4, 2, 64)
    check_flat(c.flat, c.expected)
    # a V row twice
    v = c.flat.v.clone()
    v[0, 0, 3] = v[0, 0, 2]
    flat = type(c.flat)(**{**vars(c.flat), "v": v})
    with pytest.raises(AssertionError, match="share a V row"):
        check_flat(flat, c.expected)
    # a value that float16 / bfloat16 round
    k = c.flat.k.clone()
    k[0, 0, 0, 0] = 257.0
    with pytest.raises(AssertionError, match="does not survive"):
        check_flat(type(c.flat)(**{**vars(c.flat), "k": k}), c.expected)
    # a listed blind query that sees
    b = X.batch_case("selector", "perm", "k", "random", 33, 160, 4, 2, 64)
    blind = torch.zeros_like(b.blind)
    with pytest.raises(AssertionError, match="not listed"):
        check_flat(type(b.flat)(**{**vars(b.flat), "blind": blind}), b.expected)
    # B lowered: the gap falls under 128 (a fresh case: the cached ones stay as they are)
    monkeypatch.setattr(X, "B", 64)
    weak = X.slab_case.__wrapped__("selector", "perm", "k", 17, 4, 2, 64)
    with pytest.raises(AssertionError, match="above the runner-up"):
        check_flat(weak.flat, weak.expected)
