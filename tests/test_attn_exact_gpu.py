"""Exact-answer tests of the attention kernels on the MI355X: the inputs of tests/attn_exact_ref.py, whose outputs are known
without arithmetic - one key's V row bit for bit (selector), the mean of V over exactly the visible keys within the rounding
of 1 / l, one multiply and the final conversion (uniform) - with NaN or top-ranked poison wherever a kernel must not look.
tests/test_attn_exact_cpu.py shows on the CPU that the cases hold what is relied on here and that the comparison below
rejects swapped V^T slots, a key too many at a boundary and a dropped rescale.  Every launch runs with scale = 1.0."""
import pytest
import torch

from tests import attn_exact_ref as X

pytestmark = pytest.mark.gpu


def _bits(x):
    return x.view(torch.int32 if x.dtype == torch.float32 else torch.int16)  # NaN != NaN: compare the words


class _Report:
    """What a test prints: the queries checked and, for the uniform family, the largest relative error next to its bound."""

    def __init__(self):
        self.queries, self.rel, self.bound = 0, 0.0, 0.0

    def check(self, out, expected, flat, fam, dtype, what):
        ok, rel, bound = X.compare(out, expected.to(out.device), fam[0], dtype)
        self.queries += int(flat.see.any(-1).sum()) * flat.q.shape[1]
        if fam[0] == "uniform":
            self.rel, self.bound = max(self.rel, rel), bound
        assert ok, f"{what} {'-'.join(fam)} {dtype}: " + ("not the winner's V row" if fam[0] == "selector" else f"{rel:.3e} past the bound {bound:.3e}")

    def show(self, what):
        print(f"{what}: {self.queries} queries exact; uniform max |out - mean| / |mean| = {self.rel:.3e} (bound {self.bound:.3e})")


# ---- slab signature ------------------------------------------------------------------------------------------------------------
def _run_slab(call, c, fam, dtype, dev, rep, what, spread=False):
    """One launch over NaN-poisoned slabs: exact outputs, zeros at padded queries, the new K / V appended, every other word of
    the slabs as before.  spread: the rows lie, through rows=, in a larger slab whose other rows are NaN."""
    to = lambda x: x.to(dtype).to(dev)
    q, kn, vn, pos, nn = to(c.q), to(c.k_new), to(c.v_new), c.pos.to(dev), c.n_new.to(dev)
    ks, vs, ka, va = to(c.k_slab), to(c.v_slab), to(c.k_after), to(c.v_after)
    R, rows = ks.shape[0], None
    if spread:
        rows = torch.tensor([6, 0, 3, 7, 2, 8][:R], dtype=torch.int32, device=dev)
        big = [torch.full((R + 3,) + tuple(ks.shape[1:]), float("nan"), dtype=dtype, device=dev) for _ in range(4)]
        for b, x in zip(big, (ks, vs, ka, va)):
            b[rows.long()] = x
        ks, vs, ka, va = big
    out = call(q, kn, vn, ks, vs, pos, nn, rows)
    torch.cuda.synchronize()
    assert out.shape == c.expected.shape and out.dtype == dtype
    rep.check(out, c.expected, c.flat, fam, dtype, what)
    assert not out[~c.valid.to(dev)].float().any(), what  # zeros behind a row's last token
    assert torch.equal(_bits(ks), _bits(ka)) and torch.equal(_bits(vs), _bits(va)), f"{what}: the slabs after the call"


@pytest.mark.parametrize("dtype", X.DTYPES)
@pytest.mark.parametrize("T", X.TILE_T)
@pytest.mark.parametrize("H,Hkv", X.HEADS)
@pytest.mark.parametrize("Dh", X.TILE_DIMS)
def test_slab_attention_tile_exact(engine, Dh, H, Hkv, T, dtype):
    rep = _Report()
    call = lambda q, kn, vn, ks, vs, pos, nn, rows: engine.slab_attention_tile(q, kn, vn, ks, vs, pos, nn, 1.0, rows=rows)
    for fam in X.FAMILIES:
        c = X.slab_case(*fam, T, H, Hkv, Dh)
        _run_slab(call, c, fam, dtype, engine.device, rep, "tile")
        if fam[1] == "perm":
            _run_slab(call, c, fam, dtype, engine.device, rep, "tile, rows=", spread=True)
    rep.show(f"slab_attention_tile T = {T}")


@pytest.mark.parametrize("dtype", X.DTYPES)
@pytest.mark.parametrize("T", X.CHUNK_T)
@pytest.mark.parametrize("H,Hkv", X.HEADS)
@pytest.mark.parametrize("Dh", X.WAVE_DIMS)
def test_slab_attention_chunk_exact(engine, Dh, H, Hkv, T, dtype):
    """The chunk kernel, the tile kernel at the same small chunks where it is built, and slab_attention at T = 1."""
    rep = _Report()
    calls = {"chunk": lambda q, kn, vn, ks, vs, pos, nn, rows: engine.slab_attention_chunk(q, kn, vn, ks, vs, pos, nn, 1.0, rows=rows)}
    if Dh in X.TILE_DIMS:
        calls["tile"] = lambda q, kn, vn, ks, vs, pos, nn, rows: engine.slab_attention_tile(q, kn, vn, ks, vs, pos, nn, 1.0, rows=rows)
    for fam in X.FAMILIES:
        c = X.slab_case(*fam, T, H, Hkv, Dh)
        for name, call in calls.items():
            _run_slab(call, c, fam, dtype, engine.device, rep, name)
            if fam[1] == "perm":
                _run_slab(call, c, fam, dtype, engine.device, rep, name + ", rows=", spread=True)
        if T == 1:  # (every row feeds one token: n_new is not an argument)
            _run_slab(lambda q, kn, vn, ks, vs, pos, nn, rows: engine.slab_attention(q, kn, vn, ks, vs, pos, 1.0), c, fam, dtype,
                      engine.device, rep, "slab_attention")
    rep.show(f"slab_attention_chunk{' / slab_attention' if T == 1 else ''} T = {T}")


# ---- batch signature -----------------------------------------------------------------------------------------------------------
def _run_batch(call, Lq, Lk, H, Hkv, Dh, dtype, dev, what):
    rep = _Report()
    for mask in X.MASKS:
        for fam in X.FAMILIES:
            c = X.batch_case(*fam, mask, Lq, Lk, H, Hkv, Dh)
            q, k, v = (x.to(dtype).to(dev) for x in (c.q, c.k, c.v))
            m = None if c.mask is None else c.mask.to(dev)
            if mask == "broadcast":
                m = m.expand(X.U, 1, Lq, Lk)  # (row stride 0)
            out = call(q, k, v, m)
            torch.cuda.synchronize()
            assert out.shape == c.expected.shape and out.dtype == dtype
            rep.check(out, c.expected, c.flat, fam, dtype, f"{what} {mask}")
            assert not out[c.blind.to(dev)].float().any(), mask  # exact zeros where a query sees nothing
    rep.show(f"{what} ({Lq}, {Lk})")


@pytest.mark.parametrize("dtype", X.DTYPES)
@pytest.mark.parametrize("Lq,Lk", X.BATCH_SHAPES)
@pytest.mark.parametrize("H,Hkv", X.HEADS)
@pytest.mark.parametrize("Dh", X.TILE_DIMS)
def test_batch_attention_tile_exact(engine, Dh, H, Hkv, Lq, Lk, dtype):
    _run_batch(lambda q, k, v, m: engine.batch_attention_tile(q, k, v, m, 1.0), Lq, Lk, H, Hkv, Dh, dtype, engine.device, "batch_attention_tile")


@pytest.mark.parametrize("dtype", X.DTYPES)
@pytest.mark.parametrize("Lq,Lk", X.BATCH_SHAPES + X.ROWS_SHAPES)
@pytest.mark.parametrize("H,Hkv", X.HEADS)
@pytest.mark.parametrize("Dh", X.WAVE_DIMS)
def test_short_attention_exact(engine, Dh, H, Hkv, Lq, Lk, dtype):
    """glb_short_attention takes any q_len <= k_len: one wave a query past 32 keys, its (row, KV head) form up to 16 / 32."""
    _run_batch(lambda q, k, v, m: engine.short_attention(q, k, v, m, 1.0), Lq, Lk, H, Hkv, Dh, dtype, engine.device, "short_attention")


# ---- packed signature ----------------------------------------------------------------------------------------------------------
def _run_packed(engine, call, plan, H, Hkv, Dh, dtype, short, what):
    dev, rep = engine.device, _Report()
    for fam in X.FAMILIES:
        c = X.packed_case(*fam, plan, H, Hkv, Dh, short)
        q, k, v = (x.to(dtype).to(dev) for x in (c.q, c.k, c.v))
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        out = call(q, k, v, torch.from_numpy(c.seg).to(dev), c, err, torch.full((c.M, H, Dh), X.CANARY, dtype=dtype, device=dev))
        torch.cuda.synchronize()
        assert int(err.item()) == 0
        named = c.named.to(dev)
        assert torch.equal(out[~named], torch.full_like(out[~named], X.CANARY)), f"{plan}: rows nobody names are not written"
        ok, rel, bound = X.compare(out, c.expected.to(dev), fam[0], dtype, where=named)
        rep.queries += int(named.sum()) * H
        if fam[0] == "uniform":
            rep.rel, rep.bound = max(rep.rel, rel), bound
        assert ok, f"{what} {plan} {'-'.join(fam)} {dtype}: {rel:.3e} (bound {bound:.3e})"
    rep.show(f"{what} {plan}")


@pytest.mark.parametrize("dtype", X.DTYPES)
@pytest.mark.parametrize("plan", list(X.PLANS))
@pytest.mark.parametrize("H,Hkv", X.HEADS)
@pytest.mark.parametrize("Dh", X.TILE_DIMS)
def test_packed_attention_tile_exact(engine, Dh, H, Hkv, plan, dtype):
    def call(q, k, v, seg, c, err, out):
        return engine.packed_attention_tile(q, k, v, engine.packed_row_map(seg, c.M, c.max_keys, err=err), 1.0, out=out)

    _run_packed(engine, call, plan, H, Hkv, Dh, dtype, False, "packed_attention_tile")


@pytest.mark.parametrize("dtype", X.DTYPES)
@pytest.mark.parametrize("plan", list(X.SHORT_PLANS))
@pytest.mark.parametrize("H,Hkv", X.HEADS)
@pytest.mark.parametrize("Dh", X.WAVE_DIMS)
def test_short_attention_packed_exact(engine, Dh, H, Hkv, plan, dtype):
    """The plans' forms within the 32 keys a context this kernel serves: both of its key counts (<= 16 and <= 32)."""
    def call(q, k, v, seg, c, err, out):
        return engine.short_attention_packed(q, k, v, seg, c.max_keys, 1.0, err=err, out=out)

    _run_packed(engine, call, plan, H, Hkv, Dh, dtype, True, "short_attention_packed")
