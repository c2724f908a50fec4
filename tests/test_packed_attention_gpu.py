"""glb_short_attention_packed (contexts that share the rows of their prompt, one row-packed batch) against
glb_short_attention on the equivalent right-padded batch: the same bits for every query; a plan it must not follow is
refused without a write."""
import numpy as np
import pytest
import torch

from genlm_backend_amd._lib import GLB_EINVAL, GlbError
from genlm_backend_amd.kv import packed_plan

pytestmark = pytest.mark.gpu

FORMS = [(torch.float32, 64), (torch.bfloat16, 64), (torch.bfloat16, 128)]
SIZES = [(1, 1), (8, 1), (8, 8), (15, 1), (15, 2), (16, 16), (31, 1), (1, 31)]  # (prompt, tail): both sides of 16 keys, up to 32
CANARY = 12345.0
PAD = 3  # canary rows in front of and behind the output


def _projection(seed, M, H, Hkv, D, dtype, dev):
    """q / k / v as views of one [M, (H + 2 Hkv) D] projection output, the way c_attn leaves them."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn((M, (H + 2 * Hkv) * D), generator=g).to(dtype).to(dev)
    q = qkv[:, :H * D].view(M, H, D)
    k = qkv[:, H * D:(H + Hkv) * D].view(M, Hkv, D)
    v = qkv[:, (H + Hkv) * D:].view(M, Hkv, D)
    return q, k, v


def _padded_reference(engine, q, k, v, seg, n_groups, scale):
    """glb_short_attention on the right-padded batch of the contexts (segments behind the prompts'): [U, L, H, D] and the
    packed rows of every context's tokens."""
    dev = q.device
    ctx = seg[n_groups:]
    rows = [list(range(a, a + n)) + list(range(b, b + t)) for a, n, b, t in ctx.tolist()]
    U, L = len(rows), max(len(r) for r in rows)
    idx = torch.zeros((U, L), dtype=torch.long)
    valid = torch.zeros((U, L), dtype=torch.bool)
    for u, r in enumerate(rows):
        idx[u, :len(r)] = torch.tensor(r)
        valid[u, :len(r)] = True
    idx, valid = idx.to(dev), valid.to(dev)

    def pad(x):  # [M, h, D] -> [U, h, L, D], zeros behind a context's end
        return (x[idx] * valid[:, :, None, None].to(x.dtype)).permute(0, 2, 1, 3).contiguous()

    causal = torch.tril(torch.ones((L, L), dtype=torch.bool, device=dev))
    mask = (causal[None] & valid[:, None, :])[:, None].contiguous()  # [U, 1, L, L]: what transformers builds from the padding mask
    return engine.short_attention(pad(q), pad(k), pad(v), mask, scale), rows


def _run_case(engine, dtype, D, H, Hkv, group_lens, grp, tails, seed):
    dev = engine.device
    lens = [group_lens[g] + t for g, t in zip(grp, tails)]
    seg, _, _, _ = packed_plan(group_lens, grp, lens)
    M, G = sum(group_lens) + sum(tails), len(group_lens)
    q, k, v = _projection(seed, M, H, Hkv, D, dtype, dev)
    scale = D ** -0.5
    ref, rows = _padded_reference(engine, q, k, v, seg, G, scale)
    buf = torch.full((M + 2 * PAD, H, D), CANARY, dtype=dtype, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    out = engine.short_attention_packed(q, k, v, torch.from_numpy(seg).to(dev), max(lens), scale, err=err, out=buf[PAD:PAD + M])
    assert int(err.item()) == 0
    assert torch.equal(buf[:PAD], torch.full_like(buf[:PAD], CANARY)) and torch.equal(buf[PAD + M:], torch.full_like(buf[:PAD], CANARY))
    seen = set()
    for u, r in enumerate(rows):
        P = group_lens[grp[u]]
        # the tail's queries - and the prompt's, which every context of the group computes with the same bits
        assert torch.equal(out[r[P:]], ref[u, P:len(r)]), (u, "tail")
        assert torch.equal(out[r[:P]], ref[u, :P]), (u, "prompt")
        seen.update(r)
    untouched = [m for m in range(M) if m not in seen]  # the prompt of a group without a context is still served
    assert all(not torch.equal(out[m], torch.full_like(out[m], CANARY)) for m in untouched)


@pytest.mark.parametrize("P,t", SIZES)
@pytest.mark.parametrize("dtype,D", FORMS, ids=["f32-64", "bf16-64", "bf16-128"])
def test_packed_matches_padded(engine, dtype, D, P, t):
    seed = 0
    for U in (1, 2, 5):
        for H, Hkv in ((2, 2), (4, 2)):
            for G in (1, 3):
                group_lens = [P] if G == 1 else [P, max(1, P - 1), max(1, P // 2)]
                grp = [u % G for u in range(U)]
                seed += 1
                _run_case(engine, dtype, D, H, Hkv, group_lens, grp, [t] * U, seed)


@pytest.mark.parametrize("dtype,D", FORMS, ids=["f32-64", "bf16-64", "bf16-128"])
def test_packed_unequal_tails(engine, dtype, D):
    """Tails of 1 .. 10 tokens behind prompts of 8, 5 and 1 in one call (9 to 18 keys: both kernel forms' sizes at once)."""
    _run_case(engine, dtype, D, 4, 2, [8, 5, 1], [0, 1, 2, 0, 0, 1, 2], [1, 10, 3, 7, 2, 1, 10], 77)
    _run_case(engine, dtype, D, 2, 2, [8], [0, 0, 0], [3, 1, 2], 78)  # at most 11 keys: the register form alone


def test_packed_refuses_33_keys(engine):
    """P + t = 33: the entry returns GLB_EINVAL and launches nothing."""
    dev = engine.device
    seg, _, _, _ = packed_plan([17], [0], [33])
    M = 33
    q, k, v = _projection(5, M, 2, 2, 64, torch.float32, dev)
    out = torch.full((M, 2, 64), CANARY, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(GlbError) as e:
        engine.short_attention_packed(q, k, v, torch.from_numpy(seg).to(dev), 33, 0.125, err=err, out=out)
    assert e.value.code == GLB_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, CANARY)) and int(err.item()) == 0


@pytest.mark.parametrize("bad", [(0, 4, 30, 3), (-1, 4, 4, 2), (0, 4, 4, 0), (0, 4, 2 ** 31 - 2, 2), (40, 4, 4, 2), (0, 16, 4, 2)],
                         ids=["tail past M", "negative prompt", "empty tail", "tail near 2^31", "prompt past M", "more keys than max_keys"])
def test_packed_out_of_range_segment(engine, bad):
    """A hand-made plan at U = 2 whose second context must not be followed: it writes nothing and counts in the error word;
    the well-formed segments are served as ever."""
    dev = engine.device
    good, _, _, _ = packed_plan([4], [0, 0], [6, 6])  # M = 8: prompt rows 0 .. 3, tails 4 .. 5 and 6 .. 7
    M = 8
    q, k, v = _projection(9, M, 2, 2, 64, torch.float32, dev)
    want = torch.full((M, 2, 64), CANARY, device=dev)
    engine.short_attention_packed(q, k, v, torch.from_numpy(good).to(dev), 6, 0.125, err=torch.zeros(1, dtype=torch.int32, device=dev), out=want)
    plan = good.copy()
    plan[2] = np.array(bad, np.int32)
    out = torch.full((M, 2, 64), CANARY, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    engine.short_attention_packed(q, k, v, torch.from_numpy(plan).to(dev), 6, 0.125, err=err, out=out)
    assert int(err.item()) == 1
    assert torch.equal(out[:6], want[:6])
    assert torch.equal(out[6:], torch.full_like(out[6:], CANARY))
