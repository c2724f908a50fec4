"""glb_packed_row_map + glb_packed_attention_tile on the MI355X: the row-packed MFMA tile attention against
torch in float64 segment by segment, plans and row maps it must not follow, and the host's refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from genlm_backend_amd import _lib

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2, torch.float16: 3e-3}  # tests/test_attn_batch_gpu.py's: the same arithmetic and inputs
CANARY = 12345.0


def _plan(prompts, tails, gap=0, reverse=False):
    """(segments int32 [S, 4], M): the prompts' rows, `gap` rows nobody names, then the tails (group, length) in order."""
    starts = np.concatenate([[0], np.cumsum(prompts)]).astype(int)
    seg, at = [(0, 0, int(starts[g]), n) for g, n in enumerate(prompts)], int(starts[-1]) + gap
    for g, t in tails:
        seg.append((int(starts[g]), prompts[g], at, t))
        at += t
    return np.asarray(seg[::-1] if reverse else seg, np.int32), at


MIXED = ([40, 70], [(i % 2, 3) for i in range(9)])
PLANS = {"mixed": _plan(*MIXED),  # two prefix ranges in one block, more than 32 keys, many contexts a block
         "ragged": _plan([33], [(0, 1), (0, 17), (0, 64), (0, 65)]),  # a tail from mid-block, one block exactly, across blocks
         "long-prompt": _plan([130], [(0, 5), (0, 5)]),  # the prompt spans blocks; a partial last tile of the shared walk
         "alone": _plan([1, 31, 32, 33, 97], []),  # phase B only; tile boundaries
         "gap": _plan(*MIXED, gap=5, reverse=True)}  # unnamed rows in between, segments in reverse order


def _projection(seed, M, H, Hkv, Dh, dtype, dev):
    """q | k | v as strided views of one [M, (H + 2 Hkv) Dh] projection."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    proj = torch.randn((M, (H + 2 * Hkv) * Dh), device=dev, generator=g).to(dtype)
    return (proj, proj[:, :H * Dh].view(M, H, Dh), proj[:, H * Dh:(H + Hkv) * Dh].view(M, Hkv, Dh),
            proj[:, (H + Hkv) * Dh:].view(M, Hkv, Dh))


def _reference(q, k, v, seg, scale):
    """float64, segment by segment: (ref [M, H, Dh], named bool [M])."""
    M, H, _ = q.shape
    G, dev = H // k.shape[1], q.device
    ref, named = torch.zeros(q.shape, dtype=torch.float64, device=dev), torch.zeros(M, dtype=torch.bool, device=dev)
    for a, n, b, t in seg.tolist():
        rows = torch.tensor(list(range(a, a + n)) + list(range(b, b + t)), device=dev)
        kk, vv = (x[rows].double().repeat_interleave(G, dim=1) for x in (k, v))
        sc = torch.einsum("thd,shd->hts", q[b:b + t].double(), kk) * scale
        see = torch.arange(n + t, device=dev)[None, :] <= n + torch.arange(t, device=dev)[:, None]
        ref[b:b + t] = torch.einsum("hts,shd->thd", torch.softmax(sc.masked_fill(~see, float("-inf")), -1), vv)
        named[b:b + t] = True
    return ref, named


def _check(out, ref, named, dtype, what):
    err = (out.double() - ref)[named].abs().max().item()
    print(f"{what}: max |packed tile - float64| = {err:.3e} (bound {TOL[dtype]})")
    assert err < TOL[dtype], what
    assert torch.equal(out[~named], torch.full_like(out[~named], CANARY)), what  # rows nobody names are not written


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("H,Hkv", [(4, 2), (3, 3)])
@pytest.mark.parametrize("Dh", [64, 128])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_packed_attention_tile_against_float64(engine, dtype, Dh, H, Hkv, plan):
    dev = engine.device
    seg, M = PLANS[plan]
    proj, q, k, v = _projection(Dh + H + M, M, H, Hkv, Dh, dtype, dev)
    before, scale = proj.clone(), Dh ** -0.5
    ref, named = _reference(q, k, v, seg, scale)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    row_map = engine.packed_row_map(torch.from_numpy(seg).to(dev), M, int((seg[:, 1] + seg[:, 3]).max()), err=err)
    out = engine.packed_attention_tile(q, k, v, row_map, scale, out=torch.full((M, H, Dh), CANARY, dtype=dtype, device=dev))
    torch.cuda.synchronize()
    assert int(err.item()) == 0
    _check(out, ref, named, dtype, plan)
    assert torch.equal(proj, before)
    # one replay from a captured graph: the bits of the direct call
    out2 = torch.full_like(out, CANARY)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        engine.packed_attention_tile(q, k, v, row_map, scale, out=out2)
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(out2, out)


def test_a_hostile_plan_and_a_hostile_row_map_are_not_followed(engine):
    dev, dtype, H, Hkv, Dh = engine.device, torch.float32, 4, 2, 64
    good, M0 = PLANS["mixed"]
    M, max_keys = M0 + 4, 73  # four more rows, which only the bad segments name
    bad = [(40, 70, M0, 4),  # pre_len + tail_len = max_keys + 1
           (0, 40, M0, 0),  # no query
           (0, 40, M - 1, 2),  # tail_start + tail_len = n_rows + 1
           (-1, 40, M0 + 1, 2)]
    seg = np.concatenate([good, np.asarray(bad, np.int32)])
    proj, q, k, v = _projection(11, M, H, Hkv, Dh, dtype, dev)
    scale = Dh ** -0.5
    ref, named = _reference(q, k, v, good, scale)
    err = torch.full((1,), 5, dtype=torch.int32, device=dev)
    row_map = engine.packed_row_map(torch.from_numpy(seg).to(dev), M, max_keys, err=err)
    out = engine.packed_attention_tile(q, k, v, row_map, scale, out=torch.full((M, H, Dh), CANARY, dtype=dtype, device=dev))
    assert int(err.item()) == 5 + 4
    assert not named[M0:].any()
    _check(out, ref, named, dtype, "hostile plan")
    # a valid map with two entries overwritten: those rows are not followed, the others are served
    row_map = engine.packed_row_map(torch.from_numpy(good).to(dev), M, max_keys, err=err)
    r1, r2 = M0 - 1, M0 - 5
    row_map[r1] = torch.tensor([r1 - 2, M - 10, 11, 1], dtype=torch.int32)  # pre_start + pre_len > n_rows
    row_map[r2, 0] = r2 + 1  # seg_start > row
    named[r1] = named[r2] = False
    out = engine.packed_attention_tile(q, k, v, row_map, scale, out=torch.full((M, H, Dh), CANARY, dtype=dtype, device=dev))
    _check(out, ref, named, dtype, "hostile row map")


def test_bad_arguments_are_refused_before_any_launch(engine):
    dev, H, Dh = engine.device, 2, 64
    seg, M = PLANS["long-prompt"]
    proj, q, k, v = _projection(3, M, H, H, Dh, torch.float32, dev)
    plan = torch.from_numpy(seg).to(dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    row_map = torch.full((M, 4), 7, dtype=torch.int32, device=dev)
    out = torch.full((M, H, Dh), CANARY, device=dev)
    ptr = lambda x: C.c_void_p(x.data_ptr())

    def make_map(max_keys):
        return engine.lib.glb_packed_row_map(ptr(plan), len(seg), M, max_keys, ptr(row_map), ptr(err), engine._stream())

    def call(q_ptr=ptr(q), q_stride_row=q.stride(0), head_dim=Dh):
        return engine.lib.glb_packed_attention_tile(q_ptr, q_stride_row, q.stride(1), ptr(k), k.stride(0), k.stride(1), ptr(v), v.stride(0),
                                                    v.stride(1), ptr(row_map), M, H, H, head_dim, Dh ** -0.5, _lib.F32, ptr(out),
                                                    engine._stream())

    for max_keys in (0, 65536 + 1):
        assert make_map(max_keys) == _lib.GLB_EINVAL and "keys per context" in _lib.last_error()
    torch.cuda.synchronize()
    assert (row_map == 7).all() and int(err.item()) == 0
    assert make_map(135) == _lib.GLB_OK
    assert call(head_dim=32) == _lib.GLB_EUNSUPPORTED and "head_dim 32 (64 and 128 are built)" in _lib.last_error()
    assert call(q_stride_row=q.stride(0) + 2) == _lib.GLB_EINVAL and "16-byte aligned" in _lib.last_error()
    assert call(q_ptr=C.c_void_p(q.data_ptr() + 4)) == _lib.GLB_EINVAL
    torch.cuda.synchronize()
    assert (out == CANARY).all()  # nothing was enqueued
    assert call() == _lib.GLB_OK  # ... and the same tensors are served
    _check(out, *_reference(q, k, v, seg, Dh ** -0.5), torch.float32, "served after the refusals")
