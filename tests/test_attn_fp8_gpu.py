"""glb_slab_attention_fp8 and glb_kv_quantize_rows on the MI355X: the appended codes and scales against the
quantisation rule computed by torch on the CPU, bit for bit; the output against float64 attention over the dequantised slab.
Codes are handled as bytes here (torch.uint8 views of the float8 tensors); the scales are positive, so equal values are equal bits."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2, torch.float16: 3e-3}  # test_slab_attention_matches_torch's, for unit-scale values
CAP = 40  # three slot rounds at 16 positions a step, five at 8: a partial last one at both
F8, U8 = torch.float8_e4m3fn, torch.uint8


def _rule(x):
    """The rule on the CPU in float32: (codes as bytes, scales) of x [..., head_dim] - amax / 448, 1 where amax == 0, round to nearest even."""
    x = x.detach().float().cpu()
    amax = x.abs().amax(-1, keepdim=True)
    s = torch.where(amax == 0, torch.ones_like(amax), amax / torch.full_like(amax, 448.0))
    return (x / s).to(F8).view(U8), s[..., 0].contiguous()


@functools.lru_cache(maxsize=None)
def _case(dev, dtype, Dh, H, Hkv):
    """Slabs (K codes, V codes, K scales, V scales), strided inputs, the slabs the call must leave and the float64 answer over
    them, made once per shape.  K / V magnitudes per position are spread over 2^-4 .. 2^4, dimension 5 another 50 times larger."""
    g = torch.Generator(device=dev)
    g.manual_seed(Dh + H + Hkv)
    PP, R = 64 // (Dh // 16), 6
    pos = torch.tensor([0, 1, PP - 1, PP, 17, CAP - 1], dtype=torch.int32, device=dev)
    kv = torch.randn((2, R, Hkv, CAP + 1, Dh), device=dev, generator=g) * torch.exp2(torch.rand((2, R, Hkv, CAP + 1, 1), device=dev, generator=g) * 8 - 4)
    kv[..., 5] *= 50
    kv = kv.to(dtype)
    (kc, ks), (vc, vs) = _rule(kv[0, :, :, :CAP]), _rule(kv[1, :, :, :CAP])
    proj = torch.cat([torch.randn((R, H * Dh), device=dev, generator=g).to(dtype), kv[0, :, :, CAP].flatten(1), kv[1, :, :, CAP].flatten(1)], -1)[:, None]
    proj[3, :, H * Dh:] = 0  # row 3's new K and V are all zeros: scale 1, codes 0
    q = proj[..., :H * Dh].view(R, 1, H, Dh).transpose(1, 2)  # q | k | v of one projection
    kn = proj[..., H * Dh:(H + Hkv) * Dh].view(R, 1, Hkv, Dh).transpose(1, 2)
    vn = proj[..., (H + Hkv) * Dh:].view(R, 1, Hkv, Dh).transpose(1, 2)
    want = [t.clone() for t in (kc, vc, ks, vs)]
    ar, at = torch.arange(R), pos.cpu().long()
    (want[0][ar, :, at], want[2][ar, :, at]), (want[1][ar, :, at], want[3][ar, :, at]) = _rule(kn[:, :, 0]), _rule(vn[:, :, 0])
    kd = (want[0].view(F8).double() * want[2].double()[..., None]).repeat_interleave(H // Hkv, 1)
    vd = (want[1].view(F8).double() * want[3].double()[..., None]).repeat_interleave(H // Hkv, 1)
    see = torch.arange(CAP)[None] <= at[:, None]
    sc = torch.einsum("rhd,rhpd->rhp", q[:, :, 0].double().cpu(), kd) * Dh ** -0.5
    ref = torch.einsum("rhp,rhpd->rhd", torch.softmax(sc.masked_fill(~see[:, None], float("-inf")), -1), vd)
    vmax = (vd.abs().amax(-1) * see[:, None]).amax((1, 2)).clamp_min(1.0)  # per row, over what it attends
    return dict(slabs=[t.to(dev) for t in (kc, vc, ks, vs)], q=q, kn=kn, vn=vn, pos=pos, want=want, ref=ref, vmax=vmax)


@pytest.mark.parametrize("H,Hkv", [(2, 2), (8, 2), (8, 1)])  # 1, 4 and 8 query heads per KV head: one wave of 1, one of 4, two of 4
@pytest.mark.parametrize("Dh", [64, 128])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_slab_attention_fp8_against_the_rule_and_float64(engine, dtype, Dh, H, Hkv):
    c = _case(engine.device, dtype, Dh, H, Hkv)
    attend = lambda s, pos: engine.slab_attention_fp8(c["q"], c["kn"], c["vn"], s[0].view(F8), s[1].view(F8), s[2], s[3], pos, Dh ** -0.5)
    slabs = [t.clone() for t in c["slabs"]]
    out = attend(slabs, c["pos"])
    torch.cuda.synchronize()
    assert out.shape == (6, 1, H, Dh) and out.dtype == dtype
    # (a) position pos[r] holds the rule's codes and scale; every other byte is unchanged
    assert all(torch.equal(a.cpu(), b) for a, b in zip(slabs, c["want"]))
    err = (out[:, 0].double().cpu() - c["ref"]).abs().amax((1, 2)) / c["vmax"]  # (b)
    print(f"max |fp8 - float64| / max(1, max |V|) per row = {[f'{e:.2e}' for e in err.tolist()]} (bound {TOL[dtype]})")
    assert (err < TOL[dtype]).all()
    # (c) two positions outside their rows: NaN there, nothing written, the other rows keep their bits
    pos, slabs2 = c["pos"].clone(), [t.clone() for t in c["slabs"]]
    pos[1], pos[4] = CAP, -1
    out2 = attend(slabs2, pos)
    ok = torch.tensor([True, False, True, True, False, True], device=engine.device)
    assert torch.isnan(out2[~ok].float()).all() and torch.equal(out2[ok], out[ok])
    assert all(torch.equal(a[~ok], b[~ok]) and torch.equal(a[ok], d[ok]) for a, b, d in zip(slabs2, c["slabs"], slabs))
    if (dtype, Dh, H) == (torch.bfloat16, 64, 8):  # (d) two replays of a captured call carry the eager call's bits
        held, gr = [t.clone() for t in c["slabs"]], torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            out3 = attend(held, c["pos"])
        gr.replay()
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out3, out) and all(torch.equal(a, b) for a, b in zip(held, slabs))


@pytest.mark.parametrize("dtype,Dh", [(torch.float32, 64), (torch.bfloat16, 128), (torch.float16, 64)])
def test_kv_quantize_rows_and_gather(engine, dtype, Dh):
    """Two layers (four tensors), 3 sources, 5 rows; src_row_of with -1 and a repeated source, len_of 0, 1, PP and src_cap:
    inside the rule's bits, outside the sentinel; then SlabKV.gather: rows equal their ancestors, rows with -1 untouched."""
    from genlm_backend_amd.kv import SlabKV

    dev, Hkv, PP, L, cap = engine.device, 2, 64 // (Dh // 16), 19, 24
    g = torch.Generator(device=dev)
    g.manual_seed(Dh)
    srcs = torch.randn((4, 3, Hkv, L, Dh), device=dev, generator=g) * torch.exp2(torch.rand((4, 3, Hkv, L, 1), device=dev, generator=g) * 8 - 4)
    srcs[1, 2, :, 0] = 0  # (amax == 0)
    srcs = list(srcs.to(dtype))
    src_row_of = torch.tensor([2, -1, 0, 2, 1], dtype=torch.int32, device=dev)
    len_of = torch.tensor([1, 7, PP, L, 0], dtype=torch.int32, device=dev)
    pkv = SlabKV(engine, 5, cap, 2, kv_dtype="fp8_e4m3")
    pkv._alloc_like([(srcs[0], srcs[1]), (srcs[2], srcs[3])])
    for t in pkv._tensors(pkv.layers) + pkv._scales(pkv.layers):
        t.view(U8).fill_(0x5A)
    pkv.fill_rows([(srcs[0], srcs[1]), (srcs[2], srcs[3])], src_row_of, len_of)
    torch.cuda.synchronize()
    inside = ((src_row_of >= 0)[:, None] & (torch.arange(cap, device=dev)[None] < len_of[:, None])).cpu()[:, None].expand(5, Hkv, cap)
    filled = list(zip(pkv._tensors(pkv.layers), pkv._scales(pkv.layers)))
    for src, (codes, scales) in zip(srcs, filled):
        wc, ws = _rule(torch.nn.functional.pad(src, (0, 0, 0, cap - L))[src_row_of.clamp_min(0).long()])
        codes, scales = codes.cpu().view(U8), scales.cpu().view(torch.int32)
        assert torch.equal(codes[inside], wc[inside]) and torch.equal(scales[inside], ws.view(torch.int32)[inside])
        assert (codes[~inside] == 0x5A).all() and (scales[~inside] == 0x5A5A5A5A).all()
    before = [(c.view(U8).clone(), s.clone()) for c, s in filled]
    anc = torch.tensor([3, 3, -1, 0, 2], dtype=torch.int32, device=dev)
    keep = torch.tensor([L, 5, 9, 1, PP], dtype=torch.int32, device=dev)
    pkv.gather(anc, keep)
    torch.cuda.synchronize()
    for (c0, s0), c1, s1 in zip(before, pkv._tensors(pkv.layers), pkv._scales(pkv.layers)):
        for i, (a, n) in enumerate(zip(anc.tolist(), keep.tolist())):
            if a >= 0:
                assert torch.equal(c1.view(U8)[i, :, :n], c0[a, :, :n]) and torch.equal(s1[i, :, :n], s0[a, :, :n]), i
        assert not c1[2].view(U8).any() and not s1[2].any()  # the second slab set's row, as it was made
    assert pkv.nbytes() == 2 * 4 * 5 * Hkv * cap * (Dh + 4)
