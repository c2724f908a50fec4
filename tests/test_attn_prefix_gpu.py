"""glb_slab_attention_prefix on the MI355X: one-token decode over KV rows behind prompts stored once, against
torch in float64 on the same values."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2, torch.float16: 3e-3}  # test_attn_tile_gpu.py's: the same arithmetic
CAP = 24


@functools.lru_cache(maxsize=None)
def _case(dev, dtype, Dh, H, Hkv, lens=(1, 33, 70), pcap=96, R=70):
    """Inputs and the float64 answer, made once per shape: R rows whose prefix cycles through every prefix and -1 and whose
    pos cycles through 0 (an empty own tail), a mid value and cap - 1; q | k | v are views of one projection tensor."""
    g = torch.Generator(device=dev)
    g.manual_seed(Dh + H + len(lens))
    U = len(lens)
    rnd = lambda *shape: torch.randn(shape, device=dev, generator=g).to(dtype)
    ks, vs, pk, pv = rnd(R, Hkv, CAP, Dh), rnd(R, Hkv, CAP, Dh), rnd(U, Hkv, pcap, Dh), rnd(U, Hkv, pcap, Dh)
    proj = rnd(R, 1, (H + 2 * Hkv) * Dh)
    q = proj[..., :H * Dh].view(R, 1, H, Dh).transpose(1, 2)
    kn = proj[..., H * Dh:(H + Hkv) * Dh].view(R, 1, Hkv, Dh).transpose(1, 2)
    vn = proj[..., (H + Hkv) * Dh:].view(R, 1, Hkv, Dh).transpose(1, 2)
    ar = torch.arange(R, device=dev)
    pos = torch.tensor([0, 11, CAP - 1], dtype=torch.int32, device=dev)[ar % 3]
    pf = ((ar % (U + 1)) - (ar % (U + 1) == U).long() * (U + 1)).to(torch.int32)  # 0, 1, .., U - 1, -1, 0, ..
    plen = torch.tensor(lens, dtype=torch.int32, device=dev)
    # the reference: prefix, own slab with the new token in place, one softmax over what the row may see
    k_ref, v_ref = ks.clone(), vs.clone()
    k_ref[ar, :, pos.long()], v_ref[ar, :, pos.long()] = kn[:, :, 0], vn[:, :, 0]
    pfc, G = pf.clamp_min(0).long(), H // Hkv
    kk = torch.cat([pk[pfc], k_ref], 2).double().repeat_interleave(G, 1)
    vv = torch.cat([pv[pfc], v_ref], 2).double().repeat_interleave(G, 1)
    n_pre = torch.where(pf >= 0, plen[pfc], torch.zeros_like(pf))
    see = torch.cat([torch.arange(pcap, device=dev)[None] < n_pre[:, None], torch.arange(CAP, device=dev)[None] <= pos[:, None]], 1)
    sc = torch.einsum("rhd,rhpd->rhp", q[:, :, 0].double(), kk) * Dh ** -0.5
    ref = torch.einsum("rhp,rhpd->rhd", torch.softmax(sc.masked_fill(~see[:, None], float("-inf")), -1), vv)
    return dict(ks=ks, vs=vs, pk=pk, pv=pv, q=q, kn=kn, vn=vn, pos=pos, pf=pf, plen=plen, ref=ref, k_ref=k_ref, v_ref=v_ref)


def _run(engine, c, splits, ks=None, vs=None, pos=None, pf=None):
    ks, vs = (c["ks"].clone(), c["vs"].clone()) if ks is None else (ks, vs)
    out = engine.slab_attention_prefix(c["q"], c["kn"], c["vn"], ks, vs, c["pos"] if pos is None else pos, c["pk"], c["pv"],
                                       c["plen"], c["pf"] if pf is None else pf, c["q"].shape[-1] ** -0.5, splits=splits)
    return out, ks, vs


@pytest.mark.parametrize("splits", [1, 2, 3])
@pytest.mark.parametrize("H,Hkv", [(4, 2), (3, 3)])
@pytest.mark.parametrize("Dh", [64, 128])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_slab_attention_prefix_against_float64(engine, dtype, Dh, H, Hkv, splits):
    c = _case(engine.device, dtype, Dh, H, Hkv)
    R, U = c["pos"].numel(), c["plen"].numel()
    out, k2, v2 = _run(engine, c, splits)
    torch.cuda.synchronize()
    assert out.shape == (R, 1, H, Dh) and out.dtype == dtype
    err = (out[:, 0].double() - c["ref"]).abs().max().item()
    print(f"max |prefix - float64| = {err:.3e} (bound {TOL[dtype]})")
    assert err < TOL[dtype]
    assert torch.equal(k2, c["k_ref"]) and torch.equal(v2, c["v_ref"])  # exactly position pos[r] replaced
    # rows without a prefix: glb_slab_attention's answer
    none = c["pf"] < 0
    plain = engine.slab_attention(c["q"], c["kn"], c["vn"], c["ks"].clone(), c["vs"].clone(), c["pos"], Dh ** -0.5)
    assert (out[none].float() - plain[none].float()).abs().max().item() < TOL[dtype]
    # two bad rows: NaN there, nothing appended, the other rows bit-equal
    pos, pf = c["pos"].clone(), c["pf"].clone()
    pos[5], pf[6] = -1, U
    out3, k3, v3 = _run(engine, c, splits, pos=pos, pf=pf)
    ok = torch.ones(R, dtype=torch.bool, device=engine.device)
    ok[[5, 6]] = False
    assert torch.isnan(out3[~ok].float()).all() and torch.equal(out3[ok], out[ok])
    assert torch.equal(k3[~ok], c["ks"][~ok]) and torch.equal(v3[~ok], c["vs"][~ok])
    assert torch.equal(k3[ok], k2[ok]) and torch.equal(v3[ok], v2[ok])
    # one replay from a captured graph: the same bits (the warm-up above left the workspace at its size)
    k5, v5 = c["ks"].clone(), c["vs"].clone()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out5, _, _ = _run(engine, c, splits, ks=k5, vs=v5)
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(out5, out) and torch.equal(k5, k2) and torch.equal(v5, v2)


@pytest.mark.parametrize("lens,pcap,splits", [((31, 32, 64), 64, 2), ((33,), 40, 8), ((0, 96), 96, 0)])
def test_tile_edges_and_empty_shares(engine, lens, pcap, splits):
    """Prefixes that end at a tile's edge, one key into a tile, eight shares of two tiles, an empty prefix under auto splits."""
    dtype, Dh = torch.bfloat16, 64
    c = _case(engine.device, dtype, Dh, 4, 2, lens=lens, pcap=pcap, R=9)
    out, k2, v2 = _run(engine, c, splits)
    torch.cuda.synchronize()
    err = (out[:, 0].double() - c["ref"]).abs().max().item()
    print(f"lens {lens}, splits {splits}: max |prefix - float64| = {err:.3e} (bound {TOL[dtype]})")
    assert err < TOL[dtype] and torch.equal(k2, c["k_ref"]) and torch.equal(v2, c["v_ref"])
