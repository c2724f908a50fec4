"""KV rows in e4m3 on the host (no GPU): the two C entries refuse bad arguments before anything is launched,
and the classes refuse the option where it cannot serve, by message."""
import ctypes as C

import pytest

import genlm_backend_amd  # noqa: F401
from genlm_backend_amd import _lib

BUF = (C.c_char * 80)()
P = C.c_void_p((C.addressof(BUF) + 15) & ~15)  # any aligned host address: nothing is launched
PTRS = ("q", "k_new", "v_new", "k_codes", "v_codes", "k_scale", "v_scale", "pos", "out")


def _attend(H=4, Hkv=2, Dh=64, **null):
    a = {k: null.get(k, P) for k in PTRS}
    return _lib.load().glb_slab_attention_fp8(a["q"], H * Dh, Dh, a["k_new"], Hkv * Dh, Dh, a["v_new"], Hkv * Dh, Dh, a["k_codes"],
                                              a["v_codes"], a["k_scale"], a["v_scale"], a["pos"], 4, H, Hkv, 8, Dh, 0.125, 0, a["out"], None)


def _quantize(Dh=64, src=P, scale=P):
    return _lib.load().glb_kv_quantize_rows(src, P, scale, 2, 3, 5, 2, Dh, 8, 8, P, P, 0, None)


@pytest.mark.parametrize("name", PTRS)
def test_attention_entry_refuses_a_null_pointer(name):
    assert _attend(**{name: None}) == _lib.GLB_EINVAL and "null pointer" in _lib.last_error()


def test_entries_refuse_unbuilt_shapes_before_any_launch():
    assert _attend(Dh=32) == _lib.GLB_EUNSUPPORTED and "head_dim 32" in _lib.last_error()
    assert _attend(H=6, Hkv=2) == _lib.GLB_EUNSUPPORTED and "3 query heads per KV head" in _lib.last_error()
    assert _attend(H=5, Hkv=2) == _lib.GLB_EINVAL
    assert _quantize(Dh=32) == _lib.GLB_EUNSUPPORTED and "head_dim 32" in _lib.last_error()
    assert _quantize(src=None) == _lib.GLB_EINVAL and _quantize(scale=None) == _lib.GLB_EINVAL


@pytest.mark.parametrize("attn,hidden,heads,kv_heads,match", [
    ("sdpa", 128, 2, 2, "does not go through this backend's fused attention entry"),
    ("glb", 64, 2, 2, "not built for torch.float32, head_dim 32"),
    ("glb", 384, 6, 2, "not built for 6 query heads over 2 KV heads")])
def test_a_model_the_kernel_does_not_serve_is_refused_by_name(attn, hidden, heads, kv_heads, match):
    import types

    import torch

    from genlm_backend_amd.engine import HipEngine
    from genlm_backend_amd.kv import SlabForward, SlabKV
    from genlm_backend_amd.sis import DeviceSIS

    body = torch.nn.Linear(2, 2)  # (float32 parameters; the class stands for an engine: nothing is launched)
    body.config = types.SimpleNamespace(_attn_implementation=attn, _glb_engine=HipEngine, hidden_size=hidden,
                                        num_attention_heads=heads, num_key_value_heads=kv_heads)
    with pytest.raises(ValueError, match=match):
        DeviceSIS(types.SimpleNamespace(_body=body, engine=HipEngine), 2, [1, 2], 4, 0, use_particle_kv=True, share_kv=False,
                  kv_dtype="fp8_e4m3")
    with pytest.raises(ValueError, match=match):
        SlabForward(SlabKV(HipEngine, 2, 8, 1, kv_dtype="fp8_e4m3"), body, graph=False)


def test_classes_refuse_the_option_where_it_cannot_serve():
    from genlm_backend_amd.kv import SharedSlabKV, SlabForward, SlabKV
    from genlm_backend_amd.sis import DeviceSIS

    with pytest.raises(ValueError, match="kv_dtype must be None or one of"):
        SlabKV(None, 2, 8, 1, kv_dtype="fp8_e5m2")
    with pytest.raises(ValueError, match="private rows only"):
        SharedSlabKV(None, 2, 8, 1, kv_dtype="fp8_e4m3")
    pkv = SlabKV(None, 2, 8, 1, kv_dtype="fp8_e4m3")
    with pytest.raises(ValueError, match="stand behind no stored prefix"):
        pkv.set_prefix([], None, None)
    with pytest.raises(ValueError, match="fused forward only: fused_attention=False"):
        SlabForward(pkv, object(), graph=False, fused_attention=False)
    kw = dict(llm=None, n_particles=2, prompt_ids=[1, 2], max_tokens=4, eos_id=0, kv_dtype="fp8_e4m3")
    for match, more in (("needs use_particle_kv=True", dict()), ("needs share_kv=False", dict(use_particle_kv=True)),
                        ("needs share_prompt_kv=False", dict(use_particle_kv=True, share_kv=False, share_prompt_kv=True)),
                        ("serves one rank", dict(use_particle_kv=True, share_kv=False, world=2))):
        with pytest.raises(ValueError, match=match):
            DeviceSIS(**kw, **more)
