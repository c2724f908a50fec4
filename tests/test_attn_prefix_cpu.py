"""glb_slab_attention_prefix's argument checks on the host (no GPU): GLB_EINVAL before anything is launched."""
import ctypes as C

import genlm_backend_amd  # noqa: F401
from genlm_backend_amd import _lib


def test_prefix_entry_refuses_bad_arguments_and_sizes_its_workspace():
    lib = _lib.load()
    R, H, Hkv, cap, Dh, U, pcap = 4, 4, 2, 8, 64, 2, 32
    size = lambda s: lib.glb_slab_attention_prefix_workspace(R, H, Dh, s)
    assert 0 < size(1) < size(2) < size(8) and size(0) == 0 and size(9) == 0
    buf = (C.c_char * (size(2) + 16))()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)  # any aligned host address: nothing is launched

    def call(splits=2, ws_bytes=size(2), **null):
        a = {k: null.get(k, p) for k in ("q", "k_new", "v_new", "k_slab", "v_slab", "pos", "out", "pk", "pv", "plen", "pof", "ws")}
        return lib.glb_slab_attention_prefix(a["q"], H * Dh, Dh, a["k_new"], Hkv * Dh, Dh, a["v_new"], Hkv * Dh, Dh, a["k_slab"],
                                             a["v_slab"], a["pos"], R, H, Hkv, cap, Dh, 0.125, 0, a["out"], a["pk"], a["pv"],
                                             a["plen"], a["pof"], U, pcap, splits, a["ws"], ws_bytes, None)

    for name in ("q", "k_new", "v_new", "k_slab", "v_slab", "pos", "out", "pk", "pv", "plen", "pof", "ws"):
        assert call(**{name: None}) == _lib.GLB_EINVAL, name
    assert call(splits=0) == _lib.GLB_EINVAL and call(splits=9) == _lib.GLB_EINVAL
    assert call(ws_bytes=size(2) - 1) == _lib.GLB_EINVAL and "workspace" in _lib.last_error()
