"""The constraints package's layout, without a GPU: the public names are the same objects from the top-level package and
from `constraints`, the private ones the tools import resolve, and `engine.dfa_call` admits exactly the block entries of
`_lib`'s signature table."""
import ctypes as C

import pytest

import genlm_backend_amd
from genlm_backend_amd import _lib, constraints


def test_public_names_are_one_object_each():
    for name in ("ByteDFA", "ByteWFSA", "DeviceConstraint", "minimize"):
        assert getattr(genlm_backend_amd, name) is getattr(constraints, name), name
    assert callable(constraints._kept) and callable(constraints._regex_dfa)


def test_from_regex_through_the_package():
    dfa = constraints.ByteDFA.from_regex(b"a(b|c){2}")
    assert dfa.accepts(b"abc") and not dfa.accepts(b"ab")


def test_dfa_call_admits_the_block_entries_of_the_signature_table():
    from genlm_backend_amd.engine import HipEngine

    blocks = {name for name, (_, args) in _lib.SYMBOLS.items()
              if name.startswith("glb_dfa_") and args and hasattr(args[0], "contents") and issubclass(args[0]._type_, C.Structure)}
    others = {name for name in _lib.SYMBOLS if name.startswith("glb_dfa_")} - blocks
    assert HipEngine.DFA_CALLS == blocks and len(blocks) == 13 and others == {"glb_dfa_bank_rows", "glb_dfa_weight_bank_rows"}
    for name in sorted(others) + ["glb_w4_gemm", "glb_dfa_nothing", ""]:  # (refused before the engine is looked at)
        with pytest.raises(ValueError):
            HipEngine.dfa_call(None, name, None)
