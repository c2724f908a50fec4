"""An evicting mask bank without a GPU: the new argument block against the header, `on_full` validation, the argument checks
that need no device, and the restatement tests/dfa_evict_ref.py against an example worked by hand."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import dfa_evict_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_evict_block_has_the_headers_size_and_offsets(tmp_path):
    from genlm_backend_amd import _lib

    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler"
    fields = ("dfa", "arc_logw", "final_logw", "wbank", "wbank_ld", "row_state", "row_stamp", "claimants", "victims", "ecounters",
              "epoch")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "glb.h"\nint main(void) { printf("%zu %d %zu", '
                   'sizeof(glb_dfa_evict_args), GLB_DFA_EVICT_COUNTERS, sizeof(glb_dfa_args));\n'
                   + "".join(f'printf(" %zu", offsetof(glb_dfa_evict_args, {f}));\n' for f in fields) + 'return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    A = _lib.DfaEvictArgs
    assert got[:3] == [C.sizeof(A), _lib.DFA_EVICT_COUNTERS, C.sizeof(_lib.DfaArgs)] == [296, 4, 208]
    assert got[3:] == [getattr(A, f).offset for f in fields] == [8, 216, 224, 232, 240, 248, 256, 264, 272, 280, 288]
    assert _lib.ABI_VERSION == 9 and _lib.DFA_COUNTERS == 4  # neither moved
    lib = _lib.load()
    for name in ("glb_dfa_evict_bank_init", "glb_dfa_evict_serve"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)


def test_on_full_is_validated_before_anything_else():
    from genlm_backend_amd.constraints import ByteDFA, DeviceConstraint

    dfa = ByteDFA.from_strings([b"a"])
    for bad in ("Evict", "lru", None, True, 0):
        with pytest.raises(ValueError, match="on_full"):
            DeviceConstraint(None, dfa, [b"a"], 0, on_full=bad)  # (no engine: the check comes first)


def _good(ptr):
    from genlm_backend_amd import _lib

    a = _lib.DfaArgs()
    a.struct_size = C.sizeof(_lib.DfaArgs)
    a.n_states, a.start, a.eos_id, a.vocab, a.n_bytes, a.n = 40, 0, 2, 300, 100, 8
    a.bank_ld, a.capacity, a.max_work = 10, 6, 4
    for k in ("delta", "accepting", "live", "tok_bytes", "tok_ptr", "skip", "state_in", "bank", "row_of_state", "work", "counters",
              "out_rows"):
        setattr(a, k, ptr)
    e = _lib.DfaEvictArgs()
    e.struct_size, e.dfa = C.sizeof(_lib.DfaEvictArgs), a
    for k in ("row_state", "row_stamp", "claimants", "victims", "ecounters", "epoch"):
        setattr(e, k, ptr)
    return e


def test_argument_errors_come_before_any_launch():
    from genlm_backend_amd import _lib

    lib = _lib.load()
    buf = (C.c_char * 8192)()  # never dereferenced: every call below fails its argument check first
    ptr = C.addressof(buf) + (-C.addressof(buf)) % 16

    def bad(fn, what, **kw):
        e = _good(ptr)
        for k, v in kw.items():
            setattr(e.dfa if k.startswith("dfa_") else e, k[4:] if k.startswith("dfa_") else k, v)
        assert fn(C.byref(e), None) == _lib.GLB_EINVAL, kw
        assert what in _lib.last_error(), (kw, _lib.last_error())

    for fn in (lib.glb_dfa_evict_bank_init, lib.glb_dfa_evict_serve):
        assert fn(None, None) == _lib.GLB_EINVAL
        bad(fn, "glb_dfa_evict_args.struct_size", struct_size=8)
        bad(fn, "glb_dfa_args.struct_size", dfa_struct_size=8)
        for cap in (2, 1, 0, 65536):
            bad(fn, "capacity", dfa_capacity=cap)
        for k in ("row_state", "row_stamp", "claimants", "victims", "ecounters", "epoch"):
            bad(fn, "null eviction table", **{k: None})
        for k in ("dfa_row_of_state", "dfa_work", "dfa_counters", "dfa_bank"):
            bad(fn, "null bank pointer", **{k: None})
        bad(fn, "bank_ld", dfa_bank_ld=9)
        # a float bank: all three tables and a row of at least V floats
        bad(fn, "null weight table", wbank=ptr)
        bad(fn, "null weight table", arc_logw=ptr, final_logw=ptr)
        bad(fn, "wbank_ld", wbank=ptr, arc_logw=ptr, final_logw=ptr, wbank_ld=299)
    serve = lib.glb_dfa_evict_serve
    bad(serve, "n 0", dfa_n=0)
    bad(serve, "null pointer", dfa_state_in=None)
    bad(serve, "null pointer", dfa_out_rows=None)
    bad(serve, "max_work", dfa_max_work=0)
    bad(serve, "vocabulary bytes", dfa_tok_ptr=None)


def test_restatement_against_an_example_worked_by_hand():
    """Six states, a bank of 2 + 3 rows.
    call 1 asks for {0, 1}: three never-used rows tie at stamp 0, two are taken (the restatement: rows 2 and 3).
    call 2 asks for {1, 2, 3}: state 1's row is stamped and safe; the never-used row 4 must go first, then state 0's row
           (stamp 1) - state 0 is evicted.
    call 3 asks for {0 .. 4} and two invalid states: 1, 2 and 3 hold all three rows, all requested now - nothing may be
           taken, 0 and 4 are left over."""
    ref = E.EvictRef(6, 5)
    c1 = ref.serve([0, 1, 1, 0])
    assert c1 == dict(claimants=[0, 1], need=2, must=set(), may={2, 3, 4}, excess=0)
    assert ref.row_of_state.tolist() == [2, 3, -1, -1, -1, -1] and ref.row_stamp.tolist() == [0, 0, 1, 1, 0]
    assert (ref.epoch, ref.fills, ref.evictions, ref.rows_in_use, ref.overflow) == (2, 2, 0, 4, False)
    c2 = ref.serve([3, 1, 2, 2])
    assert c2 == dict(claimants=[2, 3], need=2, must={4}, may={2, 4}, excess=0)
    assert ref.row_of_state.tolist() == [-1, 3, 4, 2, -1, -1] and ref.row_state.tolist() == [-1, -1, 3, 1, 2]
    assert ref.row_stamp.tolist() == [0, 0, 2, 2, 2]
    assert (ref.epoch, ref.fills, ref.evictions, ref.rows_in_use, ref.overflow) == (3, 4, 1, 5, False)
    c3 = ref.serve([0, 1, 2, 3, 4, -1, 6])
    assert c3 == dict(claimants=[0, 4], need=0, must=set(), may=set(), excess=2)
    assert ref.row_of_state.tolist() == [-1, 3, 4, 2, -1, -1] and ref.row_stamp.tolist() == [0, 0, 3, 3, 3]
    assert (ref.epoch, ref.fills, ref.evictions, ref.rows_in_use, ref.overflow) == (4, 4, 1, 5, True)
    acc = np.array([1, 0, 1, 0, 0, 0], np.bool_)
    assert ref.ids([0, 1, 2, 3, 4, -1, 6]) == [0, 3, 4, 2, 0, 0, 0]
    assert ref.ids([0, 1, 2, -1], done=[1, 1, 0, 1], accepting=acc) == [1, 0, 4, 0]
    # a strict order among the evictable rows: of stamps {1, 2, 2}, one row must go, and it is the oldest
    ref = E.EvictRef(8, 5)
    ref.serve([0])
    ref.serve([1, 2])
    c = ref.serve([3])
    assert c["need"] == 1 and c["must"] == set() and c["may"] == {int(ref.row_of_state[3])} and ref.row_of_state[0] == -1
    c = ref.serve([3, 4])  # rows of 1 and 2 tie at stamp 2: either may go, none must
    assert c["need"] == 1 and c["must"] == set() and len(c["may"]) == 2 and ref.evictions == 2
