"""Byte-level DFA constraints without a GPU: `ByteDFA` (validation, `live`, `from_strings`), the restatement's own sanity, the
C ABI's symbols, argument checks and argument-block size, and `DeviceSIS`'s refusal of two mask sources."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from genlm_backend_amd import constraints  # noqa: F401  (without the feature every test of this file fails here)
from tests import dfa_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("glb_dfa_bank_init", "glb_dfa_advance", "glb_dfa_claim_rows", "glb_dfa_fill_masks", "glb_dfa_mask_ids",
         "glb_dfa_bank_rows")


def test_byte_dfa_validation():
    from genlm_backend_amd.constraints import ByteDFA

    d = np.full((3, 256), -1, np.int32)
    d[0, 65], d[1, 66] = 1, 2
    acc = np.array([False, False, True])
    dfa = ByteDFA(d, acc, 0)
    assert dfa.n_states == 3 and dfa.delta.dtype == np.int32 and dfa.accepting.dtype == np.bool_ and dfa.start == 0
    assert dfa.accepts(b"AB") and not dfa.accepts(b"A") and not dfa.accepts(b"ABA")
    assert ByteDFA(d.astype(np.int64), [0, 0, 1], np.int64(2)).start == 2  # integer tables and 0 / 1 flags are taken
    bad = d.copy()
    bad[0, 0] = 3
    lower = d.copy()
    lower[2, 7] = -2
    for args in [(d[:, :255], acc, 0), (d.reshape(-1), acc, 0), (d[:0], acc[:0], 0), (bad, acc, 0), (lower, acc, 0),
                 (d.astype(np.float32), acc, 0), (d, acc[:2], 0), (d, np.array([0, 2, 1]), 0), (d, acc, 3), (d, acc, -1),
                 (d, acc, 0.0), (d, acc, True)]:
        with pytest.raises(ValueError):
            ByteDFA(*args)


def test_live_is_reachability_of_an_accepting_state():
    from genlm_backend_amd.constraints import ByteDFA

    for name, (d, acc, start) in R.automata(3).items():
        dfa = ByteDFA(d, acc, start)
        assert np.array_equal(dfa.live, R.live(d, acc)), name
    d, acc, start = R.automata()["trap"]
    assert ByteDFA(d, acc, start).live.tolist() == [True, True, False, False]
    rng = np.random.default_rng(11)
    for S in (1, 2, 9, 60):  # sparse random graphs: many states cannot reach an accepting one
        d = np.full((S, 256), -1, np.int32)
        for _ in range(2 * S):
            d[rng.integers(S), rng.integers(256)] = rng.integers(S)
        acc = rng.random(S) < 0.15
        assert np.array_equal(ByteDFA(d, acc, 0).live, R.live(d, acc))


def test_from_strings_is_the_trie_of_the_language():
    from genlm_backend_amd.constraints import ByteDFA

    words = [b"yes", b"no", b"yesno", b"y", b"\x00\xff"]
    dfa = ByteDFA.from_strings(words)
    assert dfa.n_states == 1 + len({w[:i] for w in words for i in range(1, len(w) + 1)})
    assert dfa.live.all()  # every node of a trie of accepted strings leads to one
    for w in words:
        assert dfa.accepts(w)
    for w in (b"", b"ye", b"yesn", b"yesnoo", b"n", b"\x00", b"on"):
        assert not dfa.accepts(w)
    assert ByteDFA.from_strings([b""]).accepts(b"")
    with pytest.raises(ValueError):
        ByteDFA.from_strings([])


def test_restatement_walks_tokens_the_same_way_one_by_one_and_side_by_side():
    """A self-check of the yardstick, not of the feature: tests/dfa_ref.py walks tokens in two independent ways (`next`, one
    token byte by byte; `next_all`, every token side by side) and the GPU tests compare against the second."""
    vocab, eos, skip = R.synth_vocab(300, 1)
    assert len(vocab) == 300 and b"" in vocab and max(map(len, vocab)) == 70 and all(bytes([b]) in vocab for b in range(256))
    for name, (d, acc, start) in R.automata().items():
        ref = R.Ref(d, acc, start, vocab, eos, skip)
        for s in range(min(len(acc), 5)):
            assert ref.next_all(s).tolist() == [ref.next(s, t) for t in range(300)], name
        m = ref.mask(start)
        assert m.shape == (10,) and m[-1] >> (300 - 288) == 0
        assert bool(m[eos >> 5] >> (eos & 31) & 1) == bool(acc[start])
    ref = R.Ref(*R.automata()["digits"], vocab, eos, skip)
    allowed = [t for t in range(300) if ref.mask(0)[t >> 5] >> (t & 31) & 1]
    assert allowed and all(vocab[t].isdigit() for t in allowed) and vocab.index(b"0" * 70) in allowed
    assert ref.next(0, 256) == -1 and ref.next(0, 257) == -1 and ref.next(-1, 48) == -1 and ref.next(0, 300) == -1
    assert ref.advance(0, [49, 50]) == 1 and ref.advance(0, [49, 97, 50]) == -1 and ref.advance(0, []) == 0
    assert ref.particle_mask(1, 4, 4).tolist() == ref.row_eos().tolist() and not ref.particle_mask(0, 4, 4).any()


def test_abi_symbols_and_argument_errors():
    import genlm_backend_amd
    from genlm_backend_amd import _lib

    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    for name in ("ByteDFA", "DeviceConstraint"):
        assert name in genlm_backend_amd.__all__ and getattr(genlm_backend_amd, name).__name__ == name
    assert lib.glb_dfa_bank_rows(256 << 20, 50257, 100) == 102
    assert lib.glb_dfa_bank_rows(10 * 1571 * 4 + 3, 50257, 100) == 10
    assert lib.glb_dfa_bank_rows(1 << 40, 50257, 1 << 20) == 65535
    assert lib.glb_dfa_bank_rows(1 << 20, 0, 4) == 0 and lib.glb_dfa_bank_rows(1 << 20, 64, 0) == 0
    buf = (C.c_char * 8192)()  # never dereferenced: every call below fails its argument check first
    ptr = C.addressof(buf) + (-C.addressof(buf)) % 16
    calls = [getattr(lib, n) for n in NAMES[:5]]

    def good():
        a = _lib.DfaArgs()
        a.struct_size = C.sizeof(_lib.DfaArgs)
        a.n_states, a.start, a.eos_id, a.vocab, a.n_bytes, a.n, a.ld = 4, 0, 2, 300, 100, 8, 4
        a.bank_ld, a.capacity, a.max_work = 10, 6, 4
        for k in ("delta", "accepting", "live", "tok_bytes", "tok_ptr", "skip", "tokens", "from_", "to", "state_in", "state_out",
                  "bank", "row_of_state", "work", "counters", "out_rows"):
            setattr(a, k, ptr)
        return a

    for fn in calls:
        assert fn(None, None) == _lib.GLB_EINVAL
        a = good()
        a.struct_size = 8
        assert fn(C.byref(a), None) == _lib.GLB_EINVAL and "struct_size" in _lib.last_error()
        for n_states in (0, -3):
            a = good()
            a.n_states = n_states
            assert fn(C.byref(a), None) == _lib.GLB_EINVAL and "n_states" in _lib.last_error()
        for start in (-1, 4):
            a = good()
            a.start = start
            assert fn(C.byref(a), None) == _lib.GLB_EINVAL and "start" in _lib.last_error()
        a = good()
        a.delta = None
        assert fn(C.byref(a), None) == _lib.GLB_EINVAL
    for fn in (lib.glb_dfa_bank_init, lib.glb_dfa_claim_rows, lib.glb_dfa_fill_masks, lib.glb_dfa_mask_ids):
        a = good()
        a.bank_ld = 9  # ceil(300 / 32) = 10
        assert fn(C.byref(a), None) == _lib.GLB_EINVAL and "bank_ld" in _lib.last_error()
        a = good()
        a.capacity = 1
        assert fn(C.byref(a), None) == _lib.GLB_EINVAL
        a = good()
        a.counters = None
        assert fn(C.byref(a), None) == _lib.GLB_EINVAL
    for fn in (lib.glb_dfa_advance, lib.glb_dfa_claim_rows, lib.glb_dfa_mask_ids):
        a = good()
        a.n = 0
        assert fn(C.byref(a), None) == _lib.GLB_EINVAL
    a = good()
    a.tok_ptr = None
    assert lib.glb_dfa_advance(C.byref(a), None) == _lib.GLB_EINVAL and lib.glb_dfa_fill_masks(C.byref(a), None) == _lib.GLB_EINVAL
    a = good()
    a.max_work = 0
    assert lib.glb_dfa_fill_masks(C.byref(a), None) == _lib.GLB_EINVAL and "max_work" in _lib.last_error()


def test_argument_block_has_the_headers_size(tmp_path):
    from genlm_backend_amd import _lib

    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler"
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "glb.h"\nint main(void) { printf("%zu %zu %zu %d\\n", '
                   'sizeof(glb_dfa_args), offsetof(glb_dfa_args, bank), offsetof(glb_dfa_args, out_rows), GLB_DFA_COUNTERS); '
                   'return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = tuple(int(v) for v in subprocess.check_output([str(exe)]).split())
    A = _lib.DfaArgs
    assert got == (C.sizeof(A), A.bank.offset, A.out_rows.offset, _lib.DFA_COUNTERS) == (208, 136, 200, 4)
    assert _lib.ABI_VERSION == 9


def test_constraint_and_particle_masks_are_exclusive():
    from genlm_backend_amd.llm import AsyncAmdLM
    from genlm_backend_amd.sis import DeviceSIS

    with pytest.raises(ValueError, match="particle_masks.*constraint"):
        DeviceSIS(None, 4, [1, 2], 3, 0, particle_masks=object(), constraint=object())
    with pytest.raises(ValueError, match="mask_ids.*constraint"):
        AsyncAmdLM.batch_next_token_step_device(None, None, None, mask_ids=object(), constraint=object())
