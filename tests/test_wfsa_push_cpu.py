"""Weight pushing without a GPU: the new argument block against the header, every GLB_EINVAL case (the checks run before any
launch), `push` validation, and the restatement tests/wfsa_push_ref.py against float64, a closed form and the properties a
pushed automaton has."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from genlm_backend_amd import _lib
from genlm_backend_amd.constraints import ByteDFA, ByteWFSA, DeviceConstraint
from tests import dfa_ref as R
from tests import wfsa_push_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["digits", "everything", "trap", "random37"]


def test_argument_block_has_the_headers_size_and_offsets(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler"
    fields = [name for name, _ in _lib.DfaPushArgs._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "glb.h"\nint main(void) { printf("%zu %d %d %d", '
                   'sizeof(glb_dfa_push_args), GLB_DFA_PUSH_STATUS, GLB_DFA_PUSH_LOG, GLB_DFA_PUSH_MAX);\n'
                   + "".join(f'printf(" %zu", offsetof(glb_dfa_push_args, {f}));\n' for f in fields) + "return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    A = _lib.DfaPushArgs
    assert got[:4] == [C.sizeof(A), _lib.DFA_PUSH_STATUS, _lib.DFA_PUSH_LOG, _lib.DFA_PUSH_MAX] == [96, 8, 0, 1]
    assert got[4:] == [getattr(A, f).offset for f in fields] == [0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64, 72, 80, 84, 88]


def _block(**kw):
    """A block that passes every check; its pointers are never followed: the calls below fail before any launch."""
    p = _lib.DfaPushArgs()
    p.struct_size = C.sizeof(_lib.DfaPushArgs)
    p.n_states, p.start, p.semiring = 4, 0, _lib.DFA_PUSH_LOG
    for f in ("delta", "arc_logw", "final_logw", "beta", "scratch", "arc_out", "final_out", "status"):
        setattr(p, f, 0x1000)
    p.sweeps, p.restart, p.tol = 1, 1, 2.0 ** -20
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_argument_errors_without_a_device():
    lib = _lib.load()
    for name in ("glb_dfa_backward", "glb_dfa_push_weights"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert lib.glb_abi_version() == 9 == _lib.ABI_VERSION
    both = [("struct_size", 0), ("struct_size", 88), ("struct_size", 104), ("n_states", 0), ("n_states", -3), ("start", -1),
            ("start", 4), ("semiring", 2), ("semiring", -1), ("sweeps", 0), ("sweeps", -5), ("tol", -1e-9), ("tol", float("nan")),
            ("delta", None), ("arc_logw", None), ("final_logw", None), ("beta", None)]
    own = {"glb_dfa_backward": [("scratch", None), ("status", None)], "glb_dfa_push_weights": [("arc_out", None), ("final_out", None)]}
    for name, cases in own.items():
        fn = getattr(lib, name)
        assert fn(None, None) == _lib.GLB_EINVAL
        for field, value in both + cases:
            assert fn(C.byref(_block(**{field: value})), None) == _lib.GLB_EINVAL, (name, field, value)
            assert field in _lib.last_error(), (name, field, _lib.last_error())


def test_push_validation():
    d, acc, start = R.automata()["digits"]
    wf = ByteWFSA(d, *P.substochastic_weights(d, acc, 7), start)
    vocab = [bytes([b]) for b in range(256)]
    # (the arguments are refused before the engine is looked at: no device is needed to be told so)
    with pytest.raises(ValueError, match="push must be"):
        DeviceConstraint(None, wf, vocab, 0, push="tropical")
    with pytest.raises(ValueError, match="push must be"):
        DeviceConstraint(None, wf, vocab, 0, push=True)
    for push in ("log", "max"):
        with pytest.raises(ValueError, match="ByteWFSA"):
            DeviceConstraint(None, ByteDFA(d, acc, start), vocab, 0, push=push)
        with pytest.raises(ValueError, match="push_tol"):
            DeviceConstraint(None, wf, vocab, 0, push=push, push_tol=-1.0)
        with pytest.raises(ValueError, match="push_tol"):
            DeviceConstraint(None, wf, vocab, 0, push=push, push_tol=float("nan"))
        with pytest.raises(ValueError, match="push_max_sweeps"):
            DeviceConstraint(None, wf, vocab, 0, push=push, push_max_sweeps=0)


@pytest.mark.parametrize("name", NAMES)
def test_float32_restatement_against_the_float64_fixed_point(name):
    d, acc, start = R.automata()[name]
    arc, fin = P.substochastic_weights(d, acc, 7)
    live = R.live(np.asarray(d, np.int64), acc)
    b64 = P.fixed_point64(d, arc, fin, P.LOG)
    b32, sweeps, ok = P.backward(d, arc, fin, P.LOG)
    assert ok and b32.dtype == np.float32 and sweeps <= 24
    assert np.array_equal(np.isfinite(b32), live) and np.array_equal(np.isfinite(b64), live)
    dist = np.abs(b32[live].astype(np.float64) - b64[live]).max()
    print(f"{name}: {sweeps} float32 sweeps, max distance from the float64 fixed point {dist:.3e}")
    assert dist < 5e-6
    m32, msweeps, ok = P.backward(d, arc, fin, P.MAX)
    assert ok and msweeps <= len(acc) + 1 and np.array_equal(np.isfinite(m32), live)
    assert (m32[live] <= b32[live] + 1e-6).all()  # the best string weighs no more than all of them


def test_zero_weights_diverge_under_log_and_converge_under_max():
    d, acc, start = R.automata()["digits"]
    arc = np.where(d >= 0, 0.0, -np.inf).astype(np.float32)
    fin = np.where(acc, 0.0, -np.inf).astype(np.float32)
    beta, sweeps, ok = P.backward(d, arc, fin, P.LOG, max_sweeps=200)
    assert not ok and sweeps == 200 and beta[1] > 100.0  # ten arcs of mass one round state 1: log 10 a sweep
    beta, sweeps, ok = P.backward(d, arc, fin, P.MAX)
    assert ok and sweeps == 2 and beta.tolist() == [0.0, 0.0]


def test_closed_form_of_one_state():
    """A self-loop of probability 1/2 and a final probability of 1/2: beta = log(1/2 + 1/4 + ...) = 0."""
    d = np.full((1, 256), -1, np.int32)
    d[0, 97] = 0
    arc = np.full((1, 256), -np.inf, np.float32)
    arc[0, 97] = np.log(0.5)
    fin = np.array([np.log(0.5)], np.float32)
    beta, sweeps, ok = P.backward(d, arc, fin, P.LOG)
    assert ok and abs(float(beta[0])) < 5e-6 and 15 <= sweeps <= 24  # 2^-k falls below 2^-20 after about twenty sweeps
    # (in float64 what is left is the rounding of the two float32 inputs: half an ulp of 0.69 each, 3e-8)
    assert abs(float(P.fixed_point64(d, arc, fin, P.LOG)[0])) < 1e-7
    a, f = P.push(d, arc, fin, beta)
    assert abs(np.exp(a[0, 97]) + np.exp(f[0]) - 1.0) < 1e-5 and np.isneginf(np.delete(a[0], 97)).all()


def _logsumexp(x):
    m = x.max()
    return m + np.log(np.exp(x - m).sum())


@pytest.mark.parametrize("name", NAMES)
def test_a_pushed_automaton_is_normalised_and_keeps_the_paths(name):
    d, acc, start = R.automata()[name]
    arc, fin = P.substochastic_weights(d, acc, 7)
    live = R.live(np.asarray(d, np.int64), acc)
    wf = ByteWFSA(d, arc, fin, start)
    strings = P.accepted_strings(d, acc, start, 3)
    assert len(strings) >= 5 and all(wf.accepts(s) for s in strings)
    for semiring in (P.LOG, P.MAX):
        beta, _, ok = P.backward(d, arc, fin, semiring)
        a, f = P.push(d, arc, fin, beta)
        assert ok and a.dtype == f.dtype == np.float32 and not np.isnan(a).any() and not np.isnan(f).any()
        for s in range(len(acc)):
            row = np.append(a[s], f[s])
            if not live[s]:
                assert np.isneginf(row).all()
            elif semiring == P.LOG:
                assert abs(_logsumexp(row.astype(np.float64))) < 1e-5, (name, s)
            else:
                assert row.max().tobytes() == np.float32(0.0).tobytes(), (name, s)  # (+0.0f: x - x)
        pushed = ByteWFSA(d, a, f, start)  # (arcs into states that are not live weigh -inf and leave delta)
        assert np.array_equal(pushed.live, wf.live) and np.array_equal(pushed.accepting, wf.accepting)
        for s in strings:
            assert abs(float(pushed.path_logw(s)) - (float(wf.path_logw(s)) - float(beta[start]))) < 1e-5, (name, semiring, s)
