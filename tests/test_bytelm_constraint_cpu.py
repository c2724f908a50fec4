"""A byte beam under a byte automaton without a GPU: the float64 restatement (tests/bytelm_constraint_ref.py)
against brute force over tokenisations, the argument block against the header, and the constructor's refusals."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import bytelm_constraint_ref as CR
from tests import bytelm_ref as R

LANGUAGE = {b"ab": -0.5, b"abc": 0.25, b"b": -1.5, b"ca": 0.0, b"cab": -0.75}


def _automata():
    from genlm_backend_amd.constraints import ByteDFA, ByteWFSA

    dfa = ByteDFA.from_strings(LANGUAGE)
    wfsa = ByteWFSA.from_weighted_strings(LANGUAGE)
    arc = wfsa.arc_logw.copy()
    arc[wfsa.start, ord("a")] = -0.3  # weights on arcs too: a string's weight is the sum along its path
    arc[int(wfsa.delta[wfsa.start, ord("c")]), ord("a")] = 0.7
    return dfa, ByteWFSA(wfsa.delta, arc, wfsa.final_logw, wfsa.start)


@pytest.mark.parametrize("weighted", [False, True])
def test_the_restatement_against_brute_force_over_tokenisations(weighted):
    vocab, lm = R.SMALL_VOCAB, R.hashed_lm(len(R.SMALL_VOCAB), salt=33)
    automaton = _automata()[weighted]
    weight = (lambda s: float(automaton.path_logw(s))) if weighted else (lambda s: 0.0)
    prefixes = sorted({s[:i] for s in LANGUAGE for i in range(len(s) + 1)})
    P = {x: R.brute_force(lm, vocab, 0, x) for x in sorted(set(prefixes) | {x + bytes([b]) for x in prefixes for b in b"abc"})}
    want_total = sum(P[s][1] * math.exp(weight(s)) for s in LANGUAGE)

    def walk(x):  # the automaton's state and weight after the bytes x
        s, w = automaton.start, 0.0
        for b in x:
            w += float(automaton.arc_logw[s, b]) if weighted else 0.0
            s = int(automaton.delta[s, b])
        return s, w

    # the constrained next-byte distribution after every prefix of the language
    for x in prefixes:
        ref = CR.RefConstrainedBeam(lm, vocab, [0], 64, automaton)
        for b in x:
            ref.advance(b)
        s, w = walk(x)
        assert ref.state == s and abs(ref.log_weight - w) <= 1e-9 and abs(ref.logp - math.log(P[x][0])) <= 1e-9
        num = np.zeros(257)
        for b in b"abc":
            if any(t.startswith(x + bytes([b])) for t in LANGUAGE):
                num[b] = P[x + bytes([b])][0] * math.exp(float(automaton.arc_logw[s, b]) if weighted else 0.0)
        if x in LANGUAGE:
            num[256] = P[x][1] * math.exp(float(automaton.final_logw[s]) if weighted else 0.0)
        got, logZc = ref.next_byte_logprobs(), ref.next_byte_logZ()
        assert not ref.pruned
        assert ((got == -np.inf) == (num == 0)).all(), x
        assert np.abs(np.exp(got) - num / num.sum()).max() <= 1e-9, x
        assert abs(math.exp(logZc) - num.sum() / P[x][0]) <= 1e-9, x

    # the total: read every string (given bytes: the automaton's weights), and draw every string (the weights are the Zc's)
    read = drawn = 0.0
    for text in LANGUAGE:
        ref = CR.RefConstrainedBeam(lm, vocab, [0], 64, automaton)
        for b in list(text) + [256]:
            ref.advance(b)
        assert ref.ended and ref.state == -1 and not ref.pruned
        assert abs(ref.log_weight - weight(text)) <= 1e-6  # (path_logw sums in float32)
        read += math.exp(ref.logp + ref.log_weight)
        ref = CR.RefConstrainedBeam(lm, vocab, [0], 64, automaton)
        q = 0.0  # the log-probability with which the sampler draws this text
        for b in list(text) + [256]:
            row = ref.next_byte_logprobs()
            cum = CR.cdf(row)
            q += row[b]
            assert ref.step((cum[b] - math.exp(row[b]) / 2)) == b  # the midpoint of the byte's interval
        assert ref.ended and not ref.pruned and ref.step(0.5) == -1
        drawn += math.exp(q + ref.log_weight)
    assert abs(read - want_total) <= 1e-9 and abs(drawn - want_total) <= 1e-9

    # a forbidden byte kills; a dead group stays dead, no NaN
    ref = CR.RefConstrainedBeam(lm, vocab, [0], 64, automaton)
    ref.advance(ord("b"))
    ref.advance(ord("b"))
    assert ref.state == -1 and ref.log_weight == -np.inf and not ref.ended and not np.isnan(ref.logp)
    assert (ref.next_byte_logprobs() == -np.inf).all() and ref.next_byte_logZ() == -np.inf and ref.step(0.3) == -1


def test_pick_is_the_first_column_past_the_uniform():
    row = np.full(257, -np.inf)
    row[[3, 200, 256]] = np.log([0.25, 0.5, 0.25])
    assert [CR.pick(row, u) for u in (0.0, 0.2499, 0.25, 0.74, 0.75, 0.9999)] == [3, 3, 200, 200, 256, 256]
    assert CR.pick(row, 1.0) == 256 and CR.pick(np.full(257, -np.inf), 0.5) == -1  # the fallback: the last finite column


def test_the_step_block_agrees_with_the_header_and_the_library_exports_the_call():
    import genlm_backend_amd  # noqa: F401
    from genlm_backend_amd import _lib

    lib = _lib.load()
    assert lib.glb_bytelm_step(None, None) == _lib.GLB_EINVAL
    fields = ("peek", "beam", "n_states", "delta", "accepting", "live", "arc_logw", "final_logw", "state", "ended", "log_weight",
              "uniform", "seed", "offset", "out_byte", "out_row", "out_logZc")
    src = ('#include "glb.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) { printf("%zu %zu", sizeof(glb_bytelm_step_args), '
           'sizeof(glb_bytelm_args));\n' + "".join(f'printf(" %zu", offsetof(glb_bytelm_step_args, {f}));\n' for f in fields)
           + 'printf("\\n"); return 0; }\n')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got == [C.sizeof(_lib.ByteLmStepArgs), C.sizeof(_lib.ByteLmArgs)] + [getattr(_lib.ByteLmStepArgs, f).offset for f in fields]

    def block(**kw):
        p = _lib.ByteLmStepArgs()
        p.struct_size, p.n_states = C.sizeof(_lib.ByteLmStepArgs), 7
        p.beam.struct_size = C.sizeof(_lib.ByteLmArgs)
        p.beam.width, p.beam.n_groups, p.beam.n_nodes, p.beam.root = 4, 2, 10, 9
        for f, _ in _lib.ByteLmArgs._fields_:
            if f not in ("struct_size", "width", "n_groups", "n_nodes", "root", "fresh", "byte"):
                setattr(p.beam, f, 4096 + 64 * len(f))  # any non-null value: nothing may be read
        for f in ("delta", "accepting", "live", "state", "ended", "log_weight", "out_byte", "out_logZc"):
            setattr(p, f, 8192 + 64 * len(f))
        for k, v in kw.items():
            if k.startswith("beam_"):
                setattr(p.beam, k[5:], v)
            else:
                setattr(p, k, v)
        return p

    bad = [dict(struct_size=8), dict(beam_struct_size=8), dict(beam_width=0), dict(beam_width=65), dict(beam_n_groups=0),
           dict(beam_root=10), dict(beam_node=None), dict(beam_alive=None), dict(beam_sel=None), dict(beam_u=None), dict(beam_w=None),
           dict(beam_mass=None), dict(beam_logp=None), dict(n_states=0), dict(n_states=-3), dict(n_states=1 << 24), dict(delta=None),
           dict(accepting=None), dict(live=None), dict(arc_logw=4096), dict(final_logw=4096), dict(state=None), dict(ended=None),
           dict(log_weight=None), dict(out_byte=None), dict(out_logZc=None), dict(out_byte=None, uniform=4096)]
    for kw in bad:
        assert lib.glb_bytelm_step(C.byref(block(**kw)), None) == _lib.GLB_EINVAL, kw
    assert "come together" in (lib.glb_bytelm_step(C.byref(block(arc_logw=4096)), None), _lib.last_error())[1]


def test_a_constraint_is_refused_by_kind_before_any_device_is_touched():
    from genlm_backend_amd import ByteBeam, ByteSIS
    from genlm_backend_amd.constraints import ByteDFA, ByteNFA, BytePDA

    ok = [b"<eos>", b"a", b"b"]
    with pytest.raises(ValueError, match="got a object"):
        ByteBeam(None, ok, [0], constraint=object())
    with pytest.raises(ValueError, match="ByteNFA.*determinize"):
        ByteBeam(None, ok, [0], constraint=ByteNFA.from_regex(rb"a+b"))
    with pytest.raises(ValueError, match="got a BytePDA.*determinize"):
        ByteBeam(None, ok, [0], constraint=BytePDA.from_dfa(ByteDFA.from_strings([b"ab"])))
    with pytest.raises(ValueError, match="needs an automaton"):
        ByteSIS(None, 4, None, ok, [0])
    with pytest.raises(ValueError, match="got a str"):
        ByteSIS(None, 4, "a+b", ok, [0])
