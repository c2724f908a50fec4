"""Scoring given sequences without a GPU: the layout of `glb_score_args`, the argument errors of glb_score_rows (they return
before any launch), and the host logic of `batch_sequence_logprobs_sync` against a stand-in engine that scores with the
float64 reference (tests/score_engine.py, tests/score_ref.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import dfa_ref
from tests import score_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_score_args_layout_matches_the_header(tmp_path):
    from genlm_backend_amd import _lib

    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "glb.h"\nint main(void) { printf("%zu %zu %d\\n", '
                   'sizeof(glb_score_args), offsetof(glb_score_args, out_seq_logp_masked), GLB_ABI_VERSION); return 0; }\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "size")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "size")]).split()]
    assert out == [C.sizeof(_lib.ScoreArgs), _lib.ScoreArgs.out_seq_logp_masked.offset, 9]
    assert _lib.ABI_VERSION == 9
    lib = _lib.load()
    assert lib.glb_abi_version() == 9
    for name in ("glb_score_rows", "glb_score_seq_sums"):
        assert name in _lib.SYMBOLS and getattr(lib, name)


def _valid_block(_lib):
    """An argument block that passes every check (these tests stop before a launch: the pointers are never followed)."""
    a = _lib.ScoreArgs()
    a.struct_size = C.sizeof(_lib.ScoreArgs)
    a.logits, a.dtype, a.ld = 0x10000, _lib.F32, 64
    a.n_rows, a.vocab, a.logit_scale = 2, 50, 1.0
    a.token = 0x20000
    return a


def test_score_rows_rejects_bad_arguments_before_any_launch():
    from genlm_backend_amd import _lib

    lib = _lib.load()
    call = lambda a: lib.glb_score_rows(C.byref(a), None)
    assert lib.glb_score_rows(None, None) == _lib.GLB_EINVAL
    bad = [("struct_size", 1, "struct_size"), ("logits", 0, "logits is null"), ("token", 0, "token is null"), ("dtype", 3, "dtype"),
           ("dtype", -1, "dtype"), ("n_rows", 0, "positive"), ("vocab", 0, "positive"), ("n_rows", -1, "positive"),
           ("vocab", 1 << 31, "31 bits"), ("n_rows", 1 << 31, "31 bits"), ("ld", 49, "ld"), ("logits", 0x10002, "aligned"),
           ("logit_scale", float("nan"), "NaN"), ("logit_scale", 0.0, "positive and finite"),
           ("logit_scale", -1.0, "positive and finite"), ("logit_scale", float("inf"), "positive and finite"), ("mask_kind", _lib.MASK_PREPARED, "GLB_MASK_PREPARED"), ("mask_kind", 4, "mask_kind"),
           ("mask_kind", -1, "mask_kind"), ("out_seq_logp", 0x30000, "without seq_start"),
           ("out_seq_logZ", 0x30000, "without seq_start"), ("out_seq_logp_masked", 0x30000, "without seq_start")]
    for field, value, word in bad:
        a = _valid_block(_lib)
        setattr(a, field, value)
        if field == "vocab" and value > 64:
            a.ld = value
        assert call(a) == _lib.GLB_EINVAL, field
        assert word in _lib.last_error(), (field, _lib.last_error())
    # with a mask: the table, its pitch, the ids
    a = _valid_block(_lib)
    a.mask_kind = _lib.MASK_BITS
    assert call(a) == _lib.GLB_EINVAL and "mask table missing" in _lib.last_error()
    a.mask, a.n_masks, a.mask_ld = 0x60000, 3, 1
    assert call(a) == _lib.GLB_EINVAL and "mask_ld" in _lib.last_error()
    a.mask_ld = 2
    assert call(a) == _lib.GLB_EINVAL and "neither 1 nor" in _lib.last_error()
    a.mask = 0x60002
    a.n_masks = 2
    assert call(a) == _lib.GLB_EINVAL and "misaligned" in _lib.last_error()
    a.mask, a.mask_kind, a.mask_ld = 0x60000, _lib.MASK_F32, 49
    assert call(a) == _lib.GLB_EINVAL and "mask_ld" in _lib.last_error()
    a.n_masks, a.mask_ld = 0, 50
    assert call(a) == _lib.GLB_EINVAL and "mask table missing" in _lib.last_error()
    # sequence sums
    a = _valid_block(_lib)
    a.seq_start, a.n_seq = 0x70000, -1
    assert call(a) == _lib.GLB_EINVAL and "n_seq" in _lib.last_error()
    a.n_seq, a.out_seq_logZ = 2, 0x80000
    assert call(a) == _lib.GLB_EINVAL and "per-row output" in _lib.last_error()
    assert lib.glb_score_seq_sums(None, 1, None, 1, None, None) == _lib.GLB_EINVAL
    assert lib.glb_score_seq_sums(0x10000, -1, 0x20000, 1, 0x30000, None) == _lib.GLB_EINVAL


# ---- the reference's own identities --------------------------------------------------------------------------------------------
def test_reference_rows():
    x = np.array([[0.0, 1.0, -np.inf, 2.0], [-np.inf] * 4], np.float32)
    bits = np.array([[0b0110], [0]], np.uint32)
    r = SR.score_rows(x, [3, 0], 1.0, 1, bits, [0, 0])
    l = np.log(1 + np.e + np.e ** 2)
    assert abs(r[0, 1] - l) < 1e-12 and abs(r[0, 0] - (2 - l)) < 1e-12 and abs(r[0, 2] - (1 - l)) < 1e-12 and r[0, 3] == -np.inf
    assert np.all(np.isneginf(r[1]))
    assert np.all(np.isneginf(SR.score_rows(x[:1], [4], 1.0)[0, [0, 3]])) and np.all(np.isneginf(SR.score_rows(x[:1], [-1], 1.0)[0, [0, 3]]))
    assert np.all(np.isneginf(SR.score_rows(x[:1], [1], 1.0, 1, bits, [7])[0, 2:]))
    s = SR.seq_sums(np.array([1, 2, -np.inf, 4], np.float32), [0, 0, 2, 3, 4, 4])
    assert s.tolist() == [0.0, 3.0, -np.inf, 4.0, 0.0]


# ---- host logic against the stand-in engine ------------------------------------------------------------------------------------
def _llm(score_chunk_bytes=1 << 30, V=300):
    import genlm_backend_amd  # noqa: F401
    from genlm_backend_amd.llm import AsyncAmdLM
    from tests.score_engine import ScoreEngine
    from transformers import GPT2Config, GPT2LMHeadModel

    torch.manual_seed(0)
    m = GPT2LMHeadModel(GPT2Config(vocab_size=V, n_positions=64, n_embd=32, n_layer=2, n_head=2, bos_token_id=0, eos_token_id=0)).eval()
    return AsyncAmdLM(m, None, batch_size=64, engine=ScoreEngine(), score_chunk_bytes=score_chunk_bytes)


PROMPTS = [[5], [6, 7, 8], [9, 10], [11, 12, 13, 14, 15, 16], [17, 3]]
CONTS = [[20, 21, 22], [], [30], [40, 41, 42, 43, 44, 45, 46], [50, 51]]


def _direct(llm, prompt, cont):
    """log-softmax rows of the model itself over prompt + cont, float64: the score of cont[t] is row P - 1 + t at cont[t]."""
    with torch.no_grad():
        logits = llm.model(input_ids=torch.tensor([prompt + cont])).logits[0].double()
    lp = torch.log_softmax(logits, -1)
    return [float(lp[len(prompt) - 1 + t, c]) for t, c in enumerate(cont)]


def test_ragged_pairs_gather_the_right_hidden_rows():
    llm = _llm()
    s = llm.batch_sequence_logprobs_sync(PROMPTS, CONTS)
    assert s.starts.tolist() == [0, 3, 3, 4, 11, 13] and len(s) == 5 and s.token_logZ is None
    got = s.tolist()
    for i, (p, c) in enumerate(zip(PROMPTS, CONTS)):
        want = _direct(llm, p, c)
        assert len(got[i]) == len(c)
        assert np.allclose(got[i], want, atol=2e-5, rtol=0), (i, got[i], want)
        assert abs(float(s.logprobs[i]) - sum(want)) < 2e-5 * max(1, len(c))
    assert float(s.logprobs[1]) == 0.0  # an empty continuation
    assert llm.engine.score_calls == [13]  # one chunk


def test_prompt_rules_and_the_single_pair_form():
    import asyncio

    llm = _llm()
    with pytest.raises(ValueError, match="at least one token"):
        llm.batch_sequence_logprobs_sync([[1], []], [[2], [3]])
    with pytest.raises(ValueError, match="2 prompts for 1"):
        llm.batch_sequence_logprobs_sync([[1], [2]], [[2]])
    with pytest.raises(ValueError, match="temperature"):
        llm.batch_sequence_logprobs_sync([[1]], [[2]], temperature=0.0)
    one = asyncio.run(llm.sequence_logprobs([5], [20, 21, 22]))  # a one-token prompt
    many = asyncio.run(llm.batch_sequence_logprobs(PROMPTS, CONTS))
    assert torch.equal(one.token_logprobs, many.token_logprobs[:3])
    empty = llm.batch_sequence_logprobs_sync([[4, 5]], [[]])
    assert empty.token_logprobs.numel() == 0 and empty.logprobs.tolist() == [0.0] and empty.tolist() == [[]]
    assert len(llm.batch_sequence_logprobs_sync([], [])) == 0


def test_chunk_boundaries_inside_a_sequence_change_nothing():
    whole = _llm().batch_sequence_logprobs_sync(PROMPTS, CONTS, temperature=2.0)
    llm = _llm(score_chunk_bytes=2 * 300 * 4)  # two rows' worth of float32 logits
    cut = llm.batch_sequence_logprobs_sync(PROMPTS, CONTS, temperature=2.0)
    assert llm.engine.score_calls == [2, 2, 2, 2, 2, 2, 1]
    assert torch.equal(whole.token_logprobs, cut.token_logprobs) and torch.equal(whole.logprobs, cut.logprobs)
    with torch.no_grad():
        logits = llm.model(input_ids=torch.tensor([PROMPTS[0] + CONTS[0]])).logits[0].double()
    want = torch.log_softmax(logits / 2, -1)[0, CONTS[0][0]]
    assert abs(float(cut.token_logprobs[0]) - float(want)) < 2e-5
    assert _llm(score_chunk_bytes=1 << 40).score_chunk_bytes == 16 << 30  # never above logprob_budget_bytes


def test_constraint_walk_gives_minus_inf_from_the_first_forbidden_token_on():
    from tests.score_engine import ByteDFAConstraint

    vocab, eos_id, skip = dfa_ref.synth_vocab(300, seed=3)
    delta, acc, start = dfa_ref.automata()["digits"]
    ref = dfa_ref.Ref(delta, acc, start, vocab, eos_id, skip)
    d = lambda ch: ord(ch)  # single-byte tokens are their byte values
    prompts = [[1, 2], [3], [4, 5, 6], [7]]
    conts = [[d("1"), d("2"), d("3")], [d("4"), d("a"), d("5"), d("6")], [], [d("x")]]
    llm = _llm()
    con = ByteDFAConstraint(ref)
    s = llm.batch_sequence_logprobs_sync(prompts, conts, constraint=con)
    assert con.checked == 1 and con.mask_rows_calls == 4  # one per position of the longest continuation
    plain = _llm().batch_sequence_logprobs_sync(prompts, conts)
    assert torch.equal(s.token_logprobs, plain.token_logprobs) and torch.isfinite(s.token_logprobs).all()
    lpm, lz = s.tolist("token_logprobs_masked"), s.tolist("token_logZ")
    assert all(np.isfinite(v) for v in lpm[0] + lz[0]) and np.isfinite(float(s.logprobs_masked[0]))
    assert np.isfinite(lpm[1][0]) and all(v == -np.inf for v in lpm[1][1:]) and float(s.logprobs_masked[1]) == -np.inf
    assert np.isfinite(lz[1][1]) and lz[1][2] == -np.inf and lz[1][3] == -np.inf  # (a dead state allows nothing)
    assert lpm[2] == [] and float(s.logprobs_masked[2]) == 0.0 and float(s.logZ[2]) == 0.0
    assert lpm[3] == [-np.inf]
    # the values: the reference fed with the masks of the reference walk
    for i, (p, c) in enumerate(zip(prompts, conts)):
        with torch.no_grad():
            logits = llm.model(input_ids=torch.tensor([p + c])).logits[0].numpy() if c else None
        st = ref.start
        for t, tok in enumerate(c):
            m = SR.mask_values(1, ref.mask(st) if st >= 0 else ref.row_dead(), 300)
            want = SR.score_row(logits[len(p) - 1 + t], tok, 1.0, m)
            assert np.allclose([lz[i][t], lpm[i][t]], [want[2], want[3]], atol=2e-5, rtol=0, equal_nan=False), (i, t)
            st = ref.next(st, tok)


def test_a_sequence_made_to_end_is_scored_against_the_row_of_a_finished_one():
    """forced_at: the token at that place meets the EOS-only row (state accepting) or the empty row, not the state's own."""
    from tests.score_engine import ByteDFAConstraint

    vocab, eos_id, skip = dfa_ref.synth_vocab(300, seed=3)
    delta, acc, start = dfa_ref.automata()["digits"]
    ref = dfa_ref.Ref(delta, acc, start, vocab, eos_id, skip)
    llm = _llm()
    tok = torch.tensor([[1, 2, ord("1"), ord("2"), eos_id], [3, 4, ord("7"), eos_id, 0], [5, 6, eos_id, 0, 0]], dtype=torch.int32)
    lengths, plen = torch.tensor([5, 4, 3], dtype=torch.int32), torch.tensor([2, 2, 2], dtype=torch.int32)
    free = llm.batch_sequence_logprobs_device(tok, lengths, plen, constraint=ByteDFAConstraint(ref))
    forced = llm.batch_sequence_logprobs_device(tok, lengths, plen, constraint=ByteDFAConstraint(ref),
                                                forced_at=torch.tensor([2, -1, 0], dtype=torch.int32))
    fz, zz = free.tolist("token_logZ"), forced.tolist("token_logZ")
    assert zz[0][:2] == fz[0][:2] and zz[1] == fz[1]  # elsewhere nothing changes
    assert zz[0][2] < fz[0][2]  # EOS alone has less mass than the accepting state's whole row
    with torch.no_grad():
        logits = llm.model(input_ids=tok[:1, :5].long()).logits[0].numpy()
    want = SR.score_row(logits[3], eos_id, 1.0, SR.mask_values(1, ref.row_eos(), 300))
    assert abs(zz[0][2] - want[2]) < 2e-5 and forced.tolist("token_logprobs_masked")[0][2] == 0.0
    assert zz[2] == [-np.inf]  # the start state does not accept: made to end there, nothing is allowed
    with pytest.raises(ValueError, match="needs a constraint"):
        llm.batch_sequence_logprobs_device(tok, lengths, plen, forced_at=torch.tensor([2, -1, 0], dtype=torch.int32))
